/*
 * miaudio_data.h — the data path of a device-resident dataset (part of libmiaudio.so): every clip of a dataset sits
 * in one flat f32 store in HBM and a batch is cut out of it on the device.  Replaces the reference's per-item host
 * work in EnvNetPreprocessor (src/datasets/preprocessing.py): the zero padding of `pad` samples each side (:825),
 * the right-padding of a clip shorter than the window (:842-845) and the crop itself (:855, :881).  For the
 * spectrogram path, which has no window, mia_fit_gather makes every clip one length (src/utils/audio.py::pad_or_trim).
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).
 */
#ifndef MIAUDIO_DATA_H
#define MIAUDIO_DATA_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Clip i occupies store[offsets[i] .. offsets[i+1]) (offsets: n_clips + 1 device int64).  For i = idx[b] and
 * len = offsets[i+1] - offsets[i]:
 *   out[c][b][t] = clip[s],  s = start[b][c] + t - pad,  where 0 <= s < len
 *   out[c][b][t] = +0.0f     everywhere else
 * A copied sample keeps its bits (NaN payloads, -0.0).  idx, start and offsets live on the device and are never
 * validated by the launcher: the kernel addresses store only through an s that passed 0 <= s < len, so no load
 * leaves [offsets[i], offsets[i+1]) whatever start holds (negative, huge); a row whose idx is outside
 * [0, n_clips) or whose len <= 0 is all zeros.  All index arithmetic is 64-bit (a store may exceed 2^31 elements).
 * Writes every element of out ([ncrop][B][window] f32, contiguous) and nothing else: 16-B stores where a row's
 * address allows, element stores for a row's misaligned head and tail -- the same bits either way.
 * Traffic: 8 B per output sample.  B, ncrop, window >= 1; pad >= 0; no null pointer. */
int mia_crop_gather(const float* store, const int64_t* offsets, int64_t n_clips, const int32_t* idx,
                    const int32_t* start, int32_t B, int32_t ncrop, int32_t pad, int32_t window, float* out,
                    mia_stream_t stream);

/* Clip-length fitting for the spectrogram path: every clip of a batch made exactly `length` samples long, the rule
 * of the reference's src/utils/audio.py::pad_or_trim ("pad wrap or trim").  For i = idx[b] and
 * n = offsets[i+1] - offsets[i]:
 *   n >= length:                    out[b][t] = clip[(n - length) / 2 + t]   (centred trim; the clip when n == length)
 *   0 < n < length, MIA_FIT_WRAP:   out[b][t] = clip[t mod n]                (= wav.repeat(ceil(length / n))[:length])
 *   0 < n < length, MIA_FIT_ZERO:   out[b][t] = clip[t] for t < n, +0.0f behind it
 *   n <= 0, or i outside [0, n_clips): out[b][t] = +0.0f   (the reference divides by zero on an empty clip)
 * Otherwise as mia_crop_gather: samples move as 32-bit words and keep their bits; idx and offsets are never
 * validated by the launcher and no load leaves [offsets[i], offsets[i+1]); index arithmetic against the store is
 * 64-bit (the wrap remainder, taken only when n < length <= INT32_MAX, is 32-bit: one per 16-B group); writes every
 * element of out ([B][length] f32, contiguous) and nothing else, by 16-B stores where a row's address allows.
 * Traffic: 8 B per output sample.  B, length, n_clips >= 1; mode one of the two below; no null pointer; store and
 * out 4-B aligned. */
#define MIA_FIT_WRAP 0
#define MIA_FIT_ZERO 1
int mia_fit_gather(const float* store, const int64_t* offsets, int64_t n_clips, const int32_t* idx, int32_t B,
                   int32_t length, int32_t mode, float* out, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_DATA_H */
