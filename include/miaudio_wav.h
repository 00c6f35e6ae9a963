/*
 * miaudio_wav.h — WAV ingestion on the device (part of libmiaudio.so): the per-sample work of turning the `data`
 * chunks of .wav files into the peak-normalised mono f32 clips the data modules read.  Replaces what the reference's
 * scripts/prepare_esc50.py does per file on the host (torchaudio.load(normalize=True), torch.mean(dim=0),
 * waveform / waveform.abs().max()).  The container (RIFF chunk walk, format tags) is parsed on the host
 * (src/datasets/wav.py); these entry points see only sample bytes.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains), no host synchronisation.
 */
#ifndef MIAUDIO_WAV_H
#define MIAUDIO_WAV_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample formats of MiaWavClip.format, all little-endian. */
enum {
  MIA_PCM_U8 = 0,  /* (x - 128) / 128 */
  MIA_PCM_S16 = 1, /* x / 2^15 */
  MIA_PCM_S24 = 2, /* 3 packed bytes, sign-extended; x / 2^23 */
  MIA_PCM_S32 = 3, /* (float)x rounded to nearest even, then * 2^-31 */
  MIA_PCM_F32 = 4, /* as it is */
  MIA_PCM_F64 = 5  /* rounded to nearest even to f32 */
};
#define MIA_WAV_MAX_CHANNELS 8

/* One clip of a staged group (a device table entry, 24 bytes): `frames` interleaved frames of `channels` samples
 * of `format` start at bytes + byte_off. */
typedef struct MiaWavClip {
  int64_t byte_off;
  int64_t frames;
  int32_t channels;
  int32_t format;
} MiaWavClip;

/* Decode + downmix + peak.  Clip i's mono output is out[out_offsets[i] .. out_offsets[i] + frames_i):
 *   mono[t] = (s[t][0] + s[t][1] + ... in channel order, in f32) / (float)channels     (one IEEE division; none
 *   for one channel), s = the decoded sample per the table above (torchaudio's normalize=True convention).
 * peak_bits[i] = the f32 bits of max |mono[t]| over the finite mono samples (0 for an empty or silent clip),
 * nonfinite[i] = the number of NaN / Inf mono samples.  Both arrays (n_clips uint32 each) are zeroed on the stream
 * by this call; each workgroup folds its part in registers and LDS and issues one unsigned atomicMax (and one
 * atomicAdd where it counted something) per clip, so the results do not depend on the order of arrival.
 * Safety: byte_off and out_offsets may have any alignment (out itself 4-B aligned).  Every load lies inside
 * [bytes + byte_off, bytes + byte_off + frames * channels * bytes_per_sample) of its own clip -- a lane whose four
 * frames lie whole inside it at a 4-B aligned address loads them as one span of up to 16-B loads, every other lane
 * assembles its span from aligned dwords that lie whole inside the clip and single bytes at the clip's two ends --
 * and nothing outside a clip's output range is written (16-B stores where the address allows, element stores at
 * the range's misaligned head and tail; the same bits either way).  All index arithmetic is 64-bit.  Clips of
 * different formats and channel counts share the launch.  frames = 0 writes nothing.  The table lives on the
 * device and is not read by the launcher: the caller validates its host copy (kernels.pcm_decode does); a clip
 * whose channels are outside 1..MIA_WAV_MAX_CHANNELS, whose format is unknown or whose frames are negative is
 * skipped by the kernel (nothing read, nothing written).
 * Traffic: the clips' file bytes + 4 B per output sample.  n_clips >= 0; no null pointer; clips and out_offsets
 * 8-B aligned. */
int mia_pcm_decode(const uint8_t* bytes, const MiaWavClip* clips, int64_t n_clips, const int64_t* out_offsets,
                   float* out, uint32_t* peak_bits, uint32_t* nonfinite, mia_stream_t stream);

/* The same peak and non-finite count over a flat f32 store: clip i = store[offsets[i] .. offsets[i+1])
 * (offsets: n_clips + 1 device int64, 8-B aligned; store 4-B aligned).  Needed after a resample.
 * Traffic: 4 B per sample. */
int mia_clip_peak(const float* store, const int64_t* offsets, int64_t n_clips, uint32_t* peak_bits,
                  uint32_t* nonfinite, mia_stream_t stream);

/* In place x / peak_i (a correctly rounded f32 division) over clip i where peak_i > 0; a clip whose peak is 0 is
 * left untouched (the reference's `if max_val > 0`).  peak_bits as written by the two calls above.
 * Traffic: 8 B per sample. */
int mia_clip_scale(float* store, const int64_t* offsets, int64_t n_clips, const uint32_t* peak_bits,
                   mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_WAV_H */
