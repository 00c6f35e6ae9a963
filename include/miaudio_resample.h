/*
 * miaudio_resample.h — band-limited sinc resampling of a waveform batch (part of libmiaudio.so).
 *
 * Replaces torchaudio.transforms.Resample on the data path of the reference (resample_waveform,
 * src/datasets/preprocessing.py:61-76, the first step of EnvNetPreprocessor.preprocess :822 and
 * ASTPreprocessor.preprocess :1021).  With o = orig / gcd and n = new / gcd the transform is a strided FIR bank:
 * n phases of K = 2 * width + o taps each, applied every o input samples.  The taps are built on the host
 * (src/datasets/resample.py) and passed in; this file only applies them.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).
 */
#ifndef MIAUDIO_RESAMPLE_H
#define MIAUDIO_RESAMPLE_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Limits of mia_resample: K = 2 * width + o and n up to these, B up to 65535.  Every pair among 8, 11.025, 16,
 * 22.05, 24, 32, 44.1, 48, 96 and 192 kHz at torchaudio's default filter width stays below K = 694, n = 640. */
#define MIA_RESAMPLE_MAX_TAPS 4096
#define MIA_RESAMPLE_MAX_PHASES 4096
#define MIA_RESAMPLE_MAX_BATCH 65535

/* ceil(n * T / o): the samples a clip of T samples has after resampling by n / o.  Negative for T < 0, o < 1
 * or n < 1. */
int64_t mia_resample_out_len(int64_t T, int32_t o, int32_t n);

/* x: B rows of T f32 samples, row stride ldx >= T.  lengths: B device int32, or NULL; the clip of row b is its
 * first L_b = clamp(lengths[b], 0, T) samples (T without lengths) and xz_b is that clip with zeros on both sides;
 * nothing outside [0, L_b) of a row is read.  taps: f32 [n][K], K = 2 * width + o.  o and n are coprime.
 * out: B rows, row stride ldo >= Tout, Tout == mia_resample_out_len(T, o, n).  For m = f * n + j, j < n, m < Tout:
 *   out[b * ldo + m] = sum_{k < K} xz_b[f * o + k - width] * taps[j * K + k]   if m < ceil(n * L_b / o)
 *                    = +0.0f                                                     otherwise.
 * Every element of [0, Tout) of every row is written; columns [Tout, ldo) are not touched.  No workspace.
 * Operands and sums are f32 (v_mfma_f32_32x32x2_f32: fused multiply-adds, k ascending), in a fixed order: two
 * runs give the same bits.  Row offsets are 64-bit.  Bad arguments (a NULL buffer, o and n not coprime, K or n
 * or B over the limits above, a Tout other than mia_resample_out_len's, ldx < T, ldo < Tout) return a negative
 * code before any launch; B == 0 or T == 0 is a successful no-op. */
int mia_resample(const float* x, int64_t ldx, int32_t B, int64_t T, const int32_t* lengths,
                 const float* taps, int32_t o, int32_t n, int32_t width,
                 float* out, int64_t ldo, int64_t Tout, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_RESAMPLE_H */
