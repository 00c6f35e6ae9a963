/*
 * miaudio_rowmap.h — the two elementwise producers of a (1, 2)-conv backward's gradient, storing through a row
 * map (part of libmiaudio.so).
 *
 * The backward of a (1, 2) conv reads its output gradient laid on the INPUT grid: one zero pixel, then every row
 * of the gradient followed by one zero column (mia_pad_w2's layout, miaudio.h).  These entry points are
 * mia_pool_bn_relu_bwd_apply_ex (miaudio_pool.h) and mia_bn_relu_bwd_apply (miaudio.h) writing dx in such a layout
 * themselves, so the copy pass is not needed.  The row map:
 *
 *   - dx pixel lead + r * row_pixels + x receives what the dense form writes at pixel r * w + x
 *     (r = source row: b * h + iy of the pooled form, r of the (rows, w) view of the BN form; 0 <= x < w);
 *   - the `lead` pixels before row 0 are written as zeros;
 *   - pixels w .. row_pixels - 1 of every row are written as zeros (row_pixels >= w);
 *   - zero_pixel (optional, zc elements of dtype, zc % 8 == 0, 16-byte aligned) is zeroed in the same launch.
 *
 * dx therefore holds lead + rows * row_pixels pixels of c channels, every one written, and nothing outside them
 * is touched.  lead = 0, row_pixels = w, zc = 0 is the dense form, byte for byte.  Arithmetic, grids, dbias and
 * the rows of `partial` are those of the dense forms.  With a map, dx must not alias the input gradient.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).
 */
#ifndef MIAUDIO_ROWMAP_H
#define MIAUDIO_ROWMAP_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mia_pool_bn_relu_bwd_apply_ex through a row map.  A map other than the dense one is served by the kw-pixel-run
 * form alone: dtype MIA_BF16, kw in 2..4 (any kh), x and dx 16-byte aligned; every other geometry is refused with
 * an argument error.  dx: (lead + n * h * row_pixels) * c elements of dtype, all written.  dbias, partial: as
 * mia_pool_bn_relu_bwd_apply_ex. */
int mia_pool_bn_relu_bwd_apply_rows(const void* gm, int32_t gm_dtype, const uint8_t* argmax, const void* x,
                                    int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                    const float* gamma, const float* mean, const float* invstd, const float* dgamma,
                                    const float* dbeta, void* dx, int32_t lead, int32_t row_pixels, void* zero_pixel,
                                    int32_t zc, float* dbias, void* partial, mia_stream_t stream);

/* mia_bn_relu_bwd_apply through a row map: the P pixels are rows of w (P % w == 0).  A map other than the dense one
 * needs P < 2^31.  dx: (lead + P / w * row_pixels) * C elements of dtype, all written; it must not be dact then.
 * dbias, partial: as mia_bn_relu_bwd_apply. */
int mia_bn_relu_bwd_apply_rows(const void* dact, const void* x, void* dx, int32_t dtype, int64_t P, int32_t C,
                               int32_t w, int32_t lead, int32_t row_pixels, void* zero_pixel, int32_t zc,
                               const float* gamma, const float* scale, const float* shift, const float* mean,
                               const float* invstd, const float* dgamma, const float* dbeta, float* dbias,
                               void* partial, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_ROWMAP_H */
