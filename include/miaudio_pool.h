/*
 * miaudio_pool.h — the pooled backward of miaudio.h (mia_pool_bwd_gather, mia_pool_bn_relu_bwd_apply) with the
 * masked pooled gradient gm in a dtype the caller chooses (part of libmiaudio.so).
 *
 * gm[cell][c] is the pooled gradient dout[cell][c] where relu(bn(x)) let it through, else 0.  On the bf16 path every
 * entry is therefore a bf16 value, and a bf16 gm converts back to exactly the float an f32 gm holds: dx, dgamma,
 * dbeta and dbias are the same bits either way, and gm costs half the bytes to write and to read back.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).  The entry points of miaudio.h are these with
 * gm_dtype = MIA_F32.
 */
#ifndef MIAUDIO_POOL_H
#define MIAUDIO_POOL_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mia_pool_bwd_gather with gm (n, h/kh, w/kw, c) of gm_dtype: MIA_F32, or MIA_BF16 when dtype is MIA_BF16 (an f32
 * gradient would be rounded, so that pair is refused).  gm: cells * c elements of gm_dtype, 16-byte aligned (a
 * cell's eight channels go out as one 16-B store of bf16 or two of f32); every element is written.  dgamma,
 * dbeta: c floats each, written.  partial: mia_bn_partial_bytes(n * h * w, c) bytes of workspace. */
int mia_pool_bwd_gather_ex(const void* dout, int32_t out_layout, const uint8_t* argmax, const void* x,
                           const void* win /* optional raw winners (n, h/kh, w/kw, c), x's dtype, or NULL */,
                           int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                           const float* scale, const float* shift, const float* mean, const float* invstd,
                           void* gm, int32_t gm_dtype, float* dgamma, float* dbeta, void* partial,
                           mia_stream_t stream);

/* mia_pool_bn_relu_bwd_apply reading gm of gm_dtype (MIA_F32 or MIA_BF16; 16-byte aligned, read only).  dx:
 * (n, h, w, c) of dtype, every element written; optional dbias: c floats, written, and then partial:
 * mia_bn_partial_bytes(n * h * w, c) bytes of workspace. */
int mia_pool_bn_relu_bwd_apply_ex(const void* gm, int32_t gm_dtype, const uint8_t* argmax, const void* x,
                                  int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                  const float* gamma, const float* mean, const float* invstd, const float* dgamma,
                                  const float* dbeta, void* dx, float* dbias, void* partial, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_POOL_H */
