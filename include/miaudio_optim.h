/*
 * miaudio_optim.h — the fused optimizer family beside mia_clip_adam / mia_gemm_adam (part of libmiaudio.so):
 * gradient clipping + torch.optim.SGD (momentum, dampening, Nesterov, L2 decay) and + torch.optim.AdamW
 * (decoupled decay), each as a table-driven multi-tensor step and as the epilogue of the deferred weight-gradient
 * GEMM.  Replaces Lightning's gradient_clip_val + the optimizer the reference instantiates from
 * cfg.optimizer (src/training/engine.py:299-310) when that is not Adam at its defaults.
 *
 * Conventions as in miaudio.h: extern "C", stream-ordered, the caller owns all memory, 0 on success and a
 * negative code on error (mia_last_error_string() explains).
 *
 * Tables, norm pass and workspace are mia_clip_adam's: device arrays f32* params[n], grads[n], bf16* shadow[n]
 * (the table or any entry may be NULL), int64 sizes[n]; optional pre_sq / pre_n (precomputed partial sums of
 * squares, doubles, read instead of the gradient); a NULL grads[i] marks a deferred weight gradient -- counted in
 * the norm through pre_sq[i] only and not updated here (its update is mia_gemm_sgd / mia_gemm_adamw).
 * sqnorm_ws holds mia_adam_workspace_bytes(n) bytes; the clip coefficient (f32) is left at byte
 * mia_adam_coef_offset(n) of it, where the GEMM forms read it.  max_numel sizes the update grid (NULL-gradient
 * tensors excluded), max_norm_numel the norm grid (pre_sq tensors excluded).  clip <= 0 disables clipping;
 * total_norm_out (f32[1], may be NULL) receives the global norm.
 */
#ifndef MIAUDIO_OPTIM_H
#define MIAUDIO_OPTIM_H
#include "miaudio.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Clip + torch's single-tensor SGD, per element (c = the clip coefficient):
 *   g = fma(wd, p, g * c)
 *   momentum != 0:  buf = first_use ? g : fma(momentum, buf, (1 - dampening) * g)
 *                   g   = nesterov ? fma(momentum, buf, g) : buf
 *   p = fma(-lr, g, p)
 * momentum_buf: table of f32* [n], required when momentum != 0 and not read when momentum == 0 (pass NULL: the
 * step then moves 12 B per parameter instead of 20).  first_use: device int32[n] or NULL; a non-zero entry means
 * the tensor's buffer has never been written and is initialised to g (torch creates it at the parameter's first
 * gradient, which may be later than step 1); NULL means no tensor is at first use.  Every element of p (and of
 * buf, and of a non-NULL shadow: bf16(p)) of every tensor with a gradient is rewritten; nothing else is. */
int mia_clip_sgd(void* const* params, void* const* grads, void* const* momentum_buf, void* const* shadow_bf16,
                 const int64_t* sizes, int32_t ntensors, int64_t max_numel, int64_t max_norm_numel, float lr,
                 float momentum, float dampening, float weight_decay, int32_t nesterov, float clip,
                 float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq, const int64_t* pre_n,
                 const int32_t* first_use, mia_stream_t stream);

/* Clip + torch's single-tensor AdamW (Adam with decoupled_weight_decay=True): mia_clip_adam with
 *   p *= (float)(1 - lr * wd)   first, and no L2 term in g = g * c;
 * bias corrections, per-tensor `steps` and every argument as mia_clip_adam. */
int mia_clip_adamw(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                   void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                   int64_t max_norm_numel, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int32_t step, float clip, float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq,
                   const int64_t* pre_n, const int32_t* steps, mia_stream_t stream);

/* The mia_gemm_adam form for these two updates: the product dW = A . B^T (M x N, bf16 RC operands, M and N
 * multiples of 128, K a multiple of 64) is never stored; the epilogue applies the update above -- the same
 * arithmetic bit for bit, c read from `coef` on the device -- to rows [0, M) x columns [0, N) of param (and
 * momentum_buf / exp_avg / exp_avg_sq, and the optional bf16 shadow), row stride ld >= N elements, ld % 4 == 0,
 * f32 rows 16-B aligned, the shadow 8-B aligned.  mia_gemm_sgd: momentum_buf is NULL exactly when momentum == 0;
 * first_use != 0 initialises the buffer.  mia_gemm_adamw: lr_over_bc1 = lr / (1 - beta1^step) and
 * bc2_sqrt = sqrt(1 - beta2^step) as mia_clip_adamw forms them. */
int mia_gemm_sgd(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K, float* param,
                 float* momentum_buf, void* shadow_bf16, int64_t ld, const float* coef, float lr, float momentum,
                 float dampening, float weight_decay, int32_t nesterov, int32_t first_use, mia_stream_t stream);
int mia_gemm_adamw(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K, float* param,
                   float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t ld, const float* coef,
                   float lr_over_bc1, float bc2_sqrt, float beta1, float beta2, float eps, float lr,
                   float weight_decay, mia_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MIAUDIO_OPTIM_H */
