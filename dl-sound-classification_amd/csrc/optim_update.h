// Per-element update rules of the fused optimizers (include/miaudio.h, include/miaudio_optim.h), shared by the
// streaming kernels (optim.hip) and the GEMM epilogue that applies them to a deferred weight gradient (dgemm.hip).
// Every multiply-add of every rule is an explicit fmaf and nothing else can be contracted, so an element's update
// is the same bits in every loop of either form, whatever each file's compile flags do.
#pragma once
#include "common.h"

namespace mopt {

// torch's single-tensor SGD (torch/optim/sgd.py _single_tensor_sgd), the clip coefficient applied to the raw
// gradient first
struct SgdRule {
  float lr, momentum, omd, wd;  // omd = 1 - dampening
  int nesterov;
};
static inline SgdRule sgd_rule(float lr, float momentum, float dampening, float wd, int nesterov) {
  return SgdRule{lr, momentum, 1.f - dampening, wd, nesterov ? 1 : 0};
}
template <bool MOM>
__device__ __forceinline__ float sgd_update(const SgdRule& r, float coef, bool first, float p, float g, float& buf) {
  g = fmaf(r.wd, p, g * coef);
  if constexpr (MOM) {
    buf = first ? g : fmaf(r.momentum, buf, r.omd * g);  // first use of the buffer: torch clones the gradient
    g = r.nesterov ? fmaf(r.momentum, buf, g) : buf;
  }
  return fmaf(-r.lr, g, p);
}

// torch's single-tensor Adam (L2 decay added to the gradient) and AdamW (Adam with decoupled_weight_decay:
// p *= 1 - lr * wd, then Adam with no L2 term).  The rules differ in their last member only.
struct AdamRule {
  float lr_over_bc1, bc2_sqrt, beta1, beta2, eps, wd;
};
struct AdamWRule {
  float lr_over_bc1, bc2_sqrt, beta1, beta2, eps, decay;  // decay = adamw_decay(lr, wd)
};
static inline float adamw_decay(float lr, float wd) { return (float)(1.0 - (double)lr * (double)wd); }

// The bias corrections of step `step`, from f32 lr / betas and a double pow: on the host for the whole table, in
// the kernel for a tensor with a step count of its own (a parameter that missed gradients, as torch's Adam)
template <class R>
__host__ __device__ inline void set_step(R& r, float lr, int step) {
  r.lr_over_bc1 = (float)(lr / (1.0 - pow((double)r.beta1, (double)step)));
  r.bc2_sqrt = (float)sqrt(1.0 - pow((double)r.beta2, (double)step));
}

// the moment updates and the step both rules end in; g is the clipped (and, for Adam, decayed) gradient
template <class R>
__device__ __forceinline__ float adam_moments_step(const R& r, float p, float g, float& m, float& v) {
  m = fmaf(1.f - r.beta1, g - m, m);              // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf((1.f - r.beta2) * g, g, v * r.beta2);  // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / r.bc2_sqrt + r.eps;
  return fmaf(-r.lr_over_bc1, m / denom, p);
}
__device__ __forceinline__ float adam_update(const AdamRule& r, float coef, float p, float g, float& m, float& v) {
  return adam_moments_step(r, p, fmaf(r.wd, p, g * coef), m, v);
}
__device__ __forceinline__ float adamw_update(const AdamWRule& r, float coef, float p, float g, float& m, float& v) {
  return adam_moments_step(r, p * r.decay, g * coef, m, v);
}

// The rules under one signature, for the callers that are generic in the rule: NS is the number of state tensors
// beside p (0 SGD without momentum, 1 SGD with a momentum buffer a, 2 the moments a and b); `first` is SGD's
template <int NS>
__device__ __forceinline__ float apply(const SgdRule& r, float coef, bool first, float p, float g, float& a, float&) {
  return sgd_update<NS == 1>(r, coef, first, p, g, a);
}
template <int NS>
__device__ __forceinline__ float apply(const AdamRule& r, float coef, bool, float p, float g, float& a, float& b) {
  return adam_update(r, coef, p, g, a, b);
}
template <int NS>
__device__ __forceinline__ float apply(const AdamWRule& r, float coef, bool, float p, float g, float& a, float& b) {
  return adamw_update(r, coef, p, g, a, b);
}

}  // namespace mopt
