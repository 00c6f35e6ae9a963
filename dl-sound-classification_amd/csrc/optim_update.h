// Per-element update rules of the fused optimizer family (include/miaudio_optim.h), shared by the streaming
// kernels (optim.hip) and the GEMM epilogues that apply them to a deferred weight gradient (dgemm.hip).  Every
// multiply-add is an explicit fmaf and nothing else can be contracted, so the two forms give the same bits
// whatever each file's compile flags do.
#pragma once
#include "common.h"

namespace mopt {

// torch's single-tensor SGD (torch/optim/sgd.py _single_tensor_sgd), the clip coefficient applied to the raw
// gradient first
struct SgdRule {
  float lr, momentum, omd, wd;  // omd = 1 - dampening
  int nesterov;
};
template <bool MOM>
__device__ __forceinline__ float sgd_update(const SgdRule& r, float coef, bool first, float p, float g, float& buf) {
  g = fmaf(r.wd, p, g * coef);
  if constexpr (MOM) {
    buf = first ? g : fmaf(r.momentum, buf, r.omd * g);  // first use of the buffer: torch clones the gradient
    g = r.nesterov ? fmaf(r.momentum, buf, g) : buf;
  }
  return fmaf(-r.lr, g, p);
}

// torch's single-tensor AdamW (Adam with decoupled_weight_decay): p *= 1 - lr * wd, then Adam with no L2 term
struct AdamWRule {
  float lr_over_bc1, bc2_sqrt, beta1, beta2, eps, decay;  // decay = adamw_decay(lr, wd)
};
static inline float adamw_decay(float lr, float wd) { return (float)(1.0 - (double)lr * (double)wd); }
__device__ __forceinline__ float adamw_update(const AdamWRule& r, float coef, float p, float g, float& m, float& v) {
  g *= coef;
  p *= r.decay;
  m = fmaf(1.f - r.beta1, g - m, m);           // exp_avg.lerp_(grad, 1 - beta1)
  v = fmaf((1.f - r.beta2) * g, g, v * r.beta2);  // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1 - beta2)
  const float denom = sqrtf(v) / r.bc2_sqrt + r.eps;
  return fmaf(-r.lr_over_bc1, m / denom, p);
}

}  // namespace mopt
