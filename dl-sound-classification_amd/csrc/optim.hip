// Clip + SGD and clip + AdamW over a device table of tensors (include/miaudio_optim.h): the norm pass of
// mia_clip_adam (misc.hip), then one once-through update pass built like adam_kernel.
#include <algorithm>

#include "optim_update.h"
#include "../../include/miaudio_optim.h"

namespace {

using namespace mopt;

constexpr int NT = 256;

// One tensor's update pass: p, the gradient and NS state tensors (s0, s1) walked once, the bf16 operand copy sw
// (or null) rewritten beside p.  upd(p, g, a, b) returns the new p and updates the state values in place.
// 16-B aligned tensors: four float4 groups per iteration, every load issued before any use (one HBM round trip
// per 4 groups); every byte is touched once, so loads and stores are non-temporal.  The n % 4 tail, and a tensor
// with any misaligned pointer (a view at an odd offset), go element by element.
template <int NS, class F>
__device__ __forceinline__ void stream_update(float* p, const float* g, float* s0, float* s1, bf16* sw, int64_t n,
                                              F upd) {
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
  if constexpr (NS > 0) bits |= reinterpret_cast<uintptr_t>(s0);
  if constexpr (NS > 1) bits |= reinterpret_cast<uintptr_t>(s1);
  const bool al = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(sw) & 7) == 0;
  int64_t done = 0;
  if (al) {
    const int64_t n4 = n >> 2;
    constexpr int U = 4;
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* a4 = reinterpret_cast<f32x4*>(s0);
    f32x4* b4 = reinterpret_cast<f32x4*>(s1);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto step4 = [&](int64_t i, f32x4 pv, f32x4 gv, f32x4 av, f32x4 bv) __attribute__((always_inline)) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float a = av[e], b = bv[e];
        pv[e] = upd(pv[e], gv[e], a, b);
        av[e] = a;
        bv[e] = b;
      }
      __builtin_nontemporal_store(pv, p4 + i);
      if constexpr (NS > 0) __builtin_nontemporal_store(av, a4 + i);
      if constexpr (NS > 1) __builtin_nontemporal_store(bv, b4 + i);
      if (sw) {
        const bf16x4 h4 = {(bf16)pv[0], (bf16)pv[1], (bf16)pv[2], (bf16)pv[3]};
        __builtin_nontemporal_store(h4, reinterpret_cast<bf16x4*>(sw) + i);
      }
    };
    int64_t i = tid;
    for (; i + (U - 1) * nthr < n4; i += U * nthr) {
      f32x4 pv[U], gv[U], av[U], bv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t j = i + u * nthr;
        pv[u] = __builtin_nontemporal_load(p4 + j);
        gv[u] = __builtin_nontemporal_load(g4 + j);
        av[u] = zero;
        bv[u] = zero;
        if constexpr (NS > 0) av[u] = __builtin_nontemporal_load(a4 + j);
        if constexpr (NS > 1) bv[u] = __builtin_nontemporal_load(b4 + j);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) step4(i + u * nthr, pv[u], gv[u], av[u], bv[u]);
    }
    for (; i < n4; i += nthr) {
      f32x4 av = zero, bv = zero;
      if constexpr (NS > 0) av = a4[i];
      if constexpr (NS > 1) bv = b4[i];
      step4(i, p4[i], g4[i], av, bv);
    }
    done = n4 << 2;
  }
  for (int64_t i = done + tid; i < n; i += nthr) {
    float a = 0.f, b = 0.f;
    if constexpr (NS > 0) a = s0[i];
    if constexpr (NS > 1) b = s1[i];
    const float pn = upd(p[i], g[i], a, b);
    p[i] = pn;
    if constexpr (NS > 0) s0[i] = a;
    if constexpr (NS > 1) s1[i] = b;
    if (sw) sw[i] = (bf16)pn;
  }
}

template <bool MOM>
__global__ __launch_bounds__(NT) void sgd_kernel(void* const* __restrict__ params, void* const* __restrict__ grads,
                                                 void* const* __restrict__ bufs, void* const* __restrict__ shadow,
                                                 const int64_t* __restrict__ sizes, const float* __restrict__ coef_p,
                                                 SgdRule r, const int32_t* __restrict__ first_use) {
  const int tsr = blockIdx.y;
  if (!grads[tsr]) return;  // a deferred weight gradient: its update runs in its GEMM (mia_gemm_sgd)
  float* buf = nullptr;
  if constexpr (MOM) buf = reinterpret_cast<float*>(bufs[tsr]);
  bf16* sw = shadow ? reinterpret_cast<bf16*>(shadow[tsr]) : nullptr;
  const bool first = MOM && first_use && first_use[tsr] != 0;
  const float coef = coef_p[0];
  stream_update<MOM ? 1 : 0>(reinterpret_cast<float*>(params[tsr]), reinterpret_cast<const float*>(grads[tsr]), buf,
                             nullptr, sw, sizes[tsr], [&](float pv, float gv, float& bv, float&) {
                               return sgd_update<MOM>(r, coef, first, pv, gv, bv);
                             });
}

__global__ __launch_bounds__(NT) void adamw_kernel(void* const* __restrict__ params, void* const* __restrict__ grads,
                                                   void* const* __restrict__ m1, void* const* __restrict__ m2,
                                                   void* const* __restrict__ shadow,
                                                   const int64_t* __restrict__ sizes, const float* __restrict__ coef_p,
                                                   AdamWRule r, const int32_t* __restrict__ steps, float lr) {
  const int tsr = blockIdx.y;
  if (!grads[tsr]) return;  // a deferred weight gradient: its update runs in its GEMM (mia_gemm_adamw)
  if (steps) {  // per-tensor step counts, as adam_kernel
    const double st = (double)steps[tsr];
    r.lr_over_bc1 = (float)(lr / (1.0 - pow((double)r.beta1, st)));
    r.bc2_sqrt = (float)sqrt(1.0 - pow((double)r.beta2, st));
  }
  bf16* sw = shadow ? reinterpret_cast<bf16*>(shadow[tsr]) : nullptr;
  const float coef = coef_p[0];
  stream_update<2>(reinterpret_cast<float*>(params[tsr]), reinterpret_cast<const float*>(grads[tsr]),
                   reinterpret_cast<float*>(m1[tsr]), reinterpret_cast<float*>(m2[tsr]), sw, sizes[tsr],
                   [&](float pv, float gv, float& mv, float& vv) { return adamw_update(r, coef, pv, gv, mv, vv); });
}

// blocks per tensor of the update pass (adam_kernel's grid)
int update_blocks(int64_t max_numel) {
  return (int)std::min<int64_t>(8192, std::max<int64_t>(1, cdiv(max_numel, 256 * 32)));
}

}  // namespace

extern "C" int mia_clip_sgd(void* const* params, void* const* grads, void* const* momentum_buf,
                            void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                            int64_t max_norm_numel, float lr, float momentum, float dampening, float weight_decay,
                            int32_t nesterov, float clip, float* total_norm_out, void* sqnorm_ws,
                            const void* const* pre_sq, const int64_t* pre_n, const int32_t* first_use,
                            mia_stream_t stream) {
  MIA_CHECK_ARG(params && grads && sizes && sqnorm_ws, "clip_sgd: null table");
  MIA_CHECK_ARG(ntensors > 0 && ntensors < 65536, "clip_sgd: ntensors");
  MIA_CHECK_ARG(!pre_sq || pre_n, "clip_sgd: pre_sq needs pre_n");
  MIA_CHECK_ARG((momentum != 0.f) == (momentum_buf != nullptr), "clip_sgd: momentum_buf goes with momentum != 0");
  MIA_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f),
                "clip_sgd: nesterov needs a momentum and zero dampening");
  hipStream_t s = as_stream(stream);
  float* coef = nullptr;
  if (int rc = mia::clip_norm_pass(grads, sizes, ntensors, max_norm_numel, clip, total_norm_out, sqnorm_ws, pre_sq,
                                   pre_n, s, &coef))
    return rc;
  const SgdRule r{lr, momentum, 1.f - dampening, weight_decay, nesterov ? 1 : 0};
  const dim3 grid(update_blocks(max_numel), ntensors);
  if (momentum_buf)
    sgd_kernel<true><<<grid, NT, 0, s>>>(params, grads, momentum_buf, shadow_bf16, sizes, coef, r, first_use);
  else
    sgd_kernel<false><<<grid, NT, 0, s>>>(params, grads, nullptr, shadow_bf16, sizes, coef, r, nullptr);
  MIA_LAUNCH_CHECK("sgd");
  return 0;
}

extern "C" int mia_clip_adamw(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                              void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                              int64_t max_norm_numel, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int32_t step, float clip, float* total_norm_out, void* sqnorm_ws,
                              const void* const* pre_sq, const int64_t* pre_n, const int32_t* steps,
                              mia_stream_t stream) {
  MIA_CHECK_ARG(params && grads && exp_avg && exp_avg_sq && sizes && sqnorm_ws, "clip_adamw: null table");
  MIA_CHECK_ARG(ntensors > 0 && ntensors < 65536 && step >= 1, "clip_adamw: ntensors/step");
  MIA_CHECK_ARG(!pre_sq || pre_n, "clip_adamw: pre_sq needs pre_n");
  hipStream_t s = as_stream(stream);
  float* coef = nullptr;
  if (int rc = mia::clip_norm_pass(grads, sizes, ntensors, max_norm_numel, clip, total_norm_out, sqnorm_ws, pre_sq,
                                   pre_n, s, &coef))
    return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const AdamWRule r{(float)(lr / bc1), (float)sqrt(bc2), beta1, beta2, eps, adamw_decay(lr, weight_decay)};
  adamw_kernel<<<dim3(update_blocks(max_numel), ntensors), NT, 0, s>>>(params, grads, exp_avg, exp_avg_sq, shadow_bf16,
                                                                      sizes, coef, r, steps, lr);
  MIA_LAUNCH_CHECK("adamw");
  return 0;
}
