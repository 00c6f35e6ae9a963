// Clip + update of the fused optimizers over a device table of tensors (mia_clip_adam of include/miaudio.h,
// mia_clip_sgd / mia_clip_adamw of include/miaudio_optim.h): one global-norm pass, then one once-through update
// pass -- the same walker for every optimizer, with its rule of optim_update.h.  The two stochastic-weight-averaging
// passes of include/miaudio_swa.h (mia_swa_update, mia_swa_transfer) are that walker with fewer streams.
#include <algorithm>

#include "optim_update.h"
#include "../../include/miaudio_optim.h"
#include "../../include/miaudio_swa.h"

namespace {

using namespace mopt;

constexpr int NT = 256;

// ------------------------------------------------------------------ pass 1: global norm, clip coefficient
constexpr int ADAM_PARTS = 1024;
constexpr int NF_NT = 1024;

// Squared L2 norm partials of every gradient tensor: 16-B loads (tensor storage is 16-B aligned
// torch allocations; a misaligned one takes the scalar path), f32 accumulation flushed to double.
// A tensor with precomputed partials (pre_sq[tsr], e.g. the sqsum slots of the GEMM epilogue that
// wrote it) is not re-read: its partials are summed instead, in the same fixed grid-stride order.
__global__ __launch_bounds__(NT) void sqnorm_kernel(void* const* __restrict__ grads, const int64_t* __restrict__ sizes,
                                                    const void* const* __restrict__ pre_sq,
                                                    const int64_t* __restrict__ pre_n, float* __restrict__ ws) {
  const int tsr = blockIdx.y;
  const float* g = reinterpret_cast<const float*>(grads[tsr]);
  const int64_t n = sizes[tsr];
  const int64_t tid = (int64_t)blockIdx.x * NT + threadIdx.x, nthr = (int64_t)gridDim.x * NT;
  const double* pre = pre_sq ? reinterpret_cast<const double*>(pre_sq[tsr]) : nullptr;
  double s = 0.0;
  float fs = 0.f;
  int cnt = 0;
  if (pre) {
    for (int64_t i = tid; i < pre_n[tsr]; i += nthr) s += pre[i];
  } else if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const int64_t n4 = n >> 2;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = tid; i < n4; i += nthr) {
      const float4 v = g4[i];
      fs = fmaf(v.x, v.x, fs); fs = fmaf(v.y, v.y, fs); fs = fmaf(v.z, v.z, fs); fs = fmaf(v.w, v.w, fs);
      if (++cnt == 64) { s += fs; fs = 0.f; cnt = 0; }
    }
    for (int64_t i = (n4 << 2) + tid; i < n; i += nthr) fs = fmaf(g[i], g[i], fs);
  } else {
    for (int64_t i = tid; i < n; i += nthr) {
      fs = fmaf(g[i], g[i], fs);
      if (++cnt == 256) { s += fs; fs = 0.f; cnt = 0; }
    }
  }
  s += fs;
  s = wave_sum_d(s);
  __shared__ double red[4];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0)
    reinterpret_cast<double*>(ws)[(int64_t)tsr * ADAM_PARTS + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// ws layout (doubles): [ntensors][ADAM_PARTS] partials, then [0] = coef (float in double slot)
__global__ __launch_bounds__(NF_NT) void norm_final_kernel(double* ws, int ntensors, int nparts, float clip,
                                                           float* total_out, float* coef_out) {
  double s = 0.0;
  const int total = ntensors * nparts;
  for (int i = threadIdx.x; i < total; i += NF_NT) {  // fixed order: deterministic
    const int tsr = i / nparts, p = i % nparts;
    s += ws[(int64_t)tsr * ADAM_PARTS + p];
  }
  s = wave_sum_d(s);
  __shared__ double red[NF_NT / 64];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int w = 0; w < NF_NT / 64; ++w) acc += red[w];
    const double tot = sqrt(acc);
    const float totalf = (float)tot;
    float coef = 1.f;
    if (clip > 0.f) {
      coef = clip / (totalf + 1e-6f);
      if (coef > 1.f) coef = 1.f;
    }
    if (total_out) total_out[0] = totalf;
    coef_out[0] = coef;
  }
}

// Pass 1 of every clip + update entry point: the global gradient norm into total_norm_out and the clip coefficient
// into the workspace, at *coef
int clip_norm_pass(void* const* grads, const int64_t* sizes, int ntensors, int64_t max_norm_numel, float clip,
                   float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq, const int64_t* pre_n,
                   hipStream_t s, float** coef) {
  double* ws = reinterpret_cast<double*>(sqnorm_ws);
  *coef = reinterpret_cast<float*>(ws + (int64_t)ntensors * ADAM_PARTS);
  const int parts = (int)std::min<int64_t>(ADAM_PARTS, std::max<int64_t>(1, cdiv(max_norm_numel, 256 * 256)));
  sqnorm_kernel<<<dim3(parts, ntensors), NT, 0, s>>>(grads, sizes, pre_sq, pre_n, reinterpret_cast<float*>(ws));
  MIA_LAUNCH_CHECK("sqnorm");
  norm_final_kernel<<<1, NF_NT, 0, s>>>(ws, ntensors, parts, clip, total_norm_out, *coef);
  MIA_LAUNCH_CHECK("norm_final");
  return 0;
}

// ------------------------------------------------------------------ pass 2: the update
// One tensor's update pass: p, the gradient and NS state tensors (s0, s1) walked once, the bf16 operand copy sw
// (or null) rewritten beside p.  upd(p, g, a, b) returns the new p and updates the state values in place.
// 16-B aligned tensors: four float4 groups per iteration, every load issued before any use (one HBM round trip
// per 4 groups); every byte is touched once, so loads and stores are non-temporal (no L2/MALL allocation for a
// 10 GB once-through stream).  The n % 4 tail, and a tensor with any misaligned pointer (a view at an odd offset),
// go element by element.
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

// The tables of a launch (one tensor per blockIdx.y): state0 is the momentum buffer or exp_avg, state1 exp_avg_sq
struct Tables {
  void* const* __restrict__ params;
  void* const* __restrict__ grads;
  void* const* __restrict__ state0;
  void* const* __restrict__ state1;
  void* const* __restrict__ shadow;  // bf16 operand copies of the parameters: the table or any entry may be null
  const int64_t* __restrict__ sizes;
  const float* __restrict__ coef;    // the clip coefficient pass 1 left
};

// This block's tensor through stream_update<NS>; a tensor with no gradient has a deferred weight gradient, whose
// update runs in its GEMM (mia_gemm_adam / mia_gemm_sgd / mia_gemm_adamw)
template <int NS, class R>
__device__ __forceinline__ void update_tensor(const Tables& t, const R& r, bool first) {
  const int tsr = blockIdx.y;
  if (!t.grads[tsr]) return;
  const float coef = t.coef[0];
  stream_update<NS>(reinterpret_cast<float*>(t.params[tsr]), reinterpret_cast<const float*>(t.grads[tsr]),
                    NS > 0 ? reinterpret_cast<float*>(t.state0[tsr]) : nullptr,
                    NS > 1 ? reinterpret_cast<float*>(t.state1[tsr]) : nullptr,
                    t.shadow ? reinterpret_cast<bf16*>(t.shadow[tsr]) : nullptr, t.sizes[tsr],
                    [&](float pv, float gv, float& a, float& b) { return apply<NS>(r, coef, first, pv, gv, a, b); });
}

template <bool MOM>
__global__ __launch_bounds__(NT) void sgd_kernel(Tables t, SgdRule r, const int32_t* __restrict__ first_use) {
  update_tensor<MOM ? 1 : 0>(t, r, MOM && first_use && first_use[blockIdx.y] != 0);
}

// steps: per-tensor step counts or null (a parameter that missed gradients keeps its own count, as torch's Adam)
__global__ __launch_bounds__(NT) void adam_kernel(Tables t, AdamRule r, const int32_t* __restrict__ steps, float lr) {
  if (steps) set_step(r, lr, steps[blockIdx.y]);
  update_tensor<2>(t, r, false);
}

__global__ __launch_bounds__(NT) void adamw_kernel(Tables t, AdamWRule r, const int32_t* __restrict__ steps, float lr) {
  if (steps) set_step(r, lr, steps[blockIdx.y]);
  update_tensor<2>(t, r, false);
}

// What the three entry points share: the checks on the tables, pass 1, and the tables and grid of pass 2
// (max_numel / (256 * 32) blocks per tensor, at most 8192)
int clip_pass(const char* who, void* const* params, void* const* grads, void* const* state0, void* const* state1,
              void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
              int64_t max_norm_numel, float clip, float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq,
              const int64_t* pre_n, hipStream_t s, Tables* t, dim3* grid) {
  MIA_CHECK_ARG(params && grads && sizes && sqnorm_ws, "%s: null table", who);
  MIA_CHECK_ARG(ntensors > 0 && ntensors < 65536, "%s: ntensors", who);
  MIA_CHECK_ARG(!pre_sq || pre_n, "%s: pre_sq needs pre_n", who);
  float* coef = nullptr;
  if (int rc = clip_norm_pass(grads, sizes, ntensors, max_norm_numel, clip, total_norm_out, sqnorm_ws, pre_sq, pre_n,
                              s, &coef))
    return rc;
  *t = Tables{params, grads, state0, state1, shadow_bf16, sizes, coef};
  *grid = dim3((unsigned)std::min<int64_t>(8192, std::max<int64_t>(1, cdiv(max_numel, 256 * 32))), ntensors);
  return 0;
}

// mia_clip_adam and mia_clip_adamw: `last` is the rule's last member (the L2 coefficient / the decay factor)
template <class R>
int clip_adam_family(const char* who, void (*kernel)(Tables, R, const int32_t*, float), void* const* params,
                     void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, void* const* shadow_bf16,
                     const int64_t* sizes, int32_t ntensors, int64_t max_numel, int64_t max_norm_numel, float lr,
                     float beta1, float beta2, float eps, float last, int32_t step, float clip,
                     float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq, const int64_t* pre_n,
                     const int32_t* steps, mia_stream_t stream) {
  MIA_CHECK_ARG(exp_avg && exp_avg_sq && step >= 1, "%s: null moment table, or step < 1", who);
  hipStream_t s = as_stream(stream);
  Tables t;
  dim3 grid;
  if (int rc = clip_pass(who, params, grads, exp_avg, exp_avg_sq, shadow_bf16, sizes, ntensors, max_numel,
                         max_norm_numel, clip, total_norm_out, sqnorm_ws, pre_sq, pre_n, s, &t, &grid))
    return rc;
  R r{0.f, 0.f, beta1, beta2, eps, last};
  set_step(r, lr, step);
  kernel<<<grid, NT, 0, s>>>(t, r, steps, lr);
  MIA_LAUNCH_CHECK(who);
  return 0;
}

// ------------------------------------------------------------------ stochastic weight averaging
// avg + (p - avg) / d: one subtract, one correctly rounded divide, one add -- the rounding intrinsics keep the
// three apart (nothing to contract, no reciprocal), so the vector loops and the scalar tail give the same bits
__device__ __forceinline__ float swa_rule(float a, float p, float d) {
  return __fadd_rn(a, __fdiv_rn(__fsub_rn(p, a), d));
}

// avg is the walker's written tensor, the parameter its read-only one; FIRST (n_averaged == 0) copies, and the
// unused loads of avg fall away (8 B per parameter instead of 12)
template <bool FIRST>
__global__ __launch_bounds__(NT) void swa_update_kernel(void* const* __restrict__ avg,
                                                        void* const* __restrict__ params,
                                                        const int64_t* __restrict__ sizes, float d) {
  const int tsr = blockIdx.y;
  stream_update<0>(reinterpret_cast<float*>(avg[tsr]), reinterpret_cast<const float*>(params[tsr]), nullptr, nullptr,
                   nullptr, sizes[tsr],
                   [&](float av, float pv, float&, float&) { return FIRST ? pv : swa_rule(av, pv, d); });
}

// p = avg (the old p is never loaded), the bf16 operand copy rewritten beside it as in the optimizers' pass
__global__ __launch_bounds__(NT) void swa_transfer_kernel(void* const* __restrict__ params,
                                                          void* const* __restrict__ avg,
                                                          void* const* __restrict__ shadow,
                                                          const int64_t* __restrict__ sizes) {
  const int tsr = blockIdx.y;
  stream_update<0>(reinterpret_cast<float*>(params[tsr]), reinterpret_cast<const float*>(avg[tsr]), nullptr, nullptr,
                   shadow ? reinterpret_cast<bf16*>(shadow[tsr]) : nullptr, sizes[tsr],
                   [](float, float av, float&, float&) { return av; });
}

dim3 swa_grid(int64_t max_numel, int32_t ntensors) {  // the update pass's grid (clip_pass)
  return dim3((unsigned)std::min<int64_t>(8192, std::max<int64_t>(1, cdiv(max_numel, 256 * 32))), ntensors);
}

}  // namespace

extern "C" int mia_swa_update(void* const* avg, void* const* params, const int64_t* sizes, int32_t ntensors,
                              int64_t max_numel, int64_t n_averaged, mia_stream_t stream) {
  MIA_CHECK_ARG(avg && params && sizes, "swa_update: null table");
  MIA_CHECK_ARG(ntensors > 0 && ntensors < 65536, "swa_update: ntensors");
  MIA_CHECK_ARG(n_averaged >= 0 && max_numel >= 0, "swa_update: n_averaged or max_numel < 0");
  hipStream_t s = as_stream(stream);
  const dim3 grid = swa_grid(max_numel, ntensors);
  if (n_averaged == 0)
    swa_update_kernel<true><<<grid, NT, 0, s>>>(avg, params, sizes, 1.f);
  else
    swa_update_kernel<false><<<grid, NT, 0, s>>>(avg, params, sizes, (float)(n_averaged + 1));
  MIA_LAUNCH_CHECK("swa_update");
  return 0;
}

extern "C" int mia_swa_transfer(void* const* params, void* const* avg, void* const* shadow_bf16, const int64_t* sizes,
                                int32_t ntensors, int64_t max_numel, mia_stream_t stream) {
  MIA_CHECK_ARG(params && avg && sizes, "swa_transfer: null table");
  MIA_CHECK_ARG(ntensors > 0 && ntensors < 65536, "swa_transfer: ntensors");
  MIA_CHECK_ARG(max_numel >= 0, "swa_transfer: max_numel < 0");
  swa_transfer_kernel<<<swa_grid(max_numel, ntensors), NT, 0, as_stream(stream)>>>(params, avg, shadow_bf16, sizes);
  MIA_LAUNCH_CHECK("swa_transfer");
  return 0;
}

extern "C" int64_t mia_adam_workspace_bytes(int32_t ntensors) {
  return ((int64_t)ntensors * ADAM_PARTS + 2) * 8;
}

// byte offset of the clip coefficient (f32) inside mia_clip_adam's workspace
extern "C" int64_t mia_adam_coef_offset(int32_t ntensors) { return (int64_t)ntensors * ADAM_PARTS * 8; }

extern "C" int mia_clip_adam(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                             void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                             int64_t max_norm_numel, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int32_t step, float clip,
                             float* total_norm_out, void* sqnorm_ws, const void* const* pre_sq,
                             const int64_t* pre_n, const int32_t* steps, mia_stream_t stream) {
  return clip_adam_family<AdamRule>("clip_adam", adam_kernel, params, grads, exp_avg, exp_avg_sq, shadow_bf16, sizes,
                                    ntensors, max_numel, max_norm_numel, lr, beta1, beta2, eps, weight_decay, step,
                                    clip, total_norm_out, sqnorm_ws, pre_sq, pre_n, steps, stream);
}

extern "C" int mia_clip_adamw(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq,
                              void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                              int64_t max_norm_numel, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int32_t step, float clip, float* total_norm_out, void* sqnorm_ws,
                              const void* const* pre_sq, const int64_t* pre_n, const int32_t* steps,
                              mia_stream_t stream) {
  return clip_adam_family<AdamWRule>("clip_adamw", adamw_kernel, params, grads, exp_avg, exp_avg_sq, shadow_bf16,
                                     sizes, ntensors, max_numel, max_norm_numel, lr, beta1, beta2, eps,
                                     adamw_decay(lr, weight_decay), step, clip, total_norm_out, sqnorm_ws, pre_sq,
                                     pre_n, steps, stream);
}

extern "C" int mia_clip_sgd(void* const* params, void* const* grads, void* const* momentum_buf,
                            void* const* shadow_bf16, const int64_t* sizes, int32_t ntensors, int64_t max_numel,
                            int64_t max_norm_numel, float lr, float momentum, float dampening, float weight_decay,
                            int32_t nesterov, float clip, float* total_norm_out, void* sqnorm_ws,
                            const void* const* pre_sq, const int64_t* pre_n, const int32_t* first_use,
                            mia_stream_t stream) {
  MIA_CHECK_ARG((momentum != 0.f) == (momentum_buf != nullptr), "clip_sgd: momentum_buf goes with momentum != 0");
  MIA_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f),
                "clip_sgd: nesterov needs a momentum and zero dampening");
  hipStream_t s = as_stream(stream);
  Tables t;
  dim3 grid;
  if (int rc = clip_pass("clip_sgd", params, grads, momentum_buf, nullptr, shadow_bf16, sizes, ntensors, max_numel,
                         max_norm_numel, clip, total_norm_out, sqnorm_ws, pre_sq, pre_n, s, &t, &grid))
    return rc;
  const SgdRule r = sgd_rule(lr, momentum, dampening, weight_decay, nesterov);
  if (momentum_buf)
    sgd_kernel<true><<<grid, NT, 0, s>>>(t, r, first_use);
  else
    sgd_kernel<false><<<grid, NT, 0, s>>>(t, r, nullptr);
  MIA_LAUNCH_CHECK("sgd");
  return 0;
}
