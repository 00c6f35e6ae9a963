// LEAF trunk glue (gfx950): the memory-bound passes around the mia_gemm convolutions of LeafModel's conv_block
// (reference src/models/leaf.py:60-77 Conv1d -> BatchNorm1d -> ReLU -> MaxPool1d x3 -> AdaptiveAvgPool1d(1)).
// Maps are channels-last (n, t, c), bf16 or f32, c % 8 == 0 in [8, 1024]; c / 8 need not divide the block:
// a block runs rslots = 256 / (c / 8) row slots of c / 8 threads (240 of its 256 threads at c = 384), so a
// thread keeps one 8-channel group for the whole kernel and per-channel sums live in registers.
//   pcen_cl_fwd / bwd : PCEN (leaf.hip) reading / writing P [B][F][Tp] but with y / gy channels-last
//                       (B, Tp, Fp) through LDS tiles -- the CONV operand layout of conv1.
//   pool_stats        : one read of z -> raw window winners + u8 argmax + BN shifted partial sums of EVERY frame.
//   pool_apply        : relu(scale * win + shift) -> pooled map, or its mean over time (n, c).
//   pool_bwd_gather   : pooled-size ReLU mask + dgamma / dbeta.
//   pool_bwd_apply    : one read of z, one write of dz (BN backward), optional dbias.
// Every reduction runs in a fixed order (no atomics): results are bit-identical run to run.
#include <algorithm>

#include "bn_math.h"
#include "channel_partials.h"
#include "pcen_math.h"

namespace {

constexpr int NT = CP_NT;

struct Slots {
  int G, rslots;
};
inline Slots slots_for(int c) { return Slots{c / 8, NT / (c / 8)}; }

inline int lt_blocks(int64_t units, int rslots, int per) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(units, (int64_t)rslots * per), CP_MAXBLK));
}

// ------------------------------------------------------------------------------------------- b. winners + statistics
// unit = (clip b, window w < ceil(t / k)): frames w k .. min(w k + k, t) - 1.  A unit with w < t / k is a pooled cell
// (winner + argmax written); the last, short unit of a clip (t % k frames) feeds the statistics only.
__global__ __launch_bounds__(NT) void lt_pool_stats_kernel(const void* __restrict__ z, int dtype, int n, int T, int C,
                                                           int k, const float* __restrict__ gamma,
                                                           const float* __restrict__ kshift, void* __restrict__ win,
                                                           uint8_t* __restrict__ argmax, float* __restrict__ partial) {
  const int G = C / 8, rslots = NT / G;
  const int cg = threadIdx.x % G, rs = threadIdx.x / G;
  const int OT = T / k, NW = (T + k - 1) / k;
  float dir[8], ks[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { dir[i] = 0.f; ks[i] = 0.f; s1[i] = 0.f; s2[i] = 0.f; }
  if (rs < rslots) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float gv = gamma[cg * 8 + i];
      dir[i] = gv > 0.f ? 1.f : (gv < 0.f ? -1.f : 0.f);
      ks[i] = kshift ? kshift[cg * 8 + i] : 0.f;
    }
    const int units = n * NW;  // < 2^31 (checked by the launcher)
    for (int u = blockIdx.x * rslots + rs; u < units; u += gridDim.x * rslots) {
      const int b = u / NW, w = u - b * NW;
      const int f0 = w * k, nf = min(k, T - f0);
      float best[8], bestraw[8];
      int arg[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bestraw[i] = 0.f; arg[i] = 0; }
      const int64_t base = ((int64_t)b * T + f0) * C + cg * 8;
      for (int j = 0; j < nf; ++j) {
        float f[8];
        load8(z, dtype, base + (int64_t)j * C, f);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = f[i] - ks[i];
          s1[i] += d;
          s2[i] = fmaf(d, d, s2[i]);
          const float key = dir[i] * f[i];  // gamma == 0: key 0 everywhere -> the first position wins
          // (a window whose keys are all NaN or all -inf never passes the strict >, and writes winner 0 at
          // position 0: a non-finite z is not propagated into the pooled map, but it does reach s1 / s2 and
          // with them the statistics, scale and shift of the whole channel, so the step still shows it)
          if (key > best[i]) { best[i] = key; bestraw[i] = f[i]; arg[i] = j; }
        }
      }
      if (w < OT) {
        const int64_t aoff = ((int64_t)b * OT + w) * C + cg * 8;
        *reinterpret_cast<uint2*>(argmax + aoff) = argmax_pack(arg);
        store8(win, dtype, aoff, bestraw);  // exact: z's own dtype
      }
    }
  }
  if (partial) cp_fold<2>(s1, s2, C, G, rslots, blockIdx.x, partial);
}

// ------------------------------------------------------------------------------------------- c. apply
__global__ __launch_bounds__(NT) void lt_pool_apply_kernel(const void* __restrict__ win, int dtype, int64_t groups,
                                                           int G, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, void* __restrict__ out,
                                                           int odt) {
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < groups; e += (int64_t)gridDim.x * NT) {
    const int cg = (int)(e % G);
    float f[8], v[8];
    load8(win, dtype, e * 8, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bn_relu(f[i], scale[cg * 8 + i], shift[cg * 8 + i]);
    store8(out, odt, e * 8, v);
  }
}

// time mean of relu(scale * win + shift) over the OT pooled frames of each clip (AdaptiveAvgPool1d(1)): one thread
// per (clip, 8-channel group), frames added in order
__global__ __launch_bounds__(NT) void lt_pool_apply_mean_kernel(const void* __restrict__ win, int dtype, int n, int OT,
                                                                int C, const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                void* __restrict__ out, int odt) {
  const int G = C / 8;
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= n * G) return;
  const int b = e / G, cg = e - b * G;
  BnFwd8 bn;
  bn.load(cg, scale, shift);
  float acc[8] = {0};
  for (int j = 0; j < OT; ++j) {
    float f[8];
    load8(win, dtype, ((int64_t)b * OT + j) * C + cg * 8, f);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] += bn_relu(f[i], bn.sc[i], bn.sh[i]);
  }
  const float inv = 1.f / (float)OT;
#pragma unroll
  for (int i = 0; i < 8; ++i) acc[i] *= inv;
  store8(out, odt, (int64_t)e * 8, acc);
}

// ------------------------------------------------------------------------------------------- d. backward
// pooled size: gm = dout * (scale * win + shift > 0); partial sums of gm (-> dbeta) and gm * xhat (-> dgamma).
// mean != 0: dout is dh (n, c) of the time-mean variant, dout[cell] = dh[b] / OT.
__global__ __launch_bounds__(NT) void lt_pool_bwd_gather_kernel(const void* __restrict__ dout, int ddt, int mean_mode,
                                                                const void* __restrict__ win, int dtype, int n, int OT,
                                                                int C, const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                float* __restrict__ gm, float* __restrict__ partial) {
  const int G = C / 8, rslots = NT / G;
  const int cg = threadIdx.x % G, rs = threadIdx.x / G;
  float s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  if (rs < rslots) {
    BnRed8 bn;
    bn.load(cg, scale, shift, mean, invstd);
    const float inv = 1.f / (float)OT;
    const int cells = n * OT;  // < 2^31 (checked by the launcher)
    for (int u = blockIdx.x * rslots + rs; u < cells; u += gridDim.x * rslots) {
      const int64_t off = (int64_t)u * C + cg * 8;
      float f[8], d[8], g[8];
      load8(win, dtype, off, f);
      if (mean_mode) {
        load8(dout, ddt, (int64_t)(u / OT) * C + cg * 8, d);
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] *= inv;
      } else {
        load8(dout, ddt, off, d);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) g[i] = bn.step(i, d[i], f[i], s1[i], s2[i]);
      store8(gm, MIA_F32, off, g);
    }
  }
  cp_fold<2>(s1, s2, C, G, rslots, blockIdx.x, partial);
}

// dense: dz = gamma invstd (g - dbeta / P - xhat dgamma / P), g = gm[cell] at the argmax frame, else 0; unit as in
// lt_pool_stats_kernel (the t % k frames past the last window have g = 0)
__global__ __launch_bounds__(NT) void lt_pool_bwd_apply_kernel(const float* __restrict__ gm,
                                                               const uint8_t* __restrict__ argmax,
                                                               const void* __restrict__ z, int dtype, int n, int T,
                                                               int C, int k, const float* __restrict__ gamma,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, void* __restrict__ dz,
                                                               float* __restrict__ partial) {
  const int G = C / 8, rslots = NT / G;
  const int cg = threadIdx.x % G, rs = threadIdx.x / G;
  const int OT = T / k, NW = (T + k - 1) / k;
  float s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  if (rs < rslots) {
    BnApply8 bn;
    bn.load(cg, gamma, mean, invstd, dgamma, dbeta, 1.f / (float)((int64_t)n * T));
    const int units = n * NW;
    for (int u = blockIdx.x * rslots + rs; u < units; u += gridDim.x * rslots) {
      const int b = u / NW, w = u - b * NW;
      const int f0 = w * k, nf = min(k, T - f0);
      float gv[8];
      uint2 am = make_uint2(0xffffffffu, 0xffffffffu);  // 255: no frame of a short tail unit matches
#pragma unroll
      for (int i = 0; i < 8; ++i) gv[i] = 0.f;
      if (w < OT) {
        const int64_t coff = ((int64_t)b * OT + w) * C + cg * 8;
        am = *reinterpret_cast<const uint2*>(argmax + coff);
        load8(gm, MIA_F32, coff, gv);
      }
      const int64_t base = ((int64_t)b * T + f0) * C + cg * 8;
      for (int j = 0; j < nf; ++j) {
        float x[8], g[8];
        load8(z, dtype, base + (int64_t)j * C, x);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float gi = (argmax_byte(am, i) == j && w < OT) ? gv[i] : 0.f;
          g[i] = bn.dx(i, gi, x[i]);
          s1[i] += g[i];
        }
        store8(dz, dtype, base + (int64_t)j * C, g);
      }
    }
  }
  if (partial) cp_fold<2>(s1, s2, C, G, rslots, blockIdx.x, partial);  // slot 1: zeros
}

// ------------------------------------------------------------------------------------------- a. channels-last PCEN
// The arithmetic is pcen_math.h's, shared with leaf.hip's pcen_fwd_kernel / pcen_bwd_kernel (same expressions, same
// frame -> thread map, same reduction tree), so the f32 results carry the same bits; only the side of the transpose
// differs.

constexpr int PF_TF = 32, PF_TT = 64;  // forward tile: 32 filters x 64 frames

// grid (ceil(Tp / 64), ceil(Fp / 32), B).  P rows are read along t (coalesced 4-B lanes), y rows are written as
// 8-channel runs (16 B bf16 / 32 B f32); channels F .. Fp - 1 and the halo rows are zero.
__global__ __launch_bounds__(NT) void lt_pcen_fwd_kernel(const float* __restrict__ P, const float* __restrict__ r,
                                                         const float* __restrict__ delta, float eps,
                                                         void* __restrict__ y, int odt, int F, int Fp, int Tp,
                                                         int halo) {
  __shared__ float pin[PF_TF][PF_TT + 4 + 1];
  __shared__ float yo[PF_TT][PF_TF + 1];
  const int t0 = blockIdx.x * PF_TT, f0 = blockIdx.y * PF_TF, b = blockIdx.z;
  const int tid = threadIdx.x;
  for (int e = tid; e < PF_TF * (PF_TT + 4); e += NT) {
    const int fl = e / (PF_TT + 4), tl = e - fl * (PF_TT + 4);
    const int f = f0 + fl, t = t0 - 2 + tl;
    pin[fl][tl] = (f < F && t >= 0 && t < Tp) ? P[((int64_t)b * F + f) * Tp + t] : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < PF_TF * PF_TT; e += NT) {
    const int fl = e / PF_TT, tl = e - fl * PF_TT;
    const int f = f0 + fl, j = t0 + tl;
    float v = 0.f;
    if (f < F && j < Tp) {
      const float* pr = &pin[fl][2 - t0];  // pr[j] = P[b][f][j] for j in [t0 - 2, t0 + 66)
      v = pcen_fwd_value(pr, Tp, j, eps, r[f], delta[f]);
    }
    yo[tl][fl] = v;
  }
  __syncthreads();
  const int rows = Tp + 2 * halo;
  {
    const int tl = tid >> 2, g = tid & 3;  // 64 rows x 4 channel groups
    const int j = t0 + tl, f = f0 + g * 8;
    if (j < Tp && f < Fp) {
      float v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = yo[tl][g * 8 + i];
      store8(y, odt, ((int64_t)b * rows + halo + j) * Fp + f, v);
    }
  }
  if (blockIdx.x == 0 && halo > 0) {  // the clip's leading and trailing zero rows, this block's channel groups
    const float zero[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int e = tid; e < 2 * halo * 4; e += NT) {
      const int hr = e >> 2, g = e & 3, f = f0 + g * 8;
      const int row = hr < halo ? hr : Tp + hr;  // hr in [halo, 2 halo) -> rows halo + Tp ..
      if (f < Fp) store8(y, odt, ((int64_t)b * rows + row) * Fp + f, zero);
    }
  }
}

constexpr int PB_TF = 8, PB_TT = 256, PB_RQ = 4;  // backward: 8 filters (one channel run) per block, chunks of 256 frames

// grid (ceil(F / 8), B).  Thread tid owns frames i = tid, tid + 256, .. of each of the block's 8 filter rows (the
// frame assignment of pcen_bwd_kernel), so the per-row double sums and their tree are the same; gy (channels-last)
// is staged through LDS in 16-B / 32-B channel runs, P and gP move along t.  (16 filters per block measured
// 0.47 ms at B = 64, F = 128, Tp = 1378: too few blocks and a long serial chain of powf / logf per thread.)
__global__ __launch_bounds__(NT) void lt_pcen_bwd_kernel(const float* __restrict__ P, const float* __restrict__ r,
                                                         const float* __restrict__ delta, float eps,
                                                         const void* __restrict__ gy, int gdt, float* __restrict__ gP,
                                                         double* __restrict__ part, int F, int Fp, int Tp, int halo) {
  __shared__ float pt[PB_TF][PB_TT + 8 + 1];
  __shared__ float gt[PB_TT + 4][PB_TF + 1];
  __shared__ double red[PB_RQ][2][NT];
  const int f0 = blockIdx.x * PB_TF, b = blockIdx.y;
  const int tid = threadIdx.x;
  const int rows = Tp + 2 * halo;
  double sr[PB_TF], sd[PB_TF];
#pragma unroll
  for (int q = 0; q < PB_TF; ++q) { sr[q] = 0.0; sd[q] = 0.0; }
  for (int c0 = 0; c0 < Tp; c0 += PB_TT) {
    __syncthreads();
    for (int e = tid; e < PB_TF * (PB_TT + 8); e += NT) {
      const int fl = e / (PB_TT + 8), tl = e - fl * (PB_TT + 8);
      const int f = f0 + fl, t = c0 - 4 + tl;
      pt[fl][tl] = (f < F && t >= 0 && t < Tp) ? P[((int64_t)b * F + f) * Tp + t] : 0.f;
    }
    constexpr int PB_G = PB_TF / 8;  // channel runs per frame
    for (int e = tid; e < (PB_TT + 4) * PB_G; e += NT) {
      const int tl = e / PB_G, g = e - tl * PB_G;
      const int t = c0 - 2 + tl, f = f0 + g * 8;
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (t >= 0 && t < Tp && f < Fp) load8(gy, gdt, ((int64_t)b * rows + halo + t) * Fp + f, v);
#pragma unroll
      for (int i = 0; i < 8; ++i) gt[tl][g * 8 + i] = v[i];
    }
    __syncthreads();
    const int i = c0 + tid;
    if (i < Tp) {
#pragma unroll
      for (int q = 0; q < PB_TF; ++q) {
        if (f0 + q >= F) break;
        const float* pr = &pt[q][4 - c0];  // pr[j] = P[b][f][j] for j in [c0 - 4, c0 + 260)
        const float rf = r[f0 + q], df = delta[f0 + q];
        float g = 0.f;
#pragma unroll
        for (int d = -2; d <= 2; ++d) {
          const int j = i + d;
          if (j < 0 || j >= Tp) continue;
          const PcenTap tp = pcen_bwd_tap(pr, Tp, j, eps, gt[j - c0 + 2][q], rf, df);
          g += tp.via_m;
          if (d == 0) {
            g += tp.direct;
            sr[q] += (double)tp.dr;
            sd[q] += (double)tp.ddelta;
          }
        }
        gP[((int64_t)b * F + f0 + q) * Tp + i] = g;
      }
    }
  }
  // per-row tree over the 256 threads, four rows at a time
#pragma unroll
  for (int q0 = 0; q0 < PB_TF; q0 += PB_RQ) {
    __syncthreads();
    pcen_row_tree<PB_RQ>(red, sr + q0, sd + q0);
    if (tid < PB_RQ && f0 + q0 + tid < F) {
      const int64_t row = (int64_t)b * F + f0 + q0 + tid;
      part[row * 2] = red[tid][0][0];
      part[row * 2 + 1] = red[tid][1][0];
    }
  }
}

int lt_check_map(const char* what, int32_t dtype, int32_t n, int32_t t, int32_t c, int32_t k) {
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "%s: dtype %d", what, dtype);
  MIA_CHECK_ARG(c % 8 == 0 && c >= 8 && c <= 1024, "%s: c = %d must be a multiple of 8 in [8, 1024]", what, c);
  MIA_CHECK_ARG(n >= 1 && k >= 1 && k <= 255 && t >= k, "%s: bad geometry n=%d t=%d k=%d", what, n, t, k);
  MIA_CHECK_ARG((int64_t)n * t * (c / 8) < (1ll << 31), "%s: too many elements for 32-bit indexing", what);
  return 0;
}

int lt_pcen_check(const char* what, int32_t dtype, int32_t B, int32_t F, int32_t Tp, int32_t halo) {
  MIA_CHECK_ARG(dtype == MIA_F32 || dtype == MIA_BF16, "%s: dtype %d", what, dtype);
  MIA_CHECK_ARG(B >= 1 && B <= 65535 && F >= 1 && F <= 1024 && Tp >= 1 && halo >= 0 && halo <= 8,
                "%s: bad shape B=%d F=%d Tp=%d halo=%d", what, B, F, Tp, halo);
  MIA_CHECK_ARG((int64_t)B * (Tp + 2 * halo) * ((F + 7) / 8) < (1ll << 31) && cdiv(Tp, PF_TT) <= 65535,
                "%s: too many elements", what);
  return 0;
}

}  // namespace

extern "C" int32_t mia_lt_stats_blocks(int32_t n, int32_t t, int32_t c, int32_t k) {
  if (c < 8 || c > 1024 || c % 8 || n < 1 || k < 1 || t < k) return 0;
  return lt_blocks((int64_t)n * cdiv(t, k), slots_for(c).rslots, 4);
}

extern "C" int64_t mia_lt_workspace_bytes(int32_t c) {
  if (c < 8 || c > 1024 || c % 8) return 0;
  return (int64_t)CP_MAXBLK * c * 2 * 4;
}

extern "C" int mia_lt_pool_stats(const void* z, int32_t dtype, int32_t n, int32_t t, int32_t c, int32_t k,
                                 const float* gamma, const float* kshift, void* win, uint8_t* argmax, float* partial,
                                 int32_t nblocks, mia_stream_t stream) {
  if (int rc = lt_check_map("lt_pool_stats", dtype, n, t, c, k)) return rc;
  MIA_CHECK_ARG(z && gamma && win && argmax, "lt_pool_stats: null pointer");
  MIA_CHECK_ARG(aligned16(z) && aligned16(win) && (reinterpret_cast<uintptr_t>(argmax) & 7) == 0,
                "lt_pool_stats: alignment");
  MIA_CHECK_ARG(nblocks >= 1 && nblocks <= CP_MAXBLK, "lt_pool_stats: nblocks %d out of [1, %d]", nblocks, CP_MAXBLK);
  lt_pool_stats_kernel<<<nblocks, NT, 0, as_stream(stream)>>>(z, dtype, n, t, c, k, gamma, kshift, win, argmax, partial);
  MIA_LAUNCH_CHECK("lt_pool_stats");
  return 0;
}

extern "C" int mia_lt_pool_apply(const void* win, int32_t dtype, int32_t n, int32_t ot, int32_t c, const float* scale,
                                 const float* shift, void* out, int32_t out_dtype, int32_t mean, mia_stream_t stream) {
  if (int rc = lt_check_map("lt_pool_apply", dtype, n, ot, c, 1)) return rc;
  MIA_CHECK_ARG(out_dtype == MIA_F32 || out_dtype == MIA_BF16, "lt_pool_apply: out dtype %d", out_dtype);
  MIA_CHECK_ARG(win && scale && shift && out && aligned16(win) && aligned16(out), "lt_pool_apply: null / unaligned pointer");
  hipStream_t s = as_stream(stream);
  if (mean) {
    lt_pool_apply_mean_kernel<<<(unsigned)cdiv((int64_t)n * (c / 8), NT), NT, 0, s>>>(win, dtype, n, ot, c, scale, shift,
                                                                                      out, out_dtype);
    MIA_LAUNCH_CHECK("lt_pool_apply_mean");
    return 0;
  }
  const int64_t groups = (int64_t)n * ot * (c / 8);
  const int nb = (int)std::min<int64_t>(cdiv(groups, NT), 16384);
  lt_pool_apply_kernel<<<nb, NT, 0, s>>>(win, dtype, groups, c / 8, scale, shift, out, out_dtype);
  MIA_LAUNCH_CHECK("lt_pool_apply");
  return 0;
}

extern "C" int mia_lt_pool_bwd_gather(const void* dout, int32_t dout_dtype, int32_t mean_mode, const void* win,
                                      int32_t dtype, int32_t n, int32_t ot, int32_t c, const float* scale,
                                      const float* shift, const float* mean, const float* invstd, float* gm,
                                      float* dgamma, float* dbeta, void* workspace, mia_stream_t stream) {
  if (int rc = lt_check_map("lt_pool_bwd_gather", dtype, n, ot, c, 1)) return rc;
  MIA_CHECK_ARG(dout_dtype == MIA_F32 || dout_dtype == MIA_BF16, "lt_pool_bwd_gather: dout dtype %d", dout_dtype);
  MIA_CHECK_ARG(dout && win && scale && shift && mean && invstd && gm && dgamma && dbeta && workspace,
                "lt_pool_bwd_gather: null pointer");
  MIA_CHECK_ARG(aligned16(dout) && aligned16(win) && aligned16(gm), "lt_pool_bwd_gather: alignment");
  hipStream_t s = as_stream(stream);
  const int nb = lt_blocks((int64_t)n * ot, slots_for(c).rslots, 2);
  lt_pool_bwd_gather_kernel<<<nb, NT, 0, s>>>(dout, dout_dtype, mean_mode, win, dtype, n, ot, c, scale, shift, mean,
                                              invstd, gm, (float*)workspace);
  MIA_LAUNCH_CHECK("lt_pool_bwd_gather");
  cp_final2_kernel<<<(unsigned)c, 256, 0, s>>>((const float*)workspace, nb, c, /*q0 = sum gm*/ dbeta,
                                               /*q1 = sum gm xhat*/ dgamma);
  MIA_LAUNCH_CHECK("lt_pool_bwd_gather_final");
  return 0;
}

extern "C" int mia_lt_pool_bwd_apply(const float* gm, const uint8_t* argmax, const void* z, int32_t dtype, int32_t n,
                                     int32_t t, int32_t c, int32_t k, const float* gamma, const float* mean,
                                     const float* invstd, const float* dgamma, const float* dbeta, void* dz,
                                     float* dbias, void* workspace, mia_stream_t stream) {
  if (int rc = lt_check_map("lt_pool_bwd_apply", dtype, n, t, c, k)) return rc;
  MIA_CHECK_ARG(gm && argmax && z && mean && invstd && dgamma && dbeta && dz, "lt_pool_bwd_apply: null pointer");
  MIA_CHECK_ARG(!dbias || workspace, "lt_pool_bwd_apply: dbias needs the workspace");
  MIA_CHECK_ARG(aligned16(gm) && aligned16(z) && aligned16(dz) && (reinterpret_cast<uintptr_t>(argmax) & 7) == 0,
                "lt_pool_bwd_apply: alignment");
  hipStream_t s = as_stream(stream);
  const int nb = lt_blocks((int64_t)n * cdiv(t, k), slots_for(c).rslots, 4);
  lt_pool_bwd_apply_kernel<<<nb, NT, 0, s>>>(gm, argmax, z, dtype, n, t, c, k, gamma, mean, invstd, dgamma, dbeta, dz,
                                             dbias ? (float*)workspace : nullptr);
  MIA_LAUNCH_CHECK("lt_pool_bwd_apply");
  if (dbias) {
    cp_final2_kernel<<<(unsigned)c, 256, 0, s>>>((const float*)workspace, nb, c, /*q0 = sum dz*/ dbias, nullptr);
    MIA_LAUNCH_CHECK("lt_pool_bwd_apply_final");
  }
  return 0;
}

extern "C" int mia_lt_pcen_fwd(const float* P, const float* r, const float* delta, float eps, void* y, int32_t dtype,
                               int32_t B, int32_t F, int32_t Tp, int32_t halo, mia_stream_t stream) {
  if (int rc = lt_pcen_check("lt_pcen_fwd", dtype, B, F, Tp, halo)) return rc;
  MIA_CHECK_ARG(P && r && delta && y && aligned16(y), "lt_pcen_fwd: null / unaligned pointer");
  const int Fp = (F + 7) / 8 * 8;
  dim3 grid((unsigned)cdiv(Tp, PF_TT), (unsigned)cdiv(Fp, PF_TF), (unsigned)B);
  lt_pcen_fwd_kernel<<<grid, NT, 0, as_stream(stream)>>>(P, r, delta, eps, y, dtype, F, Fp, Tp, halo);
  MIA_LAUNCH_CHECK("lt_pcen_fwd");
  return 0;
}

extern "C" int mia_lt_pcen_bwd(const float* P, const float* r, const float* delta, float eps, const void* gy,
                               int32_t dtype, float* gP, float* dr, float* ddelta, void* workspace, int32_t B,
                               int32_t F, int32_t Tp, int32_t halo, mia_stream_t stream) {
  if (int rc = lt_pcen_check("lt_pcen_bwd", dtype, B, F, Tp, halo)) return rc;
  MIA_CHECK_ARG(P && r && delta && gy && gP && dr && ddelta && workspace && aligned16(gy),
                "lt_pcen_bwd: null / unaligned pointer");
  const int Fp = (F + 7) / 8 * 8;
  hipStream_t s = as_stream(stream);
  double* part = reinterpret_cast<double*>(workspace);
  lt_pcen_bwd_kernel<<<dim3((unsigned)cdiv(F, PB_TF), (unsigned)B), NT, 0, s>>>(P, r, delta, eps, gy, dtype, gP, part, F,
                                                                               Fp, Tp, halo);
  MIA_LAUNCH_CHECK("lt_pcen_bwd");
  pcen_param_reduce_kernel<<<(unsigned)cdiv(F, 256), 256, 0, s>>>(part, dr, ddelta, B, F);
  MIA_LAUNCH_CHECK("lt_pcen_bwd (reduce)");
  return 0;
}
