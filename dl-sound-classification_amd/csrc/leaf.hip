// LEAF frontend (include/miaudio.h "LEAF frontend"): Gabor energy + average pool, forward and filter-bank
// gradient, and PCEN forward / backward.
//
// Energy, BF16 compute (the hot path): a GEMM with the Toeplitz operand A[t][k] = x[t + k - h] on the row side
// and the packed bank B[k][2 x 32 filters] on the column side, v_mfma_f32_32x32x16_bf16.  A workgroup owns one
// clip, one block of 32 filters (64 bank rows: re, im) and a run of q pool frames; it stages
//   * the bank block as ready-made B fragments (one 16-B slot per lane and k-step), and
//   * the waveform segment as ENTRIES: entry o = the 8 bf16 samples x[s0 + o .. s0 + o + 7], 16 B each.  The A
//     fragment of lane (r, hh) for time tile tt and k-step kk is entry tt + r + 16 kk + 8 hh: every fragment is
//     ONE aligned ds_read_b128, the 32 lanes of a half read 32 consecutive slots (conflict-free), and the
//     sample-misalignment of the Toeplitz rows is paid once, at staging (8 x the segment's bytes in LDS).
// The fragment of (tile m, k-step kk) depends on 2 m + kk only, so a wave that walks 4 consecutive tiles keeps
// a sliding window of fragments and reads two new ones per two k-steps.  |.|^2 and the pool run on the
// accumulators: time is the accumulator's row index (registers + lane half), the filter its column (lane), so a
// tile's pool contribution is an in-lane sum and one lane exchange; tile sums meet in LDS and are added in a
// fixed order.  Nothing of size [B][F][T] exists.
//
// Backward, BF16 compute: v_mfma_f32_16x16x32_bf16, the tile recomputed, scaled and contracted inside one wave
// ("MFMA backward" below).
//
// F32 compute (forward and backward) and the BF16 backward of filters longer than 447 taps: plain FMA kernels,
// one wave per filter, register-blocked 4 samples (forward) / 4 taps (contraction) per lane with the segment and
// the filter in LDS.  In BF16 mode they round x, w and the scaled tile to bf16 and accumulate in f32, the
// arithmetic of the MFMA path.
// dw: every workgroup owns a fixed run of (clip, frame) pairs and a slab [2][F][Kt] of the workspace; the slabs
// are added in slab order by a second kernel (no atomics: bit-identical run to run).
#include "pcen_math.h"

namespace {

constexpr int LEAF_FG = 4;         // filters per workgroup of the FMA kernels (one per wave)
constexpr int LEAF_TW_MAX = 2560;  // samples per workgroup of the MFMA kernel
constexpr int LEAF_LDS_MAX = 150 * 1024;
constexpr int LEAF_NCT = 28;        // tap tiles of 16 the MFMA backward keeps in registers (Kt <= 447)
constexpr int LEAF_TWB_MAX = 1280;  // samples per unit of the MFMA backward

struct LeafPlan {
  int h, K4, nk, Kp, p, q, Tp, nfb, nfg, nsplit, per;
  int64_t frames, pack_bytes, slab_bytes;
  bool wlds;
  int lds_mfma, lds_fwd, lds_bwd;
  // MFMA backward (BF16 compute, Kp <= 16 * LEAF_NCT)
  bool mbwd;
  int nk32, qb, nchunkb, nfb64, nsplitb, perb, lds_mbwd;
  int64_t unitsb, pack16_bytes, slabb_bytes;
};

int pad256(int v) { return (v + 255) / 256 * 256; }

int leaf_plan(int32_t B, int64_t T, int32_t F, int32_t Kt, int32_t pool, LeafPlan& pl) {
  MIA_CHECK_ARG(B >= 1 && B <= 65535, "leaf: B = %d out of range [1, 65535]", B);
  MIA_CHECK_ARG(Kt >= 3 && Kt <= 1023 && (Kt & 1), "leaf: Kt = %d must be odd and in [3, 1023]", Kt);
  MIA_CHECK_ARG(F >= 1 && F <= 65535, "leaf: F = %d out of range [1, 65535]", F);
  MIA_CHECK_ARG(pool >= 32 && pool <= 1024 && pool % 32 == 0, "leaf: pool = %d must be a multiple of 32 in [32, 1024]",
                pool);
  MIA_CHECK_ARG(T >= pool && T / pool <= (int64_t)1 << 30, "leaf: T = %lld must be >= pool (and T / pool <= 2^30)",
                (long long)T);
  pl.h = Kt / 2;
  pl.K4 = (Kt + 3) / 4 * 4;
  pl.Kp = (Kt + 31) / 32 * 32;
  pl.nk = pl.Kp / 16;
  pl.p = pool / 32;
  pl.Tp = (int)(T / pool);
  pl.nfb = (F + 31) / 32;
  pl.nfg = (F + LEAF_FG - 1) / LEAF_FG;
  // frames per workgroup of the MFMA kernel: tiles (p * q) a multiple of 16 (4 waves x groups of 4 tiles) where
  // that fits LEAF_TW_MAX samples, else the largest power of two that fits
  int g = pl.p, a = 16;
  while (a) { int t = g % a; g = a; a = t; }  // gcd(p, 16)
  const int q0 = 16 / g;
  if (pool * q0 <= LEAF_TW_MAX) pl.q = q0 * (LEAF_TW_MAX / (pool * q0));
  else {
    pl.q = 1;
    while (pool * pl.q * 2 <= LEAF_TW_MAX) pl.q *= 2;
  }
  if (pl.q > pl.Tp) pl.q = pl.Tp;
  const int nent = pl.q * pool + pl.Kp + 96;
  const int tsum = pl.q * pl.p * 32 * 4;
  pl.lds_mfma = nent * 16 + tsum + 2 * pl.nk * 64 * 16;
  pl.wlds = pl.lds_mfma <= LEAF_LDS_MAX;
  if (!pl.wlds) pl.lds_mfma = nent * 16 + tsum;
  pl.pack_bytes = (int64_t)pl.nfb * 2 * pl.nk * 64 * 16;
  pl.lds_fwd = (LEAF_FG * 2 * pl.K4 + pad256(pool) + pl.K4 + 8) * 4;
  pl.lds_bwd = (LEAF_FG * 2 * pl.K4 + pad256(pool) + pad256(pl.K4) + 8 + LEAF_FG * 2 * pool) * 4;
  pl.frames = (int64_t)B * pl.Tp;
  int64_t ns = 4096 / pl.nfg;
  if (ns < 1) ns = 1;
  if (ns > 512) ns = 512;
  if (ns > pl.frames) ns = pl.frames;
  const int64_t per = (pl.frames + ns - 1) / ns;
  MIA_CHECK_ARG(per <= INT32_MAX, "leaf: too many frames");
  pl.per = (int)per;
  pl.nsplit = (int)((pl.frames + per - 1) / per);
  pl.slab_bytes = (int64_t)pl.nsplit * 2 * F * Kt * 4;
  pl.mbwd = pl.Kp <= 16 * LEAF_NCT;
  pl.nk32 = pl.Kp / 32;
  pl.qb = LEAF_TWB_MAX / pool > 1 ? LEAF_TWB_MAX / pool : 1;
  if (pl.qb > pl.Tp) pl.qb = pl.Tp;
  pl.nchunkb = (pl.Tp + pl.qb - 1) / pl.qb;
  pl.unitsb = (int64_t)B * pl.nchunkb;
  pl.nfb64 = (F + 63) / 64;
  int64_t nsb = 512 / pl.nfb64;
  if (nsb < 1) nsb = 1;
  if (nsb > pl.unitsb) nsb = pl.unitsb;
  const int64_t perb = (pl.unitsb + nsb - 1) / nsb;
  pl.perb = (int)perb;
  pl.nsplitb = (int)((pl.unitsb + perb - 1) / perb);
  pl.lds_mbwd = (pl.qb * pool + pl.Kp + 128) * 16 + 8 * pl.nk32 * 64 * 16 + pl.qb * 64 * 4;
  pl.pack16_bytes = (int64_t)pl.nfb64 * 8 * pl.nk32 * 64 * 16;
  pl.slabb_bytes = (int64_t)pl.nsplitb * 2 * F * Kt * 4;
  return 0;
}

__device__ __forceinline__ float rnd_bf16(float v) { return (float)(bf16)v; }

// ------------------------------------------------------------------------------------------- FMA kernels
// stage the 4 filters' taps (zero-padded to K4) and the frame's segment seg[i] = x[t0 - h + i] (zero outside
// the clip and beyond the last tap's reach)
template <bool BF>
__device__ __forceinline__ void fma_stage_w(float* wl, const float* __restrict__ w, int fg, int F, int Kt, int K4) {
  for (int i = threadIdx.x; i < LEAF_FG * 2 * K4; i += 256) {
    const int wv = i / (2 * K4), rem = i - wv * 2 * K4;
    const int c = rem / K4, k = rem - c * K4;
    const int f = fg * LEAF_FG + wv;
    float v = (f < F && k < Kt) ? w[((int64_t)c * F + f) * Kt + k] : 0.f;
    wl[i] = BF ? rnd_bf16(v) : v;
  }
}
template <bool BF>
__device__ __forceinline__ void fma_stage_seg(float* seg, int nseg, const float* __restrict__ xb, int64_t T, int64_t s0,
                                              int nvalid) {
  for (int i = threadIdx.x; i < nseg; i += 256) {
    const int64_t t = s0 + i;
    float v = (i < nvalid && t >= 0 && t < T) ? xb[t] : 0.f;
    seg[i] = BF ? rnd_bf16(v) : v;
  }
}
// ar[i] / ai[i] = sum_k w_re/im[k] * seg[tb + i + k], i < 4 (tb and the bases 16-B aligned)
__device__ __forceinline__ void fma_conv4(const float* seg, const float* wr, const float* wi, int K4, int tb,
                                          float (&ar)[4], float (&ai)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) ar[i] = ai[i] = 0.f;
  for (int k = 0; k < K4; k += 4) {
    const float4 s0 = *reinterpret_cast<const float4*>(seg + tb + k);
    const float4 s1 = *reinterpret_cast<const float4*>(seg + tb + k + 4);
    const float4 a = *reinterpret_cast<const float4*>(wr + k);
    const float4 c = *reinterpret_cast<const float4*>(wi + k);
    const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ar[i] = fmaf(av[kk], s[i + kk], ar[i]);
        ai[i] = fmaf(cv[kk], s[i + kk], ai[i]);
      }
  }
}

// grid (Tp, ceil(F / 4), B): one pool frame, four filters (one per wave)
template <bool BF>
__global__ __launch_bounds__(256) void leaf_fwd_fma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           float* __restrict__ P, int64_t T, int F, int Kt, int pool,
                                                           int Tp) {
  extern __shared__ __attribute__((aligned(16))) float leaf_smem[];
  const int K4 = (Kt + 3) / 4 * 4, h = Kt / 2;
  const int nseg = (pool + 255) / 256 * 256 + K4 + 8;
  float* wl = leaf_smem;
  float* seg = wl + LEAF_FG * 2 * K4;
  const int j = blockIdx.x, fg = blockIdx.y, b = blockIdx.z;
  fma_stage_w<BF>(wl, w, fg, F, Kt, K4);
  fma_stage_seg<BF>(seg, nseg, x + (int64_t)b * T, T, (int64_t)j * pool - h, pool + Kt - 1);
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = fg * LEAF_FG + wv;
  if (f >= F) return;
  const float* wr = wl + wv * 2 * K4;
  float e = 0.f;
  for (int ib = 0; ib * 256 < pool; ++ib) {
    const int tb = ib * 256 + 4 * lane;
    float ar[4], ai[4];
    fma_conv4(seg, wr, wr + K4, K4, tb, ar, ai);
    if (tb < pool) {
#pragma unroll
      for (int i = 0; i < 4; ++i) e += ar[i] * ar[i] + ai[i] * ai[i];
    }
  }
  e = wave_sum(e);
  if (lane == 0) P[((int64_t)b * F + f) * Tp + j] = e / (float)pool;
}

// grid (nsplit, ceil(F / 4)): frames [blockIdx.x * per, + per) of the B * Tp (clip, frame) pairs; the xr / xi
// of a frame recomputed as the forward does, scaled by (2 / pool) gP into LDS, contracted over the frame's
// samples against the same segment, 4 taps per lane; sums over the frames stay in registers
template <bool BF>
__global__ __launch_bounds__(256) void leaf_bwd_fma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ gP, float* __restrict__ slab,
                                                           int64_t T, int F, int Kt, int pool, int Tp, int64_t frames,
                                                           int per) {
  extern __shared__ __attribute__((aligned(16))) float leaf_smem[];
  const int K4 = (Kt + 3) / 4 * 4, h = Kt / 2;
  const int nseg = (pool + 255) / 256 * 256 + (K4 + 255) / 256 * 256 + 8;
  float* wl = leaf_smem;
  float* seg = wl + LEAF_FG * 2 * K4;
  float* sl = seg + nseg;
  const int fg = blockIdx.y;
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int f = fg * LEAF_FG + wv;
  const float* wr = wl + wv * 2 * K4;
  float* sre = sl + wv * 2 * pool;
  float* sim = sre + pool;
  fma_stage_w<BF>(wl, w, fg, F, Kt, K4);
  float dre[4][4], dim[4][4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int i = 0; i < 4; ++i) dre[kb][i] = dim[kb][i] = 0.f;
  const int64_t fr0 = (int64_t)blockIdx.x * per;
  const int64_t fr1 = fr0 + per < frames ? fr0 + per : frames;
  for (int64_t fr = fr0; fr < fr1; ++fr) {
    const int b = (int)(fr / Tp), j = (int)(fr - (int64_t)b * Tp);
    __syncthreads();  // the previous frame's segment is no longer read (and wl is staged)
    fma_stage_seg<BF>(seg, nseg, x + (int64_t)b * T, T, (int64_t)j * pool - h, pool + Kt - 1);
    __syncthreads();
    if (f < F) {
      const float g = gP[((int64_t)b * F + f) * Tp + j] * (2.f / (float)pool);
      for (int ib = 0; ib * 256 < pool; ++ib) {
        const int tb = ib * 256 + 4 * lane;
        float ar[4], ai[4];
        fma_conv4(seg, wr, wr + K4, K4, tb, ar, ai);
        if (tb < pool) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float vr = ar[i] * g, vi = ai[i] * g;
            sre[tb + i] = BF ? rnd_bf16(vr) : vr;
            sim[tb + i] = BF ? rnd_bf16(vi) : vi;
          }
        }
      }
      wave_sync();
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        if (kb * 256 < K4) {
          const int kbase = kb * 256 + 4 * lane;
          for (int t = 0; t < pool; t += 4) {
            const float4 s0 = *reinterpret_cast<const float4*>(seg + t + kbase);
            const float4 s1 = *reinterpret_cast<const float4*>(seg + t + kbase + 4);
            const float4 a = *reinterpret_cast<const float4*>(sre + t);
            const float4 c = *reinterpret_cast<const float4*>(sim + t);
            const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
            const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (int tt = 0; tt < 4; ++tt)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                dre[kb][i] = fmaf(av[tt], s[i + tt], dre[kb][i]);
                dim[kb][i] = fmaf(cv[tt], s[i + tt], dim[kb][i]);
              }
          }
        }
      }
      wave_sync();
    }
  }
  if (f >= F) return;
  float* o_re = slab + (((int64_t)blockIdx.x * 2 + 0) * F + f) * Kt;
  float* o_im = slab + (((int64_t)blockIdx.x * 2 + 1) * F + f) * Kt;
#pragma unroll
  for (int kb = 0; kb < 4; ++kb)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = kb * 256 + 4 * lane + i;
      if (k < Kt) {
        o_re[k] = dre[kb][i];
        o_im[k] = dim[kb][i];
      }
    }
}

// dw[i] = slab 0 + slab 1 + ... in slab order (double)
__global__ __launch_bounds__(256) void leaf_slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ dw,
                                                               int64_t n, int nsplit) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int k = 0; k < nsplit; ++k) s += (double)slab[(int64_t)k * n + i];
  dw[i] = (float)s;
}

// ------------------------------------------------------------------------------------------- MFMA forward
// bank -> B fragments: slot ((fb * 2 + c) * nk + kk) * 64 + lane = w[c][fb * 32 + (lane & 31)][16 kk + 8 (lane >> 5)
// + 0..7] as bf16 (zero for f >= F and the padded taps)
__global__ __launch_bounds__(256) void leaf_pack_kernel(const float* __restrict__ w, uint4* __restrict__ wpk, int F, int Kt,
                                                        int nk, int64_t nslot) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nslot) return;
  const int lane = (int)(i & 63);
  const int64_t r = i >> 6;
  const int kk = (int)(r % nk);
  const int64_t fc = r / nk;
  const int c = (int)(fc & 1);
  const int f = (int)(fc >> 1) * 32 + (lane & 31);
  const int k0 = 16 * kk + 8 * (lane >> 5);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (f < F && k0 + j < Kt) ? w[((int64_t)c * F + f) * Kt + k0 + j] : 0.f;
  wpk[i] = make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
}

__device__ __forceinline__ bf16x8 as_frag(uint4 u) { return __builtin_bit_cast(bf16x8, u); }

// grid (ceil(Tp / q), ceil(F / 32), B)
template <bool WLDS>
__global__ __launch_bounds__(256) void leaf_fwd_mfma_kernel(const float* __restrict__ x, const uint4* __restrict__ wpk,
                                                            float* __restrict__ P, int64_t T, int F, int h, int nk,
                                                            int pool, int Tp, int q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char leaf_smem_b[];
  const int p = pool / 32, Kp = nk * 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j0 = blockIdx.x * q, fb = blockIdx.y, b = blockIdx.z;
  const int nfr = q < Tp - j0 ? q : Tp - j0;
  const int ntile = nfr * p;
  uint4* ent = reinterpret_cast<uint4*>(leaf_smem_b);  // [q * pool + Kp + 96]: the last 96 feed discarded tiles only
  float* tsum = reinterpret_cast<float*>(ent + (q * pool + Kp + 96));  // [q * p][32]
  uint4* wl = reinterpret_cast<uint4*>(tsum + q * p * 32);             // [2][nk][64]
  const float* xb = x + (int64_t)b * T;
  const int64_t s0 = (int64_t)j0 * pool - h;
  const int nent = ntile * 32 + Kp;
  for (int o = tid; o < nent; o += 256) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t t = s0 + o + j;
      v[j] = (t >= 0 && t < T) ? xb[t] : 0.f;
    }
    ent[o] = make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
  }
  const uint4* wsrc = wpk + (int64_t)fb * 2 * nk * 64;
  if (WLDS) {
    for (int i = tid; i < 2 * nk * 64; i += 256) wl[i] = wsrc[i];
  }
  __syncthreads();
  const uint4* bre = (WLDS ? (const uint4*)wl : wsrc) + lane;
  const uint4* bim = bre + nk * 64;
  const int ngroup = (ntile + 3) / 4;
  for (int grp = wave; grp < ngroup; grp += 4) {
    f32x16 acc[4][2];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][c][i] = 0.f;
    // fragment g of this group = entry base + 16 g; tile m at k-step kk takes g = 2 m + kk
    const uint4* eb = ent + grp * 128 + (lane & 31) + 8 * (lane >> 5);
    uint4 ae[4], ao[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      ae[m] = eb[16 * (2 * m)];
      ao[m] = eb[16 * (2 * m + 1)];
    }
    uint4 b0r = bre[0], b0i = bim[0], b1r = bre[64], b1i = bim[64];
    for (int kk = 0; kk < nk; kk += 2) {
      // the next k-pair's fragments are requested ahead of this pair's MFMAs (one wave per SIMD: nothing else
      // hides the LDS latency); the last pass re-reads slot 0, in bounds and unused
      const bool more = kk + 2 < nk;
      const int kn = more ? kk + 2 : 0, gn = more ? 8 + kk : 0;
      const uint4 n0r = bre[kn * 64], n0i = bim[kn * 64], n1r = bre[(kn + 1) * 64], n1i = bim[(kn + 1) * 64];
      const uint4 na = eb[16 * gn], no = eb[16 * (gn + 1)];
      __builtin_amdgcn_sched_barrier(0);  // keep the requests above the MFMAs (the scheduler sinks them to their use)
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ae[m]), as_frag(b0r), acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ae[m]), as_frag(b0i), acc[m][1], 0, 0, 0);
      }
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ao[m]), as_frag(b1r), acc[m][0], 0, 0, 0);
        acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_frag(ao[m]), as_frag(b1i), acc[m][1], 0, 0, 0);
      }
      // slide: (m, kk + 2) is (m + 1, kk); the last tile takes fragments 8 + kk, 9 + kk
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        ae[m] = ae[m + 1];
        ao[m] = ao[m + 1];
      }
      ae[3] = na;
      ao[3] = no;
      b0r = n0r; b0i = n0i; b1r = n1r; b1i = n1i;
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      float e = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) e += acc[m][0][i] * acc[m][0][i] + acc[m][1][i] * acc[m][1][i];
      e += __shfl_xor(e, 32, 64);
      const int tile = grp * 4 + m;
      if (tile < ntile && lane < 32) tsum[tile * 32 + lane] = e;
    }
  }
  __syncthreads();
  for (int i = tid; i < nfr * 32; i += 256) {
    const int fl = i / nfr, fr = i - fl * nfr;
    const int f = fb * 32 + fl;
    float s = 0.f;
    for (int m = 0; m < p; ++m) s += tsum[(fr * p + m) * 32 + fl];
    if (f < F) P[((int64_t)b * F + f) * Tp + j0 + fr] = s / (float)pool;
  }
}

// ------------------------------------------------------------------------------------------- MFMA backward
// v_mfma_f32_16x16x32_bf16.  A workgroup owns 64 filters (wave = 16 filters: its re and im bank rows as B
// fragments in LDS) and a fixed run of (clip, chunk of qb frames) units; every wave walks ALL the time tiles of
// a unit for its own filters, so the scaled tile never leaves the wave:
//   1. forward, 8 time tiles of 16 samples: X[t][f] = sum_k A[t][k] w[f][k], A fragments = segment entries as in
//      the forward kernel, sliding by two fragments per k-step of 32;
//   2. S = X * (2 / pool) gP[frame of the tile][f] -> bf16.  The accumulator holds column f on lane & 15 and rows
//      t = 4 (lane >> 4) + reg: the lane's 4 + 4 values of two consecutive tiles ARE the A fragment (row f,
//      k-group lane >> 4) of the contraction over those 32 samples, in the permuted k order
//      k = 8 (lane >> 4) + j  <->  t = 16 (j >> 2) + 4 (lane >> 4) + (j & 3): no lane movement, no LDS;
//   3. dw[f][tap] += sum_t S[t][f] x[t + tap - h]: the B fragment of (tile pair p2, tap tile ct) in that k order
//      is the first 8 B of entries o and o + 16, o = 32 p2 + 16 ct + 4 (lane >> 4) + (lane & 15): it depends on
//      2 p2 + ct only, so one fragment read feeds up to 4 pairs x (re, im) = 8 MFMAs.
// The dw accumulators (LEAF_NCT tap tiles x re, im) stay in registers over the whole run and are stored once
// into the workgroup's slab.  Kt > 16 LEAF_NCT - 1 takes the FMA kernel.
// bank -> B fragments of the 16x16x32 forward: slot ((fb16 * 2 + c) * nk32 + kk) * 64 + lane =
// w[c][fb16 * 16 + (lane & 15)][32 kk + 8 (lane >> 4) + 0..7] as bf16
__global__ __launch_bounds__(256) void leaf_pack16_kernel(const float* __restrict__ w, uint4* __restrict__ wpk, int F,
                                                          int Kt, int nk32, int64_t nslot) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nslot) return;
  const int lane = (int)(i & 63);
  const int64_t r = i >> 6;
  const int kk = (int)(r % nk32);
  const int64_t fc = r / nk32;
  const int c = (int)(fc & 1);
  const int f = (int)(fc >> 1) * 16 + (lane & 15);
  const int k0 = 32 * kk + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (f < F && k0 + j < Kt) ? w[((int64_t)c * F + f) * Kt + k0 + j] : 0.f;
  wpk[i] = make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
}

__device__ __forceinline__ f32x4 mfma16(uint4 a, uint4 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a), as_frag(b), c, 0, 0, 0);
}

// grid (nsplit, ceil(F / 64)): units [blockIdx.x * per, + per) of the B * nchunk (clip, chunk) pairs
__global__ __launch_bounds__(256) void leaf_bwd_mfma_kernel(const float* __restrict__ x, const uint4* __restrict__ wpk,
                                                            const float* __restrict__ gP, float* __restrict__ slab,
                                                            int64_t T, int F, int Kt, int nk32, int pool, int Tp, int q,
                                                            int nchunk, int64_t units, int per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char leaf_smem_b[];
  const int Kp = nk32 * 32, nct = nk32 * 2, h = Kt / 2, tpf = pool / 16;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int fb = blockIdx.y;
  const int nalloc = q * pool + Kp + 128;
  uint4* ent = reinterpret_cast<uint4*>(leaf_smem_b);  // [nalloc], every entry staged (zero outside the clip)
  uint4* wl = ent + nalloc;                             // [4 waves][2][nk32][64]
  float* gl = reinterpret_cast<float*>(wl + 8 * nk32 * 64);  // [q][64]: (2 / pool) gP of the unit
  {
    const uint4* wsrc = wpk + (int64_t)fb * 8 * nk32 * 64;
    for (int i = tid; i < 8 * nk32 * 64; i += 256) wl[i] = wsrc[i];
  }
  const int fbase = fb * 64 + wv * 16;
  const bool active = fbase < F;
  f32x4 dacc[LEAF_NCT][2];
#pragma unroll
  for (int ct = 0; ct < LEAF_NCT; ++ct)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int i = 0; i < 4; ++i) dacc[ct][c][i] = 0.f;
  const float gscale = 2.f / (float)pool;
  const int64_t u0 = (int64_t)blockIdx.x * per;
  const int64_t u1 = u0 + per < units ? u0 + per : units;
  for (int64_t u = u0; u < u1; ++u) {
    const int b = (int)(u / nchunk);
    const int j0 = (int)(u - (int64_t)b * nchunk) * q;
    const int nfr = q < Tp - j0 ? q : Tp - j0;
    const int ntile = nfr * tpf;
    const float* xb = x + (int64_t)b * T;
    const int64_t s0 = (int64_t)j0 * pool - h;
    __syncthreads();  // the previous unit is no longer read (and wl is staged)
    for (int o = tid; o < nalloc; o += 256) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int64_t t = s0 + o + j;
        v[j] = (t >= 0 && t < T) ? xb[t] : 0.f;
      }
      ent[o] = make_uint4(pk_bf16(v[0], v[1]), pk_bf16(v[2], v[3]), pk_bf16(v[4], v[5]), pk_bf16(v[6], v[7]));
    }
    for (int i = tid; i < q * 64; i += 256) {
      const int fr = i >> 6, f = fb * 64 + (i & 63);
      gl[i] = (fr < nfr && f < F) ? gP[((int64_t)b * F + f) * Tp + j0 + fr] * gscale : 0.f;
    }
    __syncthreads();
    if (!active) continue;
    for (int grp = 0; grp * 8 < ntile; ++grp) {
      // 1. forward of 8 tiles: A fragment of (tile m, k-step kk) = entry base + 16 (m + 2 kk)
      f32x4 acc[8][2];
#pragma unroll
      for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < 4; ++i) acc[m][c][i] = 0.f;
      const uint4* eb = ent + grp * 128 + (lane & 15) + 8 * (lane >> 4);
      const uint4* bw = wl + wv * 2 * nk32 * 64 + lane;
      uint4 a[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) a[m] = eb[16 * m];
      for (int kk = 0; kk < nk32; ++kk) {
        const uint4 br = bw[kk * 64], bi = bw[(nk32 + kk) * 64];
#pragma unroll
        for (int m = 0; m < 8; ++m) {
          acc[m][0] = mfma16(a[m], br, acc[m][0]);
          acc[m][1] = mfma16(a[m], bi, acc[m][1]);
        }
        if (kk + 1 < nk32) {
#pragma unroll
          for (int m = 0; m < 6; ++m) a[m] = a[m + 2];
          a[6] = eb[16 * (2 * kk + 8)];
          a[7] = eb[16 * (2 * kk + 9)];
        }
      }
      // 2. scale, round, pack: tiles 2 p2 and 2 p2 + 1 -> the contraction's A fragment of pair p2
      float gv[8];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const int ti = grp * 8 + m;
        gv[m] = ti < ntile ? gl[(ti / tpf) * 64 + wv * 16 + (lane & 15)] : 0.f;
      }
      uint4 sfr[4][2];
#pragma unroll
      for (int p2 = 0; p2 < 4; ++p2)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const f32x4 lo = acc[2 * p2][c], hi = acc[2 * p2 + 1][c];
          const float g0 = gv[2 * p2], g1 = gv[2 * p2 + 1];
          const bool v0 = grp * 8 + 2 * p2 < ntile, v1 = grp * 8 + 2 * p2 + 1 < ntile;
          sfr[p2][c] = make_uint4(v0 ? pk_bf16(lo[0] * g0, lo[1] * g0) : 0u, v0 ? pk_bf16(lo[2] * g0, lo[3] * g0) : 0u,
                                  v1 ? pk_bf16(hi[0] * g1, hi[1] * g1) : 0u, v1 ? pk_bf16(hi[2] * g1, hi[3] * g1) : 0u);
        }
      // 3. contraction along the diagonals gi = 2 p2 + ct
      const uint2* e2 = reinterpret_cast<const uint2*>(ent + grp * 128 + 4 * (lane >> 4) + (lane & 15));
#pragma unroll
      for (int gi = 0; gi < LEAF_NCT + 6; ++gi) {
        if (gi < nct + 6) {
          const uint2 lo = e2[2 * (16 * gi)], hi = e2[2 * (16 * gi + 16)];
          const uint4 fx = make_uint4(lo.x, lo.y, hi.x, hi.y);
#pragma unroll
          for (int p2 = 0; p2 < 4; ++p2) {
            const int ct = gi - 2 * p2;
            if (ct >= 0 && ct < LEAF_NCT) {
              if (ct < nct) {
                dacc[ct][0] = mfma16(sfr[p2][0], fx, dacc[ct][0]);
                dacc[ct][1] = mfma16(sfr[p2][1], fx, dacc[ct][1]);
              }
            }
          }
        }
      }
    }
  }
  if (!active) return;
#pragma unroll
  for (int ct = 0; ct < LEAF_NCT; ++ct) {
    if (ct < nct) {
      const int k = 16 * ct + (lane & 15);
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int f = fbase + 4 * (lane >> 4) + i;
          if (f < F && k < Kt) slab[(((int64_t)blockIdx.x * 2 + c) * F + f) * Kt + k] = dacc[ct][c][i];
        }
    }
  }
}

// ------------------------------------------------------------------------------------------- PCEN (pcen_math.h)
__global__ __launch_bounds__(256) void pcen_fwd_kernel(const float* __restrict__ P, const float* __restrict__ r,
                                                       const float* __restrict__ delta, float eps, float* __restrict__ y,
                                                       int F, int Tp, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t row = i / Tp;
  const int j = (int)(i - row * Tp), f = (int)(row % F);
  y[i] = pcen_fwd_value(P + row * Tp, Tp, j, eps, r[f], delta[f]);
}

// grid (F, B): one (clip, filter) row; gP carries the direct path and the path through the 5-tap mean; the row's
// dr / ddelta terms are summed in a fixed order into part[b][f][2] (double)
__global__ __launch_bounds__(256) void pcen_bwd_kernel(const float* __restrict__ P, const float* __restrict__ r,
                                                       const float* __restrict__ delta, float eps,
                                                       const float* __restrict__ gy, float* __restrict__ gP,
                                                       double* __restrict__ part, int F, int Tp) {
  __shared__ double red[1][2][256];
  const int f = blockIdx.x, b = blockIdx.y;
  const int64_t row = (int64_t)b * F + f;
  const float* pr = P + row * Tp;
  const float* gr = gy + row * Tp;
  const float rf = r[f], df = delta[f];
  double sr = 0.0, sd = 0.0;
  for (int i = threadIdx.x; i < Tp; i += 256) {
    float g = 0.f;
#pragma unroll
    for (int d = -2; d <= 2; ++d) {
      const int j = i + d;
      if (j < 0 || j >= Tp) continue;
      const PcenTap tp = pcen_bwd_tap(pr, Tp, j, eps, gr[j], rf, df);
      g += tp.via_m;
      if (d == 0) {
        g += tp.direct;
        sr += (double)tp.dr;
        sd += (double)tp.ddelta;
      }
    }
    gP[row * Tp + i] = g;
  }
  pcen_row_tree<1>(red, &sr, &sd);
  if (threadIdx.x == 0) {
    part[row * 2] = red[0][0][0];
    part[row * 2 + 1] = red[0][1][0];
  }
}

template <typename K>
int leaf_set_lds(K kernel, int bytes, const char* what) {
  if (bytes <= 48 * 1024) return 0;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     bytes);
  if (e != hipSuccess) return mia::fail(-(int)e, "%s: %d B of LDS refused: %s", what, bytes, hipGetErrorString(e));
  return 0;
}

int pcen_check(int32_t B, int32_t F, int32_t Tp) {
  MIA_CHECK_ARG(B >= 1 && B <= 65535 && F >= 1 && F <= 1 << 24 && Tp >= 1, "pcen: bad shape B=%d F=%d Tp=%d", B, F, Tp);
  return 0;
}

}  // namespace

extern "C" int64_t mia_leaf_workspace_bytes(int32_t B, int64_t T, int32_t F, int32_t Kt, int32_t pool, int32_t backward) {
  LeafPlan pl;
  if (leaf_plan(B, T, F, Kt, pool, pl)) return -1;
  if (!backward) return pl.pack_bytes;
  // either compute mode must fit: the FMA slabs, or the MFMA path's packed bank followed by its slabs
  const int64_t m = pl.mbwd ? pl.pack16_bytes + pl.slabb_bytes : 0;
  return m > pl.slab_bytes ? m : pl.slab_bytes;
}

extern "C" int mia_leaf_energy_fwd(const float* x, const float* w, float* P, int32_t B, int64_t T, int32_t F, int32_t Kt,
                                   int32_t pool, int32_t compute, void* workspace, mia_stream_t stream) {
  LeafPlan pl;
  if (int rc = leaf_plan(B, T, F, Kt, pool, pl)) return rc;
  MIA_CHECK_ARG(x && w && P, "mia_leaf_energy_fwd: null pointer");
  MIA_CHECK_ARG(compute == MIA_F32 || compute == MIA_BF16, "mia_leaf_energy_fwd: compute %d", compute);
  hipStream_t s = as_stream(stream);
  if (compute == MIA_F32) {
    if (int rc = leaf_set_lds(leaf_fwd_fma_kernel<false>, pl.lds_fwd, "mia_leaf_energy_fwd")) return rc;
    leaf_fwd_fma_kernel<false><<<dim3(pl.Tp, pl.nfg, B), 256, pl.lds_fwd, s>>>(x, w, P, T, F, Kt, pool, pl.Tp);
    MIA_LAUNCH_CHECK("mia_leaf_energy_fwd");
    return 0;
  }
  MIA_CHECK_ARG(workspace, "mia_leaf_energy_fwd: the bf16 path needs mia_leaf_workspace_bytes(.., 0) of workspace");
  uint4* wpk = reinterpret_cast<uint4*>(workspace);
  const int64_t nslot = pl.pack_bytes / 16;
  leaf_pack_kernel<<<(unsigned)cdiv(nslot, 256), 256, 0, s>>>(w, wpk, F, Kt, pl.nk, nslot);
  MIA_LAUNCH_CHECK("mia_leaf_energy_fwd (pack)");
  const dim3 grid((unsigned)cdiv(pl.Tp, pl.q), pl.nfb, B);
  if (pl.wlds) {
    if (int rc = leaf_set_lds(leaf_fwd_mfma_kernel<true>, pl.lds_mfma, "mia_leaf_energy_fwd")) return rc;
    leaf_fwd_mfma_kernel<true><<<grid, 256, pl.lds_mfma, s>>>(x, wpk, P, T, F, pl.h, pl.nk, pool, pl.Tp, pl.q);
  } else {
    if (int rc = leaf_set_lds(leaf_fwd_mfma_kernel<false>, pl.lds_mfma, "mia_leaf_energy_fwd")) return rc;
    leaf_fwd_mfma_kernel<false><<<grid, 256, pl.lds_mfma, s>>>(x, wpk, P, T, F, pl.h, pl.nk, pool, pl.Tp, pl.q);
  }
  MIA_LAUNCH_CHECK("mia_leaf_energy_fwd");
  return 0;
}

extern "C" int mia_leaf_energy_bwd(const float* x, const float* w, const float* gP, float* dw, int32_t B, int64_t T,
                                   int32_t F, int32_t Kt, int32_t pool, int32_t compute, void* workspace,
                                   mia_stream_t stream) {
  LeafPlan pl;
  if (int rc = leaf_plan(B, T, F, Kt, pool, pl)) return rc;
  MIA_CHECK_ARG(x && w && gP && dw && workspace, "mia_leaf_energy_bwd: null pointer");
  MIA_CHECK_ARG(compute == MIA_F32 || compute == MIA_BF16, "mia_leaf_energy_bwd: compute %d", compute);
  hipStream_t s = as_stream(stream);
  const int64_t n = (int64_t)2 * F * Kt;
  if (compute == MIA_BF16 && pl.mbwd) {
    uint4* wpk = reinterpret_cast<uint4*>(workspace);
    float* slabm = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(workspace) + pl.pack16_bytes);
    const int64_t nslot = pl.pack16_bytes / 16;
    leaf_pack16_kernel<<<(unsigned)cdiv(nslot, 256), 256, 0, s>>>(w, wpk, F, Kt, pl.nk32, nslot);
    MIA_LAUNCH_CHECK("mia_leaf_energy_bwd (pack)");
    if (int rc = leaf_set_lds(leaf_bwd_mfma_kernel, pl.lds_mbwd, "mia_leaf_energy_bwd")) return rc;
    leaf_bwd_mfma_kernel<<<dim3(pl.nsplitb, pl.nfb64), 256, pl.lds_mbwd, s>>>(
        x, wpk, gP, slabm, T, F, Kt, pl.nk32, pool, pl.Tp, pl.qb, pl.nchunkb, pl.unitsb, pl.perb);
    MIA_LAUNCH_CHECK("mia_leaf_energy_bwd");
    leaf_slab_reduce_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(slabm, dw, n, pl.nsplitb);
    MIA_LAUNCH_CHECK("mia_leaf_energy_bwd (reduce)");
    return 0;
  }
  float* slab = reinterpret_cast<float*>(workspace);
  const dim3 grid(pl.nsplit, pl.nfg);
  if (compute == MIA_F32) {
    if (int rc = leaf_set_lds(leaf_bwd_fma_kernel<false>, pl.lds_bwd, "mia_leaf_energy_bwd")) return rc;
    leaf_bwd_fma_kernel<false><<<grid, 256, pl.lds_bwd, s>>>(x, w, gP, slab, T, F, Kt, pool, pl.Tp, pl.frames, pl.per);
  } else {
    if (int rc = leaf_set_lds(leaf_bwd_fma_kernel<true>, pl.lds_bwd, "mia_leaf_energy_bwd")) return rc;
    leaf_bwd_fma_kernel<true><<<grid, 256, pl.lds_bwd, s>>>(x, w, gP, slab, T, F, Kt, pool, pl.Tp, pl.frames, pl.per);
  }
  MIA_LAUNCH_CHECK("mia_leaf_energy_bwd");
  leaf_slab_reduce_kernel<<<(unsigned)cdiv(n, 256), 256, 0, s>>>(slab, dw, n, pl.nsplit);
  MIA_LAUNCH_CHECK("mia_leaf_energy_bwd (reduce)");
  return 0;
}

extern "C" int64_t mia_pcen_workspace_bytes(int32_t B, int32_t F) {
  return B >= 1 && F >= 1 ? (int64_t)B * F * 2 * 8 : -1;
}

extern "C" int mia_pcen_fwd(const float* P, const float* r, const float* delta, float eps, float* y, int32_t B, int32_t F,
                            int32_t Tp, mia_stream_t stream) {
  if (int rc = pcen_check(B, F, Tp)) return rc;
  MIA_CHECK_ARG(P && r && delta && y, "mia_pcen_fwd: null pointer");
  const int64_t n = (int64_t)B * F * Tp;
  MIA_CHECK_ARG(cdiv(n, 256) <= INT32_MAX, "mia_pcen_fwd: too many elements");
  pcen_fwd_kernel<<<(unsigned)cdiv(n, 256), 256, 0, as_stream(stream)>>>(P, r, delta, eps, y, F, Tp, n);
  MIA_LAUNCH_CHECK("mia_pcen_fwd");
  return 0;
}

extern "C" int mia_pcen_bwd(const float* P, const float* r, const float* delta, float eps, const float* gy, float* gP,
                            float* dr, float* ddelta, void* workspace, int32_t B, int32_t F, int32_t Tp,
                            mia_stream_t stream) {
  if (int rc = pcen_check(B, F, Tp)) return rc;
  MIA_CHECK_ARG(P && r && delta && gy && gP && dr && ddelta && workspace, "mia_pcen_bwd: null pointer");
  hipStream_t s = as_stream(stream);
  double* part = reinterpret_cast<double*>(workspace);
  pcen_bwd_kernel<<<dim3(F, B), 256, 0, s>>>(P, r, delta, eps, gy, gP, part, F, Tp);
  MIA_LAUNCH_CHECK("mia_pcen_bwd");
  pcen_param_reduce_kernel<<<(unsigned)cdiv(F, 256), 256, 0, s>>>(part, dr, ddelta, B, F);
  MIA_LAUNCH_CHECK("mia_pcen_bwd (reduce)");
  return 0;
}
