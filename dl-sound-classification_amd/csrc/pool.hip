// Max-pool fused with the preceding BatchNorm-apply + ReLU, and its backward (gfx950).
// nn.MaxPool2d(kernel == stride, floor) after BN+ReLU (envnet_v2.py:16-23, 32-37).
// The pooled layers never materialise relu(bn(x)): the forward reads the raw conv output once and
// writes only the pooled map (+ a u8 argmax per output), the backward scatters the pooled
// gradient through the argmax, masks it with the recomputed ReLU and produces the BN backward
// reductions in the same pass.  Ties keep the first maximum in row-major window order, like the
// PyTorch CPU kernel.
#include <cstdlib>

#include "../../include/miaudio_pool.h"
#include "../../include/miaudio_rowmap.h"
#include "bn_math.h"
#include "channel_partials.h"

namespace {

constexpr int NT = CP_NT;

__device__ __forceinline__ int64_t out_index(int layout, int b, int oy, int ox, int c, int OH, int OW, int C) {
  if (layout == 0) return (((int64_t)b * OH + oy) * OW + ox) * C + c;
  if (layout == 1) return ((int64_t)b * C + c) * OW + ox;                 // (n, c, ow), OH == 1
  return (((int64_t)b * C + c) * OH + oy) * OW + ox;                       // NCHW flat
}

// A/B switch, read at call time: MIA_POOL_V1=1 selects the earlier forms of pool_fwd (run-time window walk,
// per-element transposed stores) and of pool_bwd_gather (per-element gathers of the pooled gradient)
bool pool_v1() { const char* e = getenv("MIA_POOL_V1"); return e && e[0] == '1'; }

// Block ids are dealt round-robin to the 8 XCDs (each with its own L2), so neighbouring blocks that touch the same
// 128-B lines of a channel-major tensor would each fetch them into a different L2.  This bijective relabelling
// gives every group of blocks that share an XCD a contiguous range of logical ids; what a logical block computes
// does not depend on where it runs, so results are unchanged.
__device__ __forceinline__ int xcd_block_id() {
  const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, x = blockIdx.x % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + blockIdx.x / 8;
}

// The window of one (pooled cell, 8-channel group): best = max relu(sc * x + sh), raw = the winner's x, arg its
// position; row-major window order, the first maximum wins (torch's tie rule).  off0 = the element offset of the
// window's first pixel for this group.  KH, KW > 0: a compile-time window (EnvNet's (1, 2) and (5, 3)) -- the
// loops unroll and every load is issued before the first compare; KH == 0: the run-time window (kh, kw).
template <int KH, int KW>
__device__ __forceinline__ void pool_window_dt(const void* __restrict__ x, int dtype, int64_t off0, int W, int C,
                                               int kh, int kw, const float (&sc)[8], const float (&sh)[8],
                                               float (&best)[8], float (&raw)[8], int (&arg)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; raw[i] = 0.f; arg[i] = 0; }
  if constexpr (KH > 0) {
    float f[KH * KW][8];
#pragma unroll
    for (int dy = 0; dy < KH; ++dy)
#pragma unroll
      for (int dx = 0; dx < KW; ++dx) load8(x, dtype, off0 + ((int64_t)dy * W + dx) * C, f[dy * KW + dx]);
#pragma unroll
    for (int pos = 0; pos < KH * KW; ++pos)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float v = bn_relu(f[pos][i], sc[i], sh[i]);
        if (v > best[i]) { best[i] = v; raw[i] = f[pos][i]; arg[i] = pos; }
      }
  } else {
    for (int dy = 0; dy < kh; ++dy) {
      for (int dx = 0; dx < kw; ++dx) {
        float f[8];
        load8(x, dtype, off0 + ((int64_t)dy * W + dx) * C, f);
        const int pos = dy * kw + dx;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float v = bn_relu(f[i], sc[i], sh[i]);
          if (v > best[i]) { best[i] = v; raw[i] = f[i]; arg[i] = pos; }
        }
      }
    }
  }
}

template <int KH, int KW>
__device__ __forceinline__ void pool_window(const void* __restrict__ x, int dtype, int64_t off0, int W, int C, int kh,
                                            int kw, const float (&sc)[8], const float (&sh)[8], float (&best)[8],
                                            float (&raw)[8], int (&arg)[8]) {
  // the dtype as a constant in each arm: no branch between the unrolled loads.  An f32 window of more than 4 pixels
  // walks (its 8 registers a pixel would set the kernel's register count; f32 is not the training step's dtype).
  if (dtype == MIA_BF16) pool_window_dt<KH, KW>(x, MIA_BF16, off0, W, C, kh, kw, sc, sh, best, raw, arg);
  else if constexpr (KH * KW <= 4) pool_window_dt<KH, KW>(x, MIA_F32, off0, W, C, kh, kw, sc, sh, best, raw, arg);
  else pool_window_dt<0, 0>(x, MIA_F32, off0, W, C, kh, kw, sc, sh, best, raw, arg);
}

// one thread = one (output pixel, 8-channel group); <0, 0> is the run-time window (and the MIA_POOL_V1 form)
template <int KH, int KW>
__global__ __launch_bounds__(NT) void pool_fwd_kernel(const void* __restrict__ x, int dtype, int n, int H, int W,
                                                      int C, int kh, int kw, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, void* out, int layout,
                                                      uint8_t* __restrict__ argmax, void* __restrict__ win) {
  if constexpr (KH > 0) { kh = KH; kw = KW; }
  const int OH = H / kh, OW = W / kw, G = C / 8;
  const int total = n * OH * OW * G;  // < 2^31 (checked by the launcher): 32-bit index math
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < total; idx += gridDim.x * NT) {
    const int cg = idx % G;
    int p = idx / G;
    const int ox = p % OW;
    p /= OW;
    const int oy = p % OH;
    const int b = p / OH;
    BnFwd8 bn;
    float best[8], raw[8];
    int arg[8];
    bn.load_or_identity(cg, scale, shift);
    pool_window<KH, KW>(x, dtype, (((int64_t)b * H + oy * kh) * W + ox * kw) * C + cg * 8, W, C, kh, kw, bn.sc, bn.sh,
                        best, raw, arg);
    const int64_t aoff = (((int64_t)b * OH + oy) * OW + ox) * C + cg * 8;
    *reinterpret_cast<uint2*>(argmax + aoff) = argmax_pack(arg);
    if (win) store8(win, dtype, aoff, raw);  // the winner's raw x (exact: x's own dtype) for the backward
    if (layout == 0) {
      store8(out, dtype, aoff, best);  // NHWC: the 8 channels are one 16-B (bf16) / 32-B (f32) run
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) st_elem(out, dtype, out_index(layout, b, oy, ox, cg * 8 + i, OH, OW, C), best[i]);
    }
  }
}

// pool_fwd into a channel-major output (layouts 1 and 2: out[(b * C + c) * S + p], S = OH * OW, p = oy * OW + ox):
// a block owns 64 consecutive cells p of one image x 64 channels.  The windows are walked as in pool_fwd_kernel
// (argmax and win go out as contiguous NHWC runs), the pooled values are rounded to the output dtype into a padded
// LDS tile [channel][cell] and written back as runs along p -- bf16: 8-B stores of 4 cells, started at the row's
// first 8-byte boundary, the ragged ends element by element; f32: one element per lane, 256 B per wave -- like
// pool_apply_t64_kernel (the per-element form scattered 2-B stores S * 2 bytes apart).  Same arithmetic, same bits.
constexpr int PT = 64;  // cells and channels per tile
template <int KH, int KW>
__global__ __launch_bounds__(NT) void pool_fwd_tr_kernel(const void* __restrict__ x, int dtype, int H, int W, int C,
                                                         int kh, int kw, const float* __restrict__ scale,
                                                         const float* __restrict__ shift, void* out,
                                                         uint8_t* __restrict__ argmax, void* __restrict__ win) {
  if constexpr (KH > 0) { kh = KH; kw = KW; }
  __shared__ __attribute__((aligned(16))) float tile_raw[PT * (PT + 1)];
  float(*tf)[PT + 1] = reinterpret_cast<float(*)[PT + 1]>(tile_raw);  // f32: [channel][cell]
  bf16(*tb)[PT + 4] = reinterpret_cast<bf16(*)[PT + 4]>(tile_raw);    // bf16: [channel][cell]
  const int OW = W / kw, S = (H / kh) * OW, G = C / 8;
  const int chunks = (C + PT - 1) / PT, tiles = (S + PT - 1) / PT;
  int bi = xcd_block_id();  // tiles that are neighbours along p (they share output lines) on one L2
  const int chunk = bi % chunks;
  bi /= chunks;
  const int b = bi / tiles, p0 = (bi - b * tiles) * PT;
  const int np = min(PT, S - p0);
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < PT * PT / 8 / NT; ++k) {
    const int q = t + NT * k, r = q >> 3, ch = q & 7;  // cell p0 + r, channels 8 cg .. 8 cg + 7
    const int cg = chunk * (PT / 8) + ch;
    if (r >= np || cg >= G) continue;
    const int p = p0 + r, oy = p / OW, ox = p - oy * OW;
    BnFwd8 bn;
    float best[8], raw[8];
    int arg[8];
    bn.load_or_identity(cg, scale, shift);
    pool_window<KH, KW>(x, dtype, (((int64_t)b * H + oy * kh) * W + ox * kw) * C + cg * 8, W, C, kh, kw, bn.sc, bn.sh,
                        best, raw, arg);
    const int64_t aoff = ((int64_t)b * S + p) * C + cg * 8;
    *reinterpret_cast<uint2*>(argmax + aoff) = argmax_pack(arg);
    if (win) store8(win, dtype, aoff, raw);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (dtype == MIA_BF16) tb[ch * 8 + i][r] = (bf16)best[i];
      else tf[ch * 8 + i][r] = best[i];
    }
  }
  __syncthreads();
  const int nc = min(PT, C - chunk * PT);
  const int64_t row0 = ((int64_t)b * C + chunk * PT) * S + p0;  // out element of (channel 0 of the chunk, cell p0)
  if (dtype == MIA_BF16) {
    bf16* o = reinterpret_cast<bf16*>(out) + row0;
    constexpr int NJ = PT / 4 + 1;  // 4-cell pieces per row, the first one starting up to 3 cells early
    for (int q = t; q < PT * NJ; q += NT) {
      const int c = q / NJ, j = q - c * NJ;
      if (c >= nc) break;
      bf16* dst = o + (int64_t)c * S;
      const int lead = (int)((reinterpret_cast<uintptr_t>(dst) >> 1) & 3);  // cells past an 8-byte boundary
      const int lo = 4 * j - lead;
      if (lo >= 0 && lo + 4 <= np) {
        bf16x4 w4;
#pragma unroll
        for (int i = 0; i < 4; ++i) w4[i] = tb[c][lo + i];
        *reinterpret_cast<bf16x4*>(dst + lo) = w4;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (lo + i >= 0 && lo + i < np) dst[lo + i] = tb[c][lo + i];
      }
    }
  } else {
    float* o = reinterpret_cast<float*>(out) + row0;
    for (int q = t; q < PT * PT; q += NT) {
      const int c = q >> 6, r = q & (PT - 1);
      if (c >= nc) break;
      if (r < np) o[(int64_t)c * S + r] = tf[c][r];
    }
  }
}

// maxpool(relu(bn(x))) before the BN statistics exist (bf16 x, training): relu(s*x + t) is monotone in
// x with the sign of s = gamma*invstd, i.e. of gamma, so the window's winner is the raw maximum
// (gamma > 0), the raw minimum (gamma < 0) or, gamma == 0, the first position (every z ties), always
// the first occurrence -- torch's max_pool2d routing (when relu clamps the whole window the routed
// position differs from torch's first-position pick, but its gradient relu'(z) * g is 0 at either).
// One pass over x: the winner's raw value (bf16) + argmax, and the BN shifted sums about kshift[c]
// (the conv bias) of every pixel -> partial[block][C][2] for mia_bn_finalize_shifted; the pooled
// relu(s*x_win + t) is written by pool_apply_kernel once the statistics are final.
__global__ __launch_bounds__(NT) void pool_raw_stats_kernel(const bf16* __restrict__ x, int n, int H, int W, int C,
                                                            int kh, int kw, const float* __restrict__ gamma,
                                                            const float* __restrict__ kshift, bf16* __restrict__ win,
                                                            uint8_t* __restrict__ argmax, float* __restrict__ partial) {
  const int OH = H / kh, OW = W / kw, G = C / 8;
  const int total = n * OH * OW * G;
  const int cg = threadIdx.x % G;  // constant per thread (G | NT, gridDim*NT a multiple of G)
  float dir[8], ks[8], s1[8], s2[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float gv = gamma[cg * 8 + i];
    dir[i] = gv > 0.f ? 1.f : (gv < 0.f ? -1.f : 0.f);
    ks[i] = kshift[cg * 8 + i];
    s1[i] = 0.f; s2[i] = 0.f;
  }
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < total; idx += gridDim.x * NT) {
    int p = idx / G;
    const int ox = p % OW;
    p /= OW;
    const int oy = p % OH;
    const int b = p / OH;
    float best[8], bestraw[8];
    int arg[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { best[i] = -INFINITY; bestraw[i] = 0.f; arg[i] = 0; }
    for (int dy = 0; dy < kh; ++dy) {
      const int iy = oy * kh + dy;
      const bf16* row = x + (((int64_t)b * H + iy) * W + (int64_t)ox * kw) * C + cg * 8;
#pragma unroll 4
      for (int dx = 0; dx < kw; ++dx) {
        float f[8];
        unpack8(*reinterpret_cast<const uint4*>(row + (int64_t)dx * C), f);
        const int pos = dy * kw + dx;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = f[i] - ks[i];
          s1[i] += d;
          s2[i] = fmaf(d, d, s2[i]);
          const float key = dir[i] * f[i];  // gamma == 0: key 0 everywhere -> first position wins
          if (key > best[i]) { best[i] = key; bestraw[i] = f[i]; arg[i] = pos; }
        }
      }
    }
    const int64_t aoff = (((int64_t)b * OH + oy) * OW + ox) * C + cg * 8;
    *reinterpret_cast<uint2*>(argmax + aoff) = argmax_pack(arg);
    store8(win, MIA_BF16, aoff, bestraw);  // exact: bf16 inputs
  }
  // pixels right of the last full window (W % kw of them per row) enter the statistics only
  const int tailw = W - OW * kw;
  const int ttotal = n * H * tailw * G;
  for (int idx = blockIdx.x * NT + threadIdx.x; idx < ttotal; idx += gridDim.x * NT) {
    int p = idx / G;
    const int tx = p % tailw;
    const int r = p / tailw;  // b * H + iy
    float f[8];
    unpack8(*reinterpret_cast<const uint4*>(x + ((int64_t)r * W + OW * kw + tx) * C + cg * 8), f);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = f[i] - ks[i];
      s1[i] += d;
      s2[i] = fmaf(d, d, s2[i]);
    }
  }
  // block reduction of the shifted sums per channel (threads with equal cg), fixed order
  __shared__ float red[NT][17];
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[threadIdx.x][i] = s1[i]; red[threadIdx.x][8 + i] = s2[i]; }
  __syncthreads();
  if ((int)threadIdx.x < C * 2) {
    const int c = threadIdx.x >> 1, which = threadIdx.x & 1, g = c >> 3, i = c & 7;
    float a = 0.f;
    for (int t = g; t < NT; t += G) a += red[t][which * 8 + i];
    partial[((int64_t)blockIdx.x * C + c) * 2 + which] = a;
  }
}

// pooled output relu(scale*x_win + shift) in the requested layout (see pool_fwd_kernel)
__global__ __launch_bounds__(NT) void pool_apply_kernel(const bf16* __restrict__ win, int n, int OH, int OW, int C,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        void* out, int dtype, int layout) {
  const int64_t total = (int64_t)n * OH * OW * C;
  for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
    const int c = (int)(e % C);
    int64_t p = e / C;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH), b = (int)(p / OH);
    const float v = bn_relu((float)win[e], scale[c], shift[c]);
    st_elem(out, dtype, out_index(layout, b, oy, ox, c, OH, OW, C), v);
  }
}

// pool_apply into the transposed trunk image (layout 1: (n, 64, ow), oh == 1, bf16): a 64-pixel x 64-channel
// tile per block, read as 16-B channel runs, relu(s x + t) rounded to bf16 into a padded LDS tile, written back
// as 8-B runs of 4 pixels per channel row (the per-element form scattered 2-B stores 2 * ow bytes apart:
// 0.107 ms at 1.4 TB/s for the frontend pool of a B = 256 step).  Same arithmetic, same bits.
__global__ __launch_bounds__(256) void pool_apply_t64_kernel(const bf16* __restrict__ win, int OW,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, bf16* __restrict__ out) {
  __shared__ bf16 tile[64][64 + 4];  // [channel][pixel]
  const int tiles = (OW + 63) / 64;
  const int b = blockIdx.x / tiles, p0 = (blockIdx.x - b * tiles) * 64;
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = t + 256 * k, r = q >> 3, ch = q & 7;  // pixel p0 + r, channels 8 ch .. 8 ch + 7
    bf16x8 v = {};
    if (p0 + r < OW) v = *reinterpret_cast<const bf16x8*>(win + ((int64_t)b * OW + p0 + r) * 64 + ch * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = ch * 8 + i;
      tile[c][r] = (bf16)bn_relu((float)v[i], scale[c], shift[c]);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int q = t + 256 * k, c = q >> 4, g = q & 15;  // channel c, pixels p0 + 4 g .. + 3
    const int p = p0 + 4 * g;
    bf16* dst = out + ((int64_t)b * 64 + c) * OW + p;
    const bf16x4 w4 = *reinterpret_cast<const bf16x4*>(&tile[c][4 * g]);
    if (p + 4 <= OW && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
      *reinterpret_cast<bf16x4*>(dst) = w4;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (p + i < OW) dst[i] = w4[i];
    }
  }
}

// one thread = one (input pixel, 8-channel group); block partial reductions like norm.hip
__global__ __launch_bounds__(NT) void pool_bwd_kernel(const void* __restrict__ dout, int layout,
                                                      const uint8_t* __restrict__ argmax, const void* __restrict__ x,
                                                      int dtype, int n, int H, int W, int C, int kh, int kw,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const float* __restrict__ mean,
                                                      const float* __restrict__ invstd, void* dz,
                                                      float* __restrict__ partial) {
  const int OH = H / kh, OW = W / kw, G = C / 8;
  const int t = threadIdx.x;
  const int cg = t % G, rs = t / G, rslots = NT / G;
  BnRed8 bn;
  bn.load(cg, scale, shift, mean, invstd);
  float s1[8] = {0}, s2[8] = {0};
  const int P = n * H * W;  // < 2^31 (checked by the launcher): 32-bit index math
  for (int r = blockIdx.x * rslots + rs; r < P; r += gridDim.x * rslots) {
    const int ix = r % W;
    const int q = r / W;
    const int iy = q % H;
    const int b = q / H;
    const int64_t off = (int64_t)r * C + cg * 8;
    float g[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) g[i] = 0.f;
    const int oy = iy / kh, ox = ix / kw;
    if (oy < OH && ox < OW) {
      const int pos = (iy - oy * kh) * kw + (ix - ox * kw);
      const int64_t aoff = (((int64_t)b * OH + oy) * OW + ox) * C + cg * 8;
      const uint2 am = *reinterpret_cast<const uint2*>(argmax + aoff);
      float xv[8];
      if (dtype == MIA_BF16) {
        unpack8(*reinterpret_cast<const uint4*>(reinterpret_cast<const bf16*>(x) + off), xv);
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[i] = reinterpret_cast<const float*>(x)[off + i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (argmax_byte(am, i) == pos && bn_relu_on(xv[i], bn.sc[i], bn.sh[i])) {
          g[i] = ld_elem(dout, dtype, out_index(layout, b, oy, ox, cg * 8 + i, OH, OW, C));
          bn_red_step(g[i], xv[i], bn.mu[i], bn.is[i], s1[i], s2[i]);
        }
      }
    }
    store8(dz, dtype, off, g);
  }
  cp_fold<2>(s1, s2, C, G, rslots, blockIdx.x, partial);
}

// Sparse BN reductions of the pooled backward: only the argmax position of each pooled cell carries
// a gradient, so dbeta = sum g and dgamma = sum g * xhat are gathered per pooled cell (one thread =
// one (pooled cell, 8-channel group)) without touching the other kh*kw - 1 pixels of the window.
// gm[cell][c] (NHWC cells; f32, or x's dtype: each entry is a dout value or 0, so a bf16 gm converts back to the
// same float) keeps the ReLU-masked gradient at the argmax for the dense pass.
// win (optional, NHWC cells, x's dtype): the raw winner value of each cell saved by the forward
// (pool_raw_stats); when given, x is not gathered at all -- a contiguous read replaces kh*kw-strided
// 2-byte gathers that each touch a separate cache line.
// (the MIA_POOL_V1 oracle of the forms tests: its text stays written out, off bn_math.h and the shared fold)
__global__ __launch_bounds__(NT) void pool_bwd_sparse_kernel(const void* __restrict__ dout, int layout,
                                                             const uint8_t* __restrict__ argmax,
                                                             const void* __restrict__ x,
                                                             const void* __restrict__ win, int dtype, int n, int H,
                                                             int W, int C, int kh, int kw,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             void* __restrict__ gm, int gdt,
                                                             float* __restrict__ partial) {
  const int OH = H / kh, OW = W / kw, G = C / 8;
  const int t = threadIdx.x;
  const int cg = t % G, rs = t / G, rslots = NT / G;
  float sc[8], sh[8], mu[8], is[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    sc[i] = scale[cg * 8 + i]; sh[i] = shift[cg * 8 + i]; mu[i] = mean[cg * 8 + i]; is[i] = invstd[cg * 8 + i];
  }
  float s1[8] = {0}, s2[8] = {0};
  const int cells = n * OH * OW;
  for (int cell = blockIdx.x * rslots + rs; cell < cells; cell += gridDim.x * rslots) {
    const int ox = cell % OW;
    const int q = cell / OW;
    const int oy = q % OH;
    const int b = q / OH;
    float xv[8], dv[8];
    if (win) {
      const int64_t off = (int64_t)cell * C + cg * 8;
      load8(win, dtype, off, xv);
#pragma unroll
      for (int i = 0; i < 8; ++i) dv[i] = ld_elem(dout, dtype, out_index(layout, b, oy, ox, cg * 8 + i, OH, OW, C));
    } else {
      const uint2 am = *reinterpret_cast<const uint2*>(argmax + (int64_t)cell * C + cg * 8);
#pragma unroll
      for (int i = 0; i < 8; ++i) {  // all loads first, unconditionally
        const uint32_t word = i < 4 ? am.x : am.y;
        const int a = (int)((word >> (8 * (i & 3))) & 0xffu);
        const int iy = oy * kh + a / kw, ix = ox * kw + a % kw;
        xv[i] = ld_elem(x, dtype, (((int64_t)b * H + iy) * W + ix) * C + cg * 8 + i);
        dv[i] = ld_elem(dout, dtype, out_index(layout, b, oy, ox, cg * 8 + i, OH, OW, C));
      }
    }
    float gv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float g = fmaf(xv[i], sc[i], sh[i]) > 0.f ? dv[i] : 0.f;
      gv[i] = g;
      s1[i] += g;
      s2[i] = fmaf(g, (xv[i] - mu[i]) * is[i], s2[i]);
    }
    store8(gm, gdt, (int64_t)cell * C + cg * 8, gv);  // bf16 gm: gv is a bf16 value or 0, the rounding is exact
  }
  // cp_fold<2> written out: this kernel is the MIA_POOL_V1 oracle of pool_bwd_sparse_tr_kernel
  // (tests/test_gpu_pool_forms.py) and stays independent of the shared fold that kernel uses
  __shared__ float red[NT * 16];
#pragma unroll
  for (int i = 0; i < 8; ++i) { red[t * 16 + i] = s1[i]; red[t * 16 + 8 + i] = s2[i]; }
  __syncthreads();
  for (int e = t; e < 2 * C; e += NT) {
    const int qq = e / C, c = e % C, g2 = c / 8, ci = c % 8;
    float acc = 0.f;
    for (int r2 = 0; r2 < rslots; ++r2) acc += red[(r2 * G + g2) * 16 + qq * 8 + ci];
    partial[((int64_t)blockIdx.x * C + c) * 2 + qq] = acc;
  }
}

// Eight consecutive elements of a DT-typed array as raw 16-B vectors (bf16: one, f32: two) and their floats: the
// load and the conversion apart, so that a kernel can issue the loads of several iterations before the first use.
template <int DT>
struct Raw8 {
  uint4 v[DT == MIA_BF16 ? 1 : 2];
  __device__ __forceinline__ void load(const void* p, int64_t off) {
    const uint4* q = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(p) + off * (DT == MIA_BF16 ? 2 : 4));
    v[0] = q[0];
    if constexpr (DT != MIA_BF16) v[1] = q[1];
  }
  __device__ __forceinline__ void unpack(float (&f)[8]) const {
    if constexpr (DT == MIA_BF16) {
      unpack8(v[0], f);
    } else {
      const uint32_t w[8] = {v[0].x, v[0].y, v[0].z, v[0].w, v[1].x, v[1].y, v[1].z, v[1].w};
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = __uint_as_float(w[i]);
    }
  }
};

#ifndef PG_DEPTH
// loop iterations whose loads pool_bwd_sparse_ra_kernel issues before the first use.  In the B = 256 EnvNet step the
// three NHWC trunk launches take 21.9-23.8 / 23.0-26.3 / 25.1-27.7 / 27.7-30.0 us at 1 / 2 / 4 / 8:
// with 16-B loads the kernel runs at the rate its bytes arrive, and reading ahead only costs registers
#define PG_DEPTH 1
#endif
// pool_bwd_sparse_kernel for an NHWC pooled gradient with the winners saved (win): same grid, same cell ->
// (block, thread) map, the same per-thread order of adds and the same fold, so gm and partial come out bit for bit.
// Only how the bytes arrive changes: no division decodes the cell (dout and win share gm's offset), a thread's eight
// channels of dout are one 16-B load like win's (bf16; the earlier form issued eight 2-byte loads through
// out_index / ld_elem), and the loads of D consecutive loop iterations are issued before the first use -- clamped
// to the last cell, never under a branch.
template <int DT, int GDT, int D>
__global__ __launch_bounds__(NT) void pool_bwd_sparse_ra_kernel(const void* __restrict__ dout,
                                                                const void* __restrict__ win, int cells, int C,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                void* __restrict__ gm, float* __restrict__ partial) {
  const int G = C / 8;
  const int t = threadIdx.x;
  const int cg = t % G, rs = t / G, rslots = NT / G;
  BnRed8 bn;
  bn.load(cg, scale, shift, mean, invstd);
  float s1[8] = {0}, s2[8] = {0};
  const int stride = gridDim.x * rslots;  // cells + D * stride < 2^31 (checked by the launcher)
  for (int cell0 = blockIdx.x * rslots + rs; cell0 < cells; cell0 += D * stride) {
    Raw8<DT> wr[D], dr[D];
#pragma unroll
    for (int v = 0; v < D; ++v) {
      const int64_t off = (int64_t)min(cell0 + v * stride, cells - 1) * C + cg * 8;
      wr[v].load(win, off);
      dr[v].load(dout, off);
    }
#pragma unroll
    for (int v = 0; v < D; ++v) {
      // no branch around the arithmetic: hipcc sinks an iteration's loads into a branch that holds their only
      // uses, next to the first use, and one iteration is in flight again.  Past the last cell the sums keep
      // their value.
      const bool live = cell0 + v * stride < cells;
      float xv[8], dv[8], gv[8];
      wr[v].unpack(xv);
      dr[v].unpack(dv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        float t1 = s1[i], t2 = s2[i];
        gv[i] = bn.step(i, dv[i], xv[i], t1, t2);
        s1[i] = live ? t1 : s1[i];
        s2[i] = live ? t2 : s2[i];
      }
      if (live) store8(gm, GDT, (int64_t)(cell0 + v * stride) * C + cg * 8, gv);
    }
  }
  cp_fold<2>(s1, s2, C, G, rslots, blockIdx.x, partial);
}

// pool_bwd_sparse_kernel for a channel-major pooled gradient (layouts 1 and 2: dout[(b * C + c) * S + p],
// S = OH * OW) with the winners saved (win): same grid, same cell -> (block, thread) map, same per-thread sums and
// in-block combine, so gm and partial come out bit for bit.  Only the way dout arrives changes: the block's
// rslots consecutive cells x C channels are staged through LDS -- per channel a run of cells that is contiguous
// in memory, read in 4-cell pieces (8 B bf16 / 16 B f32) where the piece is aligned and stays in one image, cell
// by cell at the ragged ends -- instead of eight 2-byte loads from eight cache lines per thread and cell.  The next
// iteration's dout pieces and win row are requested before this iteration's arithmetic.  rslots % 4 == 0 (the
// launcher takes this form from rslots = 16 on).
__global__ __launch_bounds__(NT) void pool_bwd_sparse_tr_kernel(const void* __restrict__ dout,
                                                                const uint8_t* __restrict__ argmax,
                                                                const void* __restrict__ x,
                                                                const void* __restrict__ win, int dtype, int cells,
                                                                int H, int W, int C, int kh, int kw, int lg_nch,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ shift,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                void* __restrict__ gm, int gdt,
                                                                float* __restrict__ partial) {
  const int OW = W / kw, S = (H / kh) * OW, G = C / 8;
  const int t = threadIdx.x;
  const int lb = xcd_block_id();  // the logical block: blocks whose cells share dout lines on one L2
  const int cg = t % G, rs = t / G, rslots = NT / G;
  const int LD = C + 4;  // tile row (one cell) in floats: 16-B aligned rows
  __shared__ __attribute__((aligned(16))) float red[NT * 16];  // the dout tile [rslots][LD] until the final combine
  float* tile = red;
  BnRed8 bn;
  bn.load(cg, scale, shift, mean, invstd);
  float s1[8] = {0}, s2[8] = {0};
  const int es = dtype == MIA_BF16 ? 1 : 2;
  const uintptr_t dbase = reinterpret_cast<uintptr_t>(dout) >> es;  // dout's address in elements
  // piece u of this thread: channel pc[u], cells 4 pk[u] .. + 3 of the block's rslots (C * rslots / 4 = 512 pieces)
  int pc[2], pk[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) { const int q = t + NT * u; pc[u] = q >> lg_nch; pk[u] = q & ((1 << lg_nch) - 1); }
  float pv[2][4], wx[8] = {0};
  auto fetch = [&](int cell0) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c0 = cell0 + 4 * pk[u];
      const int b0 = c0 / S, b3 = (c0 + 3) / S;
      const int64_t i0 = ((int64_t)b0 * C + pc[u]) * S + (c0 - b0 * S);
      if (c0 + 3 < cells && b0 == b3 && ((dbase + (uintptr_t)i0) & 3) == 0) {
        if (dtype == MIA_BF16) {
          const uint2 v = *reinterpret_cast<const uint2*>(reinterpret_cast<const bf16*>(dout) + i0);
          pv[u][0] = bf16_lo(v.x); pv[u][1] = bf16_hi(v.x);
          pv[u][2] = bf16_lo(v.y); pv[u][3] = bf16_hi(v.y);
        } else {
          const float4 v = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(dout) + i0);
          pv[u][0] = v.x; pv[u][1] = v.y; pv[u][2] = v.z; pv[u][3] = v.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int cj = c0 + j, bj = cj / S;
          pv[u][j] = cj < cells ? ld_elem(dout, dtype, ((int64_t)bj * C + pc[u]) * S + (cj - bj * S)) : 0.f;
        }
      }
    }
    if (win && cell0 + rs < cells) load8(win, dtype, (int64_t)(cell0 + rs) * C + cg * 8, wx);
  };
  const int64_t step = (int64_t)gridDim.x * rslots;
  int64_t cell0 = (int64_t)lb * rslots;
  if (cell0 < cells) fetch((int)cell0);
  for (; cell0 < cells; cell0 += step) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) tile[(4 * pk[u] + j) * LD + pc[u]] = pv[u][j];
    float xv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) xv[i] = wx[i];
    __syncthreads();
    if (cell0 + step < cells) fetch((int)(cell0 + step));
    const int64_t cell = cell0 + rs;
    if (cell < cells) {
      const float4 d0 = *reinterpret_cast<const float4*>(tile + rs * LD + cg * 8);
      const float4 d1 = *reinterpret_cast<const float4*>(tile + rs * LD + cg * 8 + 4);
      const float dv[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
      if (!win) {  // no saved winners: gather x at the argmax positions, as pool_bwd_sparse_kernel does
        const int b = (int)cell / S, p = (int)cell - b * S, oy = p / OW, ox = p - oy * OW;
        const uint2 am = *reinterpret_cast<const uint2*>(argmax + cell * C + cg * 8);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int a = argmax_byte(am, i);
          const int iy = oy * kh + a / kw, ix = ox * kw + a % kw;
          xv[i] = ld_elem(x, dtype, (((int64_t)b * H + iy) * W + ix) * C + cg * 8 + i);
        }
      }
      float gv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) gv[i] = bn.step(i, dv[i], xv[i], s1[i], s2[i]);
      store8(gm, gdt, cell * C + cg * 8, gv);
    }
    __syncthreads();  // also the barrier between the last tile reads and the fold's writes to red
  }
  cp_fold<2>(s1, s2, C, G, rslots, lb, partial, red);
}

// Dense BN backward of a pooled layer in one pass: dx = gamma*invstd*(g - dbeta/P - xhat*dgamma/P)
// with g = gm[cell] at the argmax position of the pixel's pooled cell, 0 elsewhere (gm already
// carries the ReLU mask).  Reads x once, writes dx once; the masked dense gradient is never
// materialised.  s1 partials = dbias.  All loads are unconditional (a conditional load makes hipcc
// wait vmcnt(0) in the loop); four pixels per thread-iteration.
// Same pass for pool windows kw % 8 == 0 (the frontend (1, 64) pool): a thread owns 8 channels x
// 8 consecutive pixels of one row, which always fall in ONE pooled cell, so the cell's argmax bytes
// and masked gradient (40 B) are read once per 8 pixels instead of once per pixel, and the index
// math runs once per octet.  All 8 pixel loads are issued before any use.
template <int GDT>  // gm's dtype
__global__ __launch_bounds__(NT) void pool_bn_bwd_apply_oct_kernel(const void* __restrict__ gm,
                                                                   const uint8_t* __restrict__ argmax,
                                                                   const bf16* __restrict__ x, int n, int H, int W,
                                                                   int C, int kh, int kw, FastDiv dNO, FastDiv dH,
                                                                   FastDiv dG, const float* __restrict__ gamma,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd,
                                                                   const float* __restrict__ dgamma,
                                                                   const float* __restrict__ dbeta, bf16* dx,
                                                                   float* __restrict__ partial) {
  const int OH = H / kh, OW = W / kw, G = C / 8, NO = (W + 7) / 8;
  const int t = threadIdx.x;
  const int cg = t % G;
  const int P = n * H * W;
  BnApply8 bn;
  bn.load(cg, gamma, mean, invstd, dgamma, dbeta, 1.f / (float)P);
  float s1[8] = {0};
  const int64_t units = (int64_t)n * H * NO * G;
  for (int64_t u = (int64_t)blockIdx.x * NT + t; u < units; u += (int64_t)gridDim.x * NT) {
    const int rest = (int)fdiv((uint32_t)(u), dG);       // (b*H + iy)*NO + o8   (units < 2^31 checked)
    const int rowi = (int)fdiv((uint32_t)rest, dNO);     // b*H + iy
    const int o8 = rest - rowi * NO;
    const int iy = rowi - (int)fdiv((uint32_t)rowi, dH) * H;
    const int b = (rowi - iy) / H;
    const int ix0 = o8 * 8;
    const int oy = iy / kh, ox = ix0 / kw;
    const bool cell = oy < OH && ox < OW;
    const int64_t coff = cell ? (((int64_t)b * OH + oy) * OW + ox) * C + cg * 8 : 0;
    const uint2 am = *reinterpret_cast<const uint2*>(argmax + coff);
    Raw8<GDT> gr;
    gr.load(gm, coff);
    const int64_t xoff = ((int64_t)rowi * W + ix0) * C + cg * 8;
    uint4 xr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t o = ix0 + j < W ? xoff + (int64_t)j * C : xoff;
      xr[j] = *reinterpret_cast<const uint4*>(x + o);
    }
    float gv[8];
    gr.unpack(gv);
    const int pos0 = (iy - oy * kh) * kw + (ix0 - ox * kw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (ix0 + j >= W) break;
      const uint32_t w4[4] = {xr[j].x, xr[j].y, xr[j].z, xr[j].w};
      uint32_t o4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float g[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int i = 2 * q + h;
          const float xv = h ? bf16_hi(w4[q]) : bf16_lo(w4[q]);
          const float gi = cell && argmax_byte(am, i) == pos0 + j ? gv[i] : 0.f;
          g[h] = bn.dx(i, gi, xv);
          s1[i] += g[h];
        }
        o4[q] = pk_bf16(g[0], g[1]);
      }
      *reinterpret_cast<uint4*>(dx + xoff + (int64_t)j * C) = uint4{o4[0], o4[1], o4[2], o4[3]};
    }
  }
  if (partial) cp_fold<1>(s1, nullptr, C, G, NT / G, blockIdx.x, partial);
}

// Same pass for short pool windows (kw = 2..4, the trunk's (5, 3) and (1, 2) pools): a thread owns 8
// channels x the KW pixels of one row that fall in one pooled cell (a "run"); the cell's argmax bytes
// and masked gradient are read once per run and the index math runs once per run.  Pixels past the
// last whole cell (W % kw, H % kh) form runs with no cell (gradient term 0).  RU runs per
// thread-iteration, all loads issued before any use.  EnvNet block 0 (B = 256, 50 x 846 x 32, (5, 3)):
// 0.447 ms per pixel -> 0.345 ms per run (4.25 TB/s on x + dx + gm); folding the five per-channel
// constants into three (occupancy 4 -> 5) measured no faster.
// RM: dx through a row map (RowMap, common.h): pixel ix of row b*H + iy is stored at pixel lead + (b*H + iy) * rowpx +
// ix.  The thread that owns a row's last run also zeroes that row's pixels W .. rowpx - 1, the one that owns run 0
// of row 0 the lead pixels, block 0 the zero pixel -- same grid, same runs, same sums.
template <int KW, int RU, int GDT, bool RM = false>
__global__ __launch_bounds__(NT) void pool_bn_bwd_apply_run_kernel(const void* __restrict__ gm,
                                                                   const uint8_t* __restrict__ argmax,
                                                                   const bf16* __restrict__ x, int n, int H, int W,
                                                                   int C, int kh, FastDiv dNR, FastDiv dH, FastDiv dG,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd,
                                                                   const float* __restrict__ dgamma,
                                                                   const float* __restrict__ dbeta, bf16* dx,
                                                                   float* __restrict__ partial, RowMap rm = RowMap{}) {
  const int OH = H / kh, OW = W / KW, G = C / 8, NR = (W + KW - 1) / KW;
  const int t = threadIdx.x;
  const int cg = t % G;
  const int P = n * H * W;
  if constexpr (RM) {
    if (rm.zp && blockIdx.x == 0)
      for (int i = t; i < rm.zc16; i += NT) reinterpret_cast<uint4*>(rm.zp)[i] = uint4{0u, 0u, 0u, 0u};
  }
  BnApply8 bn;
  bn.load(cg, gamma, mean, invstd, dgamma, dbeta, 1.f / (float)P);
  float s1[8] = {0};
  const int units = n * H * NR * G;  // < 2^31 (checked by the launcher)
  const int stride = gridDim.x * NT;
  for (int u0 = blockIdx.x * NT + t; u0 < units; u0 += RU * stride) {
    uint4 xr[RU][KW];
    uint2 am[RU];
    Raw8<GDT> gr[RU];
    int64_t xoff[RU];
    int64_t doff[RU];  // RM: where the run's first pixel goes in dx
    int pos0[RU], ix0[RU];
    bool first[RU];
#pragma unroll
    for (int v = 0; v < RU; ++v) {
      const int u = min(u0 + v * stride, units - 1);
      const int rest = (int)fdiv((uint32_t)u, dG);        // (b*H + iy)*NR + run
      const int rowi = (int)fdiv((uint32_t)rest, dNR);    // b*H + iy
      const int run = rest - rowi * NR;
      const int b = (int)fdiv((uint32_t)rowi, dH);
      const int iy = rowi - b * H;
      ix0[v] = run * KW;
      const int oy = iy / kh;
      const bool cell = oy < OH && run < OW;
      const int64_t coff = cell ? (((int64_t)b * OH + oy) * OW + run) * C + cg * 8 : 0;
      pos0[v] = cell ? (iy - oy * kh) * KW : -256;
      am[v] = *reinterpret_cast<const uint2*>(argmax + coff);
      gr[v].load(gm, coff);
      xoff[v] = ((int64_t)rowi * W + ix0[v]) * C + cg * 8;
      if constexpr (RM) {
        doff[v] = (rm.lead + (int64_t)rowi * rm.rowpx + ix0[v]) * C + cg * 8;
        first[v] = rest == 0;
      } else {
        doff[v] = xoff[v];
        first[v] = false;
      }
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        const int64_t o = ix0[v] + j < W ? xoff[v] + (int64_t)j * C : xoff[v];
        xr[v][j] = *reinterpret_cast<const uint4*>(x + o);
      }
    }
#pragma unroll
    for (int v = 0; v < RU; ++v) {
      if (u0 + v * stride >= units) break;
      float gv[8];
      gr[v].unpack(gv);
#pragma unroll
      for (int j = 0; j < KW; ++j) {
        if (ix0[v] + j >= W) break;
        const uint32_t w4[4] = {xr[v][j].x, xr[v][j].y, xr[v][j].z, xr[v][j].w};
        uint32_t o4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float g[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int i = 2 * q + h;
            const float xv = h ? bf16_hi(w4[q]) : bf16_lo(w4[q]);
            const float gi = argmax_byte(am[v], i) == pos0[v] + j ? gv[i] : 0.f;
            g[h] = bn.dx(i, gi, xv);
            s1[i] += g[h];
          }
          o4[q] = pk_bf16(g[0], g[1]);
        }
        *reinterpret_cast<uint4*>(dx + doff[v] + (int64_t)j * C) = uint4{o4[0], o4[1], o4[2], o4[3]};
      }
      if constexpr (RM) {
        if (ix0[v] + KW >= W)  // the row's last run: its zero pixels W .. rowpx - 1
          for (int px = W - ix0[v]; px < rm.rowpx - ix0[v]; ++px)
            *reinterpret_cast<uint4*>(dx + doff[v] + (int64_t)px * C) = uint4{0u, 0u, 0u, 0u};
        if (first[v])
          for (int px = 0; px < rm.lead; ++px)
            *reinterpret_cast<uint4*>(dx + (int64_t)px * C + cg * 8) = uint4{0u, 0u, 0u, 0u};
      }
    }
  }
  if (partial) cp_fold<1>(s1, nullptr, C, G, NT / G, blockIdx.x, partial);
}

#ifndef PB_UNROLL
#define PB_UNROLL 4
#endif
#ifndef PB_NB
#define PB_NB CP_MAXBLK  // the partial slab holds no more rows
#endif
#ifndef PB_RUNS
#define PB_RUNS 1  // runs per thread-iteration: 1, 2, 3 measured equal within 5% (block 0: 0.34-0.36 ms)
#endif
// the per-pixel form (MIA_POOL_BWD_PIXEL, and every f32 / long-window layer): the oracle of the run and octet forms
// in tests/test_gpu_pool_forms.py, so its prologue and apply expression stay written out, off bn_math.h
template <int GDT>
__global__ __launch_bounds__(NT) void pool_bn_bwd_apply_kernel(const void* __restrict__ gm,
                                                               const uint8_t* __restrict__ argmax,
                                                               const void* __restrict__ x, int dtype, int n, int H,
                                                               int W, int C, int kh, int kw, FastDiv dW, FastDiv dH,
                                                               FastDiv dkw, FastDiv dkh,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ invstd,
                                                               const float* __restrict__ dgamma,
                                                               const float* __restrict__ dbeta, void* dx,
                                                               float* __restrict__ partial) {
  const int OH = H / kh, OW = W / kw, G = C / 8;
  const int t = threadIdx.x;
  const int cg = t % G, rs = t / G, rslots = NT / G;
  const int P = n * H * W;
  float mu[8], is[8], a[8], mb[8], mg[8];
  const float invP = 1.f / (float)P;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = cg * 8 + i;
    mu[i] = mean[c]; is[i] = invstd[c];
    a[i] = (gamma ? gamma[c] : 1.f) * is[i];
    mb[i] = dbeta[c] * invP;
    mg[i] = dgamma[c] * invP;
  }
  float s1[8] = {0};
  const int stride = gridDim.x * rslots;
  for (int r0 = blockIdx.x * rslots + rs; r0 < P; r0 += PB_UNROLL * stride) {
    float xv[PB_UNROLL][8];
    uint2 am[PB_UNROLL];
    Raw8<GDT> gr[PB_UNROLL];
#pragma unroll
    for (int u = 0; u < PB_UNROLL; ++u) {
      const int r = min(r0 + u * stride, P - 1);
      load8(x, dtype, (int64_t)r * C + cg * 8, xv[u]);
      const int q = (int)fdiv(r, dW), ix = r - q * W;
      const int b = (int)fdiv(q, dH), iy = q - b * H;
      const int oy = min((int)fdiv(iy, dkh), OH - 1), ox = min((int)fdiv(ix, dkw), OW - 1);
      const int64_t coff = (((int64_t)b * OH + oy) * OW + ox) * C + cg * 8;
      am[u] = *reinterpret_cast<const uint2*>(argmax + coff);
      gr[u].load(gm, coff);
    }
#pragma unroll
    for (int u = 0; u < PB_UNROLL; ++u) {
      const int r = r0 + u * stride;
      if (r >= P) break;
      const int q = (int)fdiv(r, dW), ix = r - q * W;
      const int iy = q - (int)fdiv(q, dH) * H;
      const int oy = (int)fdiv(iy, dkh), ox = (int)fdiv(ix, dkw);
      const int pos = oy < OH && ox < OW ? (iy - oy * kh) * kw + (ix - ox * kw) : -1;
      float gv[8];
      gr[u].unpack(gv);
      float g[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const uint32_t word = i < 4 ? am[u].x : am[u].y;
        const int av = (int)((word >> (8 * (i & 3))) & 0xffu);
        const float gi = av == pos ? gv[i] : 0.f;
        g[i] = a[i] * (gi - mb[i] - (xv[u][i] - mu[i]) * is[i] * mg[i]);
        s1[i] += g[i];
      }
      store8(dx, dtype, (int64_t)r * C + cg * 8, g);
    }
  }
  if (partial) cp_fold<1>(s1, nullptr, C, G, rslots, blockIdx.x, partial);
}

// out[b][ih][iw] = sum_ky p[b][ih-ky][iw][ky]
__global__ void col2im_rows_kernel(const float* __restrict__ p, int n, int ph, int w, int kh, void* out, int dtype) {
  const int H = ph + kh - 1;
  const int total = n * H * w;  // < 2^31 (checked by the launcher)
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int iw = idx % w;
    const int q = idx / w;
    const int ih = q % H;
    const int b = q / H;
    float s = 0.f;
    for (int ky = 0; ky < kh; ++ky) {
      const int r = ih - ky;
      if (r >= 0 && r < ph) s += p[(((int64_t)b * ph + r) * w + iw) * kh + ky];
    }
    st_elem(out, dtype, idx, s);
  }
}

}  // namespace

extern "C" int mia_pool_fwd(const void* x, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh,
                            int32_t kw, const float* scale, const float* shift, void* out, int32_t out_layout,
                            uint8_t* argmax, void* win, mia_stream_t stream) {
  MIA_CHECK_ARG(x && out && argmax, "pool_fwd: null pointer");
  MIA_CHECK_ARG(!win || (reinterpret_cast<uintptr_t>(win) & 15) == 0, "pool_fwd: win alignment");
  MIA_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | (out_layout == 0 ? reinterpret_cast<uintptr_t>(out) : 0)) & 15) == 0,
                "pool_fwd: x (and an NHWC out) must be 16-byte aligned");
  MIA_CHECK_ARG(c % 8 == 0 && kh > 0 && kw > 0 && kh * kw <= 256 && h >= kh && w >= kw, "pool_fwd: bad geometry");
  MIA_CHECK_ARG(out_layout >= 0 && out_layout <= 2 && (out_layout != 1 || h / kh == 1), "pool_fwd: bad layout");
  MIA_CHECK_ARG((int64_t)n * h * w * (c / 8) < (1ll << 31), "pool_fwd: too many elements for 32-bit indexing");
  const int64_t total = (int64_t)n * (h / kh) * (w / kw) * (c / 8);
  const int nb = (int)std::min<int64_t>(cdiv(total, NT), 16384);
  hipStream_t s = as_stream(stream);
  const bool v1 = pool_v1();
  const int win_id = v1 ? 0 : (kh == 1 && kw == 2) ? 1 : (kh == 5 && kw == 3) ? 2 : 0;  // the windows EnvNet uses
  const int64_t tblocks = (int64_t)n * cdiv((int64_t)(h / kh) * (w / kw), PT) * cdiv(c, PT);
  if (!v1 && out_layout != 0 && tblocks < (1ll << 31)) {  // channel-major output: through an LDS transpose
    if (win_id == 1)
      pool_fwd_tr_kernel<1, 2><<<(unsigned)tblocks, NT, 0, s>>>(x, dtype, h, w, c, kh, kw, scale, shift, out, argmax, win);
    else if (win_id == 2)
      pool_fwd_tr_kernel<5, 3><<<(unsigned)tblocks, NT, 0, s>>>(x, dtype, h, w, c, kh, kw, scale, shift, out, argmax, win);
    else
      pool_fwd_tr_kernel<0, 0><<<(unsigned)tblocks, NT, 0, s>>>(x, dtype, h, w, c, kh, kw, scale, shift, out, argmax, win);
    MIA_LAUNCH_CHECK("pool_fwd_tr");
    return 0;
  }
  // NHWC output: the (1, 2) window measured no faster unrolled (EnvNet's two: 53.4 -> 51.7 and 87.9 -> 86.3 us) and
  // stays on the run-time walk; (5, 3) went 176 -> 157 us
  if (win_id == 2)
    pool_fwd_kernel<5, 3><<<nb, NT, 0, s>>>(x, dtype, n, h, w, c, kh, kw, scale, shift, out, out_layout, argmax, win);
  else
    pool_fwd_kernel<0, 0><<<nb, NT, 0, s>>>(x, dtype, n, h, w, c, kh, kw, scale, shift, out, out_layout, argmax, win);
  MIA_LAUNCH_CHECK("pool_fwd");
  return 0;
}

extern "C" int mia_pool_raw_stats(const void* x, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                  const float* gamma, const float* kshift, void* win, uint8_t* argmax, float* partial,
                                  int32_t nblocks, mia_stream_t stream) {
  MIA_CHECK_ARG(x && gamma && kshift && win && argmax && partial && nblocks > 0, "pool_raw_stats: null pointer");
  MIA_CHECK_ARG(c % 8 == 0 && c >= 8 && c * 2 <= NT && (NT % (c / 8)) == 0, "pool_raw_stats: channels");
  MIA_CHECK_ARG(h % kh == 0 && w >= kw && kh * kw <= 256, "pool_raw_stats: window geometry");
  MIA_CHECK_ARG((int64_t)n * h * w * (c / 8) < (1ll << 31), "pool_raw_stats: too many elements for 32-bit indexing");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(win)) % 16 == 0 &&
                reinterpret_cast<uintptr_t>(argmax) % 8 == 0, "pool_raw_stats: alignment");
  pool_raw_stats_kernel<<<nblocks, NT, 0, as_stream(stream)>>>(reinterpret_cast<const bf16*>(x), n, h, w, c, kh, kw,
                                                               gamma, kshift, reinterpret_cast<bf16*>(win), argmax,
                                                               partial);
  MIA_LAUNCH_CHECK("pool_raw_stats");
  return 0;
}

extern "C" int mia_pool_apply(const void* win, int32_t n, int32_t oh, int32_t ow, int32_t c, const float* scale,
                              const float* shift, void* out, int32_t dtype, int32_t out_layout, mia_stream_t stream) {
  MIA_CHECK_ARG(win && scale && shift && out && n > 0 && oh > 0 && ow > 0 && c > 0, "pool_apply: bad arguments");
  if (out_layout == 1 && oh == 1 && c == 64 && dtype == MIA_BF16 && (reinterpret_cast<uintptr_t>(win) & 15) == 0 &&
      (int64_t)n * cdiv(ow, 64) < (1ll << 31)) {
    pool_apply_t64_kernel<<<(unsigned)(n * cdiv(ow, 64)), 256, 0, as_stream(stream)>>>(
        reinterpret_cast<const bf16*>(win), ow, scale, shift, reinterpret_cast<bf16*>(out));
    MIA_LAUNCH_CHECK("pool_apply_t64");
    return 0;
  }
  const int64_t total = (int64_t)n * oh * ow * c;
  const int nb = (int)std::min<int64_t>(cdiv(total, NT), 16384);
  pool_apply_kernel<<<nb, NT, 0, as_stream(stream)>>>(reinterpret_cast<const bf16*>(win), n, oh, ow, c, scale, shift,
                                                      out, dtype, out_layout);
  MIA_LAUNCH_CHECK("pool_apply");
  return 0;
}

extern "C" int mia_pool_bwd_bn_relu_reduce(const void* dout, int32_t out_layout, const uint8_t* argmax, const void* x,
                                           int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh,
                                           int32_t kw, const float* scale, const float* shift, const float* mean,
                                           const float* invstd, void* dz, float* dgamma, float* dbeta, void* partial,
                                           mia_stream_t stream) {
  MIA_CHECK_ARG(dout && argmax && x && scale && shift && mean && invstd && dz && dgamma && dbeta && partial,
                "pool_bwd: null pointer");
  MIA_CHECK_ARG(c % 8 == 0 && c >= 8 && (NT % (c / 8)) == 0, "pool_bwd: channels");
  MIA_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "pool_bwd: too many pixels for 32-bit indexing");
  const int rslots = NT / (c / 8);
  const int64_t P = (int64_t)n * h * w;
  hipStream_t s = as_stream(stream);
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(P, (int64_t)rslots * 8), CP_MAXBLK));
  pool_bwd_kernel<<<nb, NT, 0, s>>>(dout, out_layout, argmax, x, dtype, n, h, w, c, kh, kw, scale, shift, mean,
                                    invstd, dz, (float*)partial);
  MIA_LAUNCH_CHECK("pool_bwd");
  cp_final2_kernel<<<(unsigned)c, 256, 0, s>>>((const float*)partial, nb, c, /*q0 = sum g*/ dbeta,
                                               /*q1 = sum g xhat*/ dgamma);
  MIA_LAUNCH_CHECK("pool_bwd_final");
  return 0;
}

// MIA_POOL_GRID=n, read at call time: at most n blocks for mia_pool_bwd_gather's main kernel, whichever form runs,
// and for the run form of mia_pool_bn_relu_bwd_apply (it only lowers the grid; the tests use it to make a thread
// walk many cells at small shapes)
static int pool_grid_cap(int nb) {
  const char* e = getenv("MIA_POOL_GRID");
  const int cap = e ? atoi(e) : 0;
  return cap > 0 ? std::min(nb, cap) : nb;
}

extern "C" int mia_pool_bwd_gather_ex(const void* dout, int32_t out_layout, const uint8_t* argmax, const void* x,
                                      const void* win, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c,
                                      int32_t kh, int32_t kw, const float* scale, const float* shift,
                                      const float* mean, const float* invstd, void* gm, int32_t gm_dtype,
                                      float* dgamma, float* dbeta, void* partial, mia_stream_t stream) {
  MIA_CHECK_ARG(dout && argmax && x && scale && shift && mean && invstd && gm && dgamma && dbeta && partial,
                "pool_bwd_gather: null pointer");
  MIA_CHECK_ARG(c % 8 == 0 && c >= 8 && (NT % (c / 8)) == 0, "pool_bwd_gather: channels");
  MIA_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "pool_bwd_gather: too many pixels for 32-bit indexing");
  // a cell's eight channels are one 16-B (bf16 gm) or two 16-B (f32 gm) stores: 16-byte alignment either way
  MIA_CHECK_ARG(h >= kh && w >= kw && kh * kw <= 256 && (reinterpret_cast<uintptr_t>(gm) & 15) == 0,
                "pool_bwd_gather: bad geometry / alignment");
  MIA_CHECK_ARG(gm_dtype == MIA_F32 || (gm_dtype == MIA_BF16 && dtype == MIA_BF16),
                "pool_bwd_gather: gm is f32, or bf16 beside bf16 activations (gm dtype %d, dtype %d)", gm_dtype, dtype);
  const int rslots = NT / (c / 8);
  const int64_t cells = (int64_t)n * (h / kh) * (w / kw);
  const int nb = pool_grid_cap((int)std::max<int64_t>(1, std::min<int64_t>(cdiv(cells, (int64_t)rslots * 2), CP_MAXBLK)));
  hipStream_t s = as_stream(stream);
  MIA_CHECK_ARG(!win || (reinterpret_cast<uintptr_t>(win) & 15) == 0, "pool_bwd_gather: win alignment");
  const bool v1 = pool_v1();
  const bool chmajor = out_layout == 2 || (out_layout == 1 && h / kh == 1);
  // the staged form from 16 cells a block iteration on (channel runs of 32 B and more; C <= 128): the frontend's
  // gradient (C = 64) went 50 -> 33 us, the last trunk pool's (C = 256, 8 cells, 16-B runs) measured 87 -> 89 us
  if (!v1 && chmajor && rslots >= 16 && cells < (1ll << 31) - 1024) {
    int lg_nch = 0;
    while ((4 << lg_nch) < rslots) ++lg_nch;  // rslots / 4 pieces per channel (rslots divides 256: a power of two)
    pool_bwd_sparse_tr_kernel<<<nb, NT, 0, s>>>(dout, argmax, x, win, dtype, (int)cells, h, w, c, kh, kw, lg_nch, scale,
                                                shift, mean, invstd, gm, gm_dtype, (float*)partial);
  } else if (!v1 && win && out_layout == 0 && (dtype == MIA_BF16 || dtype == MIA_F32) &&
             (reinterpret_cast<uintptr_t>(dout) & 15) == 0 && cells + (int64_t)PG_DEPTH * nb * rslots < (1ll << 31)) {
    // NHWC dout and saved winners: 16-B loads, PG_DEPTH iterations ahead.  (Channel-major dout with 8 cells a block
    // iteration, the last trunk pool: this form with element loads 1 / 2 / 4 / 8 iterations ahead measured 78 ->
    // 78-85 / 82-89 / 86-89 / 106-132 us: not kept, it stays on pool_bwd_sparse_kernel.)
    float* part = (float*)partial;
    const int nc = (int)cells;
    if (dtype == MIA_F32)
      pool_bwd_sparse_ra_kernel<MIA_F32, MIA_F32, PG_DEPTH><<<nb, NT, 0, s>>>(dout, win, nc, c, scale, shift, mean,
                                                                              invstd, gm, part);
    else if (gm_dtype == MIA_F32)
      pool_bwd_sparse_ra_kernel<MIA_BF16, MIA_F32, PG_DEPTH><<<nb, NT, 0, s>>>(dout, win, nc, c, scale, shift, mean,
                                                                               invstd, gm, part);
    else
      pool_bwd_sparse_ra_kernel<MIA_BF16, MIA_BF16, PG_DEPTH><<<nb, NT, 0, s>>>(dout, win, nc, c, scale, shift, mean,
                                                                                invstd, gm, part);
  } else {
    pool_bwd_sparse_kernel<<<nb, NT, 0, s>>>(dout, out_layout, argmax, x, win, dtype, n, h, w, c, kh, kw, scale, shift,
                                             mean, invstd, gm, gm_dtype, (float*)partial);
  }
  MIA_LAUNCH_CHECK("pool_bwd_gather");
  cp_final2_kernel<<<(unsigned)c, 256, 0, s>>>((const float*)partial, nb, c, /*q0 = sum g*/ dbeta,
                                               /*q1 = sum g xhat*/ dgamma);
  MIA_LAUNCH_CHECK("pool_bwd_gather_final");
  return 0;
}

extern "C" int mia_pool_bwd_gather(const void* dout, int32_t out_layout, const uint8_t* argmax, const void* x,
                                   const void* win, int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                   const float* scale, const float* shift, const float* mean, const float* invstd,
                                   float* gm, float* dgamma, float* dbeta, void* partial, mia_stream_t stream) {
  return mia_pool_bwd_gather_ex(dout, out_layout, argmax, x, win, dtype, n, h, w, c, kh, kw, scale, shift, mean, invstd,
                                gm, MIA_F32, dgamma, dbeta, partial, stream);
}

template <int GDT>
static int pool_bn_bwd_apply_launch(const void* gm, const uint8_t* argmax, const void* x, int32_t dtype, int32_t n,
                                    int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw, const float* gamma,
                                    const float* mean, const float* invstd, const float* dgamma, const float* dbeta,
                                    void* dx, float* dbias, void* partial, hipStream_t s, const RowMap& rm) {
  const bool mapped = rm.lead != 0 || rm.rowpx != w || rm.zp;
  const int rslots = NT / (c / 8);
  const int64_t P = (int64_t)n * h * w;
  const int64_t units = (int64_t)n * h * ((w + 7) / 8) * (c / 8);
  // every form ends the same way: its launch check, then the final pass of the dx sums (dbias) over its nb rows
  auto finish = [&](const char* what, int nb) -> int {
    MIA_LAUNCH_CHECK(what);
    if (dbias) {
      cp_final2_kernel<<<(unsigned)c, 256, 0, s>>>((const float*)partial, nb, c, /*q0 = sum dx*/ dbias, nullptr);
      MIA_LAUNCH_CHECK("pool_bn_bwd_apply_final");
    }
    return 0;
  };
  if (!mapped && kw % 8 == 0 && dtype == MIA_BF16 && units < (1ll << 31) &&
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0) {
    const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(units, NT), CP_MAXBLK));
    pool_bn_bwd_apply_oct_kernel<GDT><<<nb, NT, 0, s>>>(gm, argmax, reinterpret_cast<const bf16*>(x), n, h, w, c, kh, kw,
                                                        make_fastdiv((w + 7) / 8), make_fastdiv(h), make_fastdiv(c / 8),
                                                        gamma, mean, invstd, dgamma, dbeta, reinterpret_cast<bf16*>(dx),
                                                        dbias ? (float*)partial : nullptr);
    return finish("pool_bn_bwd_apply", nb);
  }
  const int64_t runs = (int64_t)n * h * cdiv(w, kw) * (c / 8);
  static const bool per_pixel = getenv("MIA_POOL_BWD_PIXEL") != nullptr;  // A/B switch: the per-pixel form
  if (kw >= 2 && kw <= 4 && dtype == MIA_BF16 && runs < (1ll << 31) && !per_pixel &&
      ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dx)) & 15) == 0) {
    constexpr int RU = PB_RUNS;
    const int nb = pool_grid_cap((int)std::max<int64_t>(1, std::min<int64_t>(cdiv(runs, (int64_t)NT * RU), PB_NB)));
    const FastDiv dNR = make_fastdiv((int)cdiv(w, kw)), dH = make_fastdiv(h), dG = make_fastdiv(c / 8);
    float* part = dbias ? (float*)partial : nullptr;
    const bf16* xb = reinterpret_cast<const bf16*>(x);
    bf16* dxb = reinterpret_cast<bf16*>(dx);
    if (mapped) {
      MIA_CHECK_ARG(((int64_t)rm.lead + (int64_t)n * h * rm.rowpx) * c < (1ll << 40), "pool_bn_bwd_apply: row map size");
      if (kw == 2)
        pool_bn_bwd_apply_run_kernel<2, RU, GDT, true><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                         mean, invstd, dgamma, dbeta, dxb, part, rm);
      else if (kw == 3)
        pool_bn_bwd_apply_run_kernel<3, RU, GDT, true><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                         mean, invstd, dgamma, dbeta, dxb, part, rm);
      else
        pool_bn_bwd_apply_run_kernel<4, RU, GDT, true><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                         mean, invstd, dgamma, dbeta, dxb, part, rm);
      return finish("pool_bn_bwd_apply_run", nb);
    }
    if (kw == 2)
      pool_bn_bwd_apply_run_kernel<2, RU, GDT><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                 mean, invstd, dgamma, dbeta, dxb, part);
    else if (kw == 3)
      pool_bn_bwd_apply_run_kernel<3, RU, GDT><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                 mean, invstd, dgamma, dbeta, dxb, part);
    else
      pool_bn_bwd_apply_run_kernel<4, RU, GDT><<<nb, NT, 0, s>>>(gm, argmax, xb, n, h, w, c, kh, dNR, dH, dG, gamma,
                                                                 mean, invstd, dgamma, dbeta, dxb, part);
    return finish("pool_bn_bwd_apply_run", nb);
  }
  // the row map is served by the run form alone (bf16 activations, kw = 2..4, any kh, 16-byte aligned x and dx)
  MIA_CHECK_ARG(!mapped, "pool_bn_bwd_apply: a row map needs the run form (bf16, kw 2..4, 16-byte aligned x / dx)");
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(P, (int64_t)rslots * 8), CP_MAXBLK));
  pool_bn_bwd_apply_kernel<GDT><<<nb, NT, 0, s>>>(gm, argmax, x, dtype, n, h, w, c, kh, kw, make_fastdiv(w),
                                                  make_fastdiv(h), make_fastdiv(kw), make_fastdiv(kh), gamma, mean,
                                                  invstd, dgamma, dbeta, dx, dbias ? (float*)partial : nullptr);
  return finish("pool_bn_bwd_apply", nb);
}

extern "C" int mia_pool_bn_relu_bwd_apply_rows(const void* gm, int32_t gm_dtype, const uint8_t* argmax, const void* x,
                                               int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh,
                                               int32_t kw, const float* gamma, const float* mean, const float* invstd,
                                               const float* dgamma, const float* dbeta, void* dx, int32_t lead,
                                               int32_t row_pixels, void* zero_pixel, int32_t zc, float* dbias,
                                               void* partial, mia_stream_t stream) {
  MIA_CHECK_ARG(lead >= 0 && row_pixels >= w && zc >= 0 && zc % 8 == 0 && (zc == 0 || zero_pixel),
                "pool_bn_bwd_apply: bad row map (lead %d, row_pixels %d, w %d, zc %d)", lead, row_pixels, w, zc);
  MIA_CHECK_ARG(!zero_pixel || aligned16(zero_pixel), "pool_bn_bwd_apply: zero_pixel alignment");
  MIA_CHECK_ARG(gm && argmax && x && mean && invstd && dgamma && dbeta && dx, "pool_bn_bwd_apply: null pointer");
  MIA_CHECK_ARG(!dbias || partial, "pool_bn_bwd_apply: dbias needs the partial workspace");
  MIA_CHECK_ARG(c % 8 == 0 && c >= 8 && (NT % (c / 8)) == 0, "pool_bn_bwd_apply: channels");
  MIA_CHECK_ARG((int64_t)n * h * w < (1ll << 31), "pool_bn_bwd_apply: too many pixels for 32-bit indexing");
  MIA_CHECK_ARG(h >= kh && w >= kw && kh * kw <= 256, "pool_bn_bwd_apply: bad geometry");
  MIA_CHECK_ARG(gm_dtype == MIA_F32 || gm_dtype == MIA_BF16, "pool_bn_bwd_apply: gm dtype %d", gm_dtype);
  // a cell's eight channels are read as 16-B vectors (one of bf16, two of f32)
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(gm) & 15) == 0, "pool_bn_bwd_apply: gm alignment");
  hipStream_t s = as_stream(stream);
  const RowMap rm{lead, row_pixels, zc ? zero_pixel : nullptr, zc / 8};
  if (gm_dtype == MIA_BF16)
    return pool_bn_bwd_apply_launch<MIA_BF16>(gm, argmax, x, dtype, n, h, w, c, kh, kw, gamma, mean, invstd, dgamma,
                                              dbeta, dx, dbias, partial, s, rm);
  return pool_bn_bwd_apply_launch<MIA_F32>(gm, argmax, x, dtype, n, h, w, c, kh, kw, gamma, mean, invstd, dgamma, dbeta,
                                           dx, dbias, partial, s, rm);
}

extern "C" int mia_pool_bn_relu_bwd_apply_ex(const void* gm, int32_t gm_dtype, const uint8_t* argmax, const void* x,
                                             int32_t dtype, int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh,
                                             int32_t kw, const float* gamma, const float* mean, const float* invstd,
                                             const float* dgamma, const float* dbeta, void* dx, float* dbias,
                                             void* partial, mia_stream_t stream) {
  return mia_pool_bn_relu_bwd_apply_rows(gm, gm_dtype, argmax, x, dtype, n, h, w, c, kh, kw, gamma, mean, invstd, dgamma,
                                         dbeta, dx, 0, w, nullptr, 0, dbias, partial, stream);
}

extern "C" int mia_pool_bn_relu_bwd_apply(const float* gm, const uint8_t* argmax, const void* x, int32_t dtype,
                                          int32_t n, int32_t h, int32_t w, int32_t c, int32_t kh, int32_t kw,
                                          const float* gamma, const float* mean, const float* invstd,
                                          const float* dgamma, const float* dbeta, void* dx, float* dbias,
                                          void* partial, mia_stream_t stream) {
  return mia_pool_bn_relu_bwd_apply_ex(gm, MIA_F32, argmax, x, dtype, n, h, w, c, kh, kw, gamma, mean, invstd, dgamma,
                                       dbeta, dx, dbias, partial, stream);
}

extern "C" int mia_col2im_rows(const float* p, int32_t n, int32_t ph, int32_t w, int32_t kh, void* out, int32_t dtype,
                               mia_stream_t stream) {
  MIA_CHECK_ARG(p && out && n > 0 && ph > 0 && w > 0 && kh > 0, "col2im_rows: bad arguments");
  MIA_CHECK_ARG((int64_t)n * (ph + kh - 1) * w < (1ll << 31), "col2im_rows: too many elements");
  const int64_t total = (int64_t)n * (ph + kh - 1) * w;
  const int nb = (int)std::min<int64_t>(cdiv(total, 256), 16384);
  col2im_rows_kernel<<<nb, 256, 0, as_stream(stream)>>>(p, n, ph, w, kh, out, dtype);
  MIA_LAUNCH_CHECK("col2im_rows");
  return 0;
}
