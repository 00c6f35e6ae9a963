// EnvNet-v2 trunk conv4 (Conv2d(32, 32, (8, 8)), reference src/models/envnet_v2.py:34) forward and
// backward-data on bf16 MFMA, gfx950.
//
//   y[b][oy][ox][co] = sum_{ky, kx, ci} a[b][oy+ky-ph][ox+kx-pw][ci] * W[co][ky][kx][ci]
//
// forward: a = relu(bn(conv3 output)) applied while staging, ph = pw = 0, bias + BN statistics of
// the stored bf16 output in the epilogue; backward-data: a = dY, ph = pw = 7, W = the flipped OHWI
// weights of the transposed conv (mia_pack_weight layout 1).
//
// Row-rolling schedule, one wave per SIMD: a wave owns (clip, 64 output columns) items and walks the
// padded input rows top to bottom.  Input row r feeds output rows r-7 .. r (kernel rows ky = 7 .. 0),
// so the wave keeps EIGHT output rows in flight in its accumulators (8 rows x 2 pixel tiles x 16 =
// 256 registers) and every input fragment it reads from LDS serves 8 MFMAs (one per ky); after row r
// the output row r-7 is complete, is stored from the accumulators and its slot restarts at zero.
// The accumulator slot of (row r, ky) is (r - ky) mod 8: the row loop is unrolled by 8 so the slot is
// a compile-time register index.  All 64 weight fragments x 2 channel halves (128 KB) sit in LDS in
// MFMA-fragment order (lane-contiguous 16-B pieces: conflict-free), read once per (row, ky, kx, c)
// and used for both pixel tiles: 160 ds_read_b128 per 256 MFMAs, ~80 B/clk per CU at the MFMA peak.
// Each wave stages its own 71-pixel strip (row pitch 80 B: conflict-free b128 reads), so the waves
// never wait for each other; the next row's raw loads fly while the current row computes.
#include "bn_math.h"
#include "channel_partials.h"

#include <algorithm>
#include <type_traits>


namespace {

constexpr int C8_NT = 256;
constexpr int C8_PX = 64;                    // output columns per item (2 MFMA tiles)
constexpr int C8_SPX = C8_PX + 7;            // staged input columns
constexpr int C8_PSB = 80;                   // LDS bytes per staged pixel (32 ch bf16 + 16 pad)
constexpr int C8_STRIP = C8_SPX * C8_PSB;    // 5 680 B per wave
constexpr int C8_WB = 128 * 1024;            // weight fragments
constexpr int C8_LDC = (C8_SPX * 4 + 63) / 64;  // 16-B chunks per lane per staged row (5)

struct C8Args {
  const bf16* x;      // (n, h, wd, 32)
  const float* ps;    // pre-op scale / shift (32) or null
  const float* pt;
  const bf16* w;      // (32 co, 8 ky, 8 kx, 32 ci)
  const float* bias;  // (32) or null
  bf16* y;            // (n, oh, ow, 32)
  float* part;        // [waves][32][2] BN shifted sums about bias (STATS) or ReLU+BN backward sums (RED), or null
  const bf16* bx;     // RED: the BN input at the output pixels (n, oh, ow, 32)
  const float *bsc, *bsh, *bmu, *bis;  // RED: its BN scale, shift, mean, invstd (32 each)
  int n, h, wd, ph, pw, oh, ow, nchunk;
  int nfull0, nsplit;  // items < nfull0 cover all output rows; the rest are row parts (nsplit per chunk)
};

__device__ __forceinline__ u32x4 cook(u32x4 u, bool ok, const float* sc, const float* sh) {
  if (!ok) return u32x4{0u, 0u, 0u, 0u};
  if (sc == nullptr) return u;
  return bn_relu_pack(u, sc, sh);
}

#ifndef C8_EDGE
#define C8_EDGE 1
#endif
// RED (backward-data only): the epilogue also forms the ReLU+BN backward sums of the stored gradient
// dA = dX against the BN input bx of the forward (mask relu(bx*scale+shift) > 0, xhat = (bx-mean)*invstd):
// sum dA*mask and sum dA*mask*xhat per channel, as mia_bn_relu_bwd_reduce computes them from a second read
// of dA.  The bx row of output row r-7 is loaded when input row r starts, so its latency sits under the
// row's MFMAs.
template <bool PRE, bool STATS, bool RED, int JU>
__global__ __launch_bounds__(C8_NT) __attribute__((amdgpu_waves_per_eu(1, 1))) void conv8_kernel(C8Args g) {
  __shared__ __attribute__((aligned(16))) char smem[C8_WB + 4 * C8_STRIP];
  __shared__ __attribute__((aligned(16))) float prm[224];  // pre-op scale, shift, bias, RED's BN (out of VGPRs)
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t < 32) {
    prm[t] = g.ps ? g.ps[t] : 1.f;
    prm[32 + t] = g.pt ? g.pt[t] : 0.f;
    prm[64 + t] = g.bias ? g.bias[t] : 0.f;
    if constexpr (RED) {
      prm[96 + t] = g.bsc[t];
      prm[128 + t] = g.bsh[t];
      prm[160 + t] = g.bmu[t];
      prm[192 + t] = g.bis[t];
    }
  }

  // weights -> fragment order: fragment f = (ky*8 + kx)*2 + c, piece [lane] = W[lane&31][ky][kx][16c + 8(lane>>5) .. +8]
  for (int q = t; q < C8_WB / 16; q += C8_NT) {
    const int f = q >> 6, l = q & 63;
    const int kk = (f >> 1) * 32 + (f & 1) * 16 + 8 * (l >> 5);
    *reinterpret_cast<u32x4*>(smem + q * 16) = *reinterpret_cast<const u32x4*>(g.w + (l & 31) * 2048 + kk);
  }

  const int cg = lane & 3;  // channel group of every staged 16-B chunk this lane handles
  const int c0 = 8 * (lane >> 5);
  float s1[16], s2[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  __syncthreads();

  const int gw = blockIdx.x * 4 + wv, nw = gridDim.x * 4;
  const int items = g.nfull0 + (g.n * g.nchunk - g.nfull0) * g.nsplit;
  char* strip = smem + C8_WB + wv * C8_STRIP;
  const u32x4* xs = reinterpret_cast<const u32x4*>(g.x);

  f32x16 acc[8][2];
  u32x4 raw[C8_LDC];
  u32x4 bxr[2][2];  // RED: bx of the output row being retired, [pixel tile][channel half]
  uint32_t rok = 0;

  for (int item = gw; item < items; item += nw) {
    int base = item, oy_lo = 0, oy_hi = g.oh;
    if (item >= g.nfull0) {  // last round: chunks split into row parts so every wave gets one
      const int j = item - g.nfull0, part = j % g.nsplit;
      base = g.nfull0 + j / g.nsplit;
      oy_lo = part * g.oh / g.nsplit;
      oy_hi = (part + 1) * g.oh / g.nsplit;
    }
    const int b = base / g.nchunk;
    const int x0 = (base - b * g.nchunk) * C8_PX;
    const int ix0 = x0 - g.pw;
    const int r_lo = oy_lo, r_hi = oy_hi + 7;  // padded input rows of this item

    auto load_row = [&](int r) __attribute__((always_inline)) {
      const int iy = r - g.ph;
      const bool rowok = iy >= 0 && iy < g.h;
      rok = 0;
#pragma unroll
      for (int s = 0; s < C8_LDC; ++s) {
        const int p = (lane + 64 * s) >> 2;
        const int ix = ix0 + p;
        const bool ok = rowok && p < C8_SPX && ix >= 0 && ix < g.wd;
        const int64_t off = ok ? (((int64_t)b * g.h + iy) * g.wd + ix) * 4 + cg : 0;
        raw[s] = xs[off];
        rok |= (uint32_t)ok << s;
      }
    };
    auto store_row = [&]() __attribute__((always_inline)) {
      BnFwd8 pre;
      pre.load(cg, prm, prm + 32);
#pragma unroll
      for (int s = 0; s < C8_LDC; ++s) {
        const int p = (lane + 64 * s) >> 2;
        if (p < C8_SPX)
          *reinterpret_cast<u32x4*>(strip + p * C8_PSB + cg * 16) =
              cook(raw[s], (rok >> s) & 1u, PRE ? pre.sc : nullptr, pre.sh);
      }
    };
    auto load_bx = [&](int oy) __attribute__((always_inline)) {
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        const int ox = x0 + 32 * tt + (lane & 31);
        const int64_t off = ox < g.ow ? (((int64_t)b * g.oh + oy) * g.ow + ox) * 32 + c0 : 0;
#pragma unroll
        for (int h = 0; h < 2; ++h) bxr[tt][h] = *reinterpret_cast<const u32x4*>(g.bx + off + 16 * h);
      }
    };
    // output row oy from accumulator slot S: bias, bf16 store, BN statistics
    auto emit = [&](const f32x16 (&a)[2], int oy) __attribute__((always_inline)) {
      float bv[16];
#pragma unroll
      for (int i = 0; i < 8; ++i) { bv[i] = prm[64 + c0 + i]; bv[8 + i] = prm[64 + c0 + 16 + i]; }
#pragma unroll
      for (int tt = 0; tt < 2; ++tt) {
        float v[16];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a[tt][8 * h + j]),
                                                             __float_as_uint(a[tt][8 * h + 4 + j]), false, false);
            v[8 * h + j] = __builtin_bit_cast(float, (unsigned)sw[0]);
            v[8 * h + 4 + j] = __builtin_bit_cast(float, (unsigned)sw[1]);
          }
        const int ox = x0 + 32 * tt + (lane & 31);
        if (ox < g.ow) {
          bf16* dst = g.y + (((int64_t)b * g.oh + oy) * g.ow + ox) * 32 + c0;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            uint32_t w4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int e = 8 * h + 2 * i;
              w4[i] = pk_bf16(v[e] + bv[e], v[e + 1] + bv[e + 1]);
              if constexpr (STATS) {
                const float d0 = bf16_lo(w4[i]) - bv[e], d1 = bf16_hi(w4[i]) - bv[e + 1];
                s1[e] += d0; s2[e] = fmaf(d0, d0, s2[e]);
                s1[e + 1] += d1; s2[e + 1] = fmaf(d1, d1, s2[e + 1]);
              }
              if constexpr (RED) {
                const uint32_t xw = bxr[tt][h][i];
                const float xv[2] = {bf16_lo(xw), bf16_hi(xw)};
                const float dv[2] = {bf16_lo(w4[i]), bf16_hi(w4[i])};
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                  const int c = c0 + 16 * h + 2 * i + k;
                  const float gk = bn_relu_on(xv[k], prm[96 + c], prm[128 + c]) ? dv[k] : 0.f;
                  bn_red_step(gk, xv[k], prm[160 + c], prm[192 + c], s1[e + k], s2[e + k]);
                }
              }
            }
            *reinterpret_cast<u32x4*>(dst + 16 * h) = u32x4{w4[0], w4[1], w4[2], w4[3]};
          }
        }
      }
    };

#pragma unroll
    for (int sl = 0; sl < 8; ++sl)
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[sl][tt][i] = 0.f;

    // one padded input row r (r % 8 == P): stage it, start the next row's loads, 8 x 32 MFMAs,
    // then retire output row r - 7 (slot (P + 1) % 8)
    auto step = [&](auto PC, auto EC, int r) __attribute__((always_inline)) {
      constexpr int P = decltype(PC)::value;
      constexpr bool EDGE = decltype(EC)::value;  // a row whose kernel rows partly map outside [oy_lo, oy_hi)
      const int kylo = r - oy_hi + 1, kyhi = r - oy_lo;  // kernel rows with a live output row
      const int iy = r - g.ph;
      const bool live = iy >= 0 && iy < g.h;  // wave-uniform: padding rows contribute nothing
      if (live) {
        wave_sync();  // the previous row's fragment reads are done (common.h)
#ifdef C8_PROBE_NOSTAGE  // timing probe only: the strip is never restaged
        if (g.n < 0)
#endif
        store_row();
        wave_sync();
      }
      if (r + 1 < r_hi) load_row(r + 1);
      if constexpr (RED) {
        if (r - 7 >= oy_lo) load_bx(r - 7);
      }
      if (live) {
        // (kx, c) blocks of 16 MFMAs; the 10 fragments of block j+1 are read while block j computes
        // (interleaved one DS read per MFMA), so every LDS read has >= 6 MFMAs of cover
        bf16x8 fw[2][8], fb[2][2];
        auto fetch = [&](int j, int buf) __attribute__((always_inline)) {
          const int kx = j >> 1, c = j & 1;
#pragma unroll
          for (int tt = 0; tt < 2; ++tt)
            fb[buf][tt] = *reinterpret_cast<const bf16x8*>(strip + (32 * tt + (lane & 31) + kx) * C8_PSB + c * 32 +
                                                           (lane >> 5) * 16);
#pragma unroll
          for (int ky = 0; ky < 8; ++ky)
            fw[buf][ky] = *reinterpret_cast<const bf16x8*>(smem + ((ky * 8 + kx) * 2 + c) * 1024 + lane * 16);
        };
        fetch(0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll JU
        for (int j = 0; j < 16; ++j) {
          const int cur = j & 1;
          fetch((j + 1) & 15, cur ^ 1);  // (the last block re-reads block 0: harmless, keeps the body uniform)
#pragma unroll
          for (int ky = 0; ky < 8; ++ky) {
            if constexpr (EDGE) {
              if (ky < kylo || ky > kyhi) continue;  // wave-uniform: that output row is outside the item
            }
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
              acc[(P - ky + 8) & 7][tt] =
                  __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[cur][ky], fb[cur][tt], acc[(P - ky + 8) & 7][tt], 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < 10; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);
          __builtin_amdgcn_sched_barrier(0);  // keep block j+1's reads inside block j's MFMA stream
        }
      }
      constexpr int S = (P + 1) & 7;
#ifdef C8_PROBE_NOEMIT  // timing probe only (tools/probe/c8_variant.sh): the epilogue never runs
      if (g.n < 0)
#endif
      if (r - 7 >= oy_lo) emit(acc[S], r - 7);
#pragma unroll
      for (int tt = 0; tt < 2; ++tt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[S][tt][i] = 0.f;
    };

    load_row(r_lo);
    for (int r0 = r_lo & ~7; r0 < r_hi; r0 += 8) {
#if C8_EDGE
      // rows within 7 of either end of the item run only the kernel rows that land on its output rows
#define C8_STEP(k)                                                                                   \
  if (r0 + k >= r_lo && r0 + k < r_hi) {                                                             \
    if (r0 + k < oy_lo + 7 || r0 + k >= oy_hi)                                                       \
      step(std::integral_constant<int, k>{}, std::true_type{}, r0 + k);                              \
    else                                                                                             \
      step(std::integral_constant<int, k>{}, std::false_type{}, r0 + k);                             \
  }
#else
#define C8_STEP(k) if (r0 + k >= r_lo && r0 + k < r_hi) step(std::integral_constant<int, k>{}, std::false_type{}, r0 + k);
#endif
      C8_STEP(0) C8_STEP(1) C8_STEP(2) C8_STEP(3) C8_STEP(4) C8_STEP(5) C8_STEP(6) C8_STEP(7)
#undef C8_STEP
    }
  }

  if constexpr (STATS || RED) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
#pragma unroll
      for (int m = 1; m < 32; m <<= 1) {
        s1[i] += __shfl_xor(s1[i], m, 64);
        s2[i] += __shfl_xor(s2[i], m, 64);
      }
    }
    if ((lane & 31) == 0) {
      float* dst = g.part + (int64_t)gw * 64;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        dst[(c0 + i) * 2] = s1[i];
        dst[(c0 + i) * 2 + 1] = s2[i];
        dst[(c0 + 16 + i) * 2] = s1[8 + i];
        dst[(c0 + 16 + i) * 2 + 1] = s2[8 + i];
      }
    }
  }
}

}  // namespace

extern "C" int mia_trunk_conv8(const void* x, const float* pre_scale, const float* pre_shift, const void* w,
                               const float* bias, void* y, float* partial, int32_t nblocks, int32_t n, int32_t h,
                               int32_t wd, int32_t ph, int32_t pw, mia_stream_t stream) {
  MIA_CHECK_ARG(x && w && y && n > 0 && h > 0 && wd > 0 && ph >= 0 && pw >= 0 && nblocks > 0,
                "trunk_conv8: bad arguments");
  MIA_CHECK_ARG((pre_scale == nullptr) == (pre_shift == nullptr), "trunk_conv8: pre_scale/pre_shift come together");
  MIA_CHECK_ARG(partial == nullptr || bias != nullptr, "trunk_conv8: statistics are shifted about the bias");
  MIA_CHECK_ARG(aligned16(x) && aligned16(w) && aligned16(y), "trunk_conv8: x/w/y must be 16-byte aligned");
  const int oh = h + 2 * ph - 7, ow = wd + 2 * pw - 7;
  MIA_CHECK_ARG(oh > 0 && ow > 0, "trunk_conv8: output is empty");
  MIA_CHECK_ARG((int64_t)n * h * wd * 4 < (1ll << 40), "trunk_conv8: input too large");
  C8Args a{reinterpret_cast<const bf16*>(x), pre_scale, pre_shift, reinterpret_cast<const bf16*>(w), bias,
           reinterpret_cast<bf16*>(y), partial, nullptr, nullptr, nullptr, nullptr, nullptr,
           n, h, wd, ph, pw, oh, ow, (int)cdiv(ow, C8_PX), 0, 1};
  MIA_CHECK_ARG((int64_t)n * a.nchunk * 8 < (1ll << 31), "trunk_conv8: too many items");
  // balance the last round: split the chunks left over after the full rounds into row parts
  const int nw = 4 * nblocks, full = n * a.nchunk, rem = full % nw;
  a.nfull0 = full - rem;
  if (rem > 0) a.nsplit = (int)std::max(1, std::min(std::min(nw / rem, 4), oh / 8 > 0 ? oh / 8 : 1));
  hipStream_t s = as_stream(stream);
  // (kx, c) block loop unrolled by 2 only (double-buffer parity static): a 16x smaller body than the
  // full unroll, measured 3 % faster on the forward (instruction-cache pressure) and equal on dgrad
  if (pre_scale) {
    if (partial) conv8_kernel<true, true, false, 2><<<nblocks, C8_NT, 0, s>>>(a);
    else conv8_kernel<true, false, false, 2><<<nblocks, C8_NT, 0, s>>>(a);
  } else {
    if (partial) conv8_kernel<false, true, false, 2><<<nblocks, C8_NT, 0, s>>>(a);
    else conv8_kernel<false, false, false, 2><<<nblocks, C8_NT, 0, s>>>(a);
  }
  MIA_LAUNCH_CHECK("trunk_conv8");
  return 0;
}

extern "C" int mia_trunk_conv8_dgrad_bn(const void* dy, const void* w, void* dx, int32_t nblocks, int32_t n,
                                        int32_t h, int32_t wd, const void* bx, const float* scale,
                                        const float* shift, const float* mean, const float* invstd, float* dgamma,
                                        float* dbeta, float* partial, mia_stream_t stream) {
  MIA_CHECK_ARG(dy && w && dx && bx && scale && shift && mean && invstd && dgamma && dbeta && partial && n > 0 &&
                    h > 0 && wd > 0 && nblocks > 0,
                "trunk_conv8_dgrad_bn: bad arguments");
  MIA_CHECK_ARG(aligned16(dy) && aligned16(w) && aligned16(dx) && aligned16(bx),
                "trunk_conv8_dgrad_bn: dy/w/dx/bx must be 16-byte aligned");
  const int oh = h + 7, ow = wd + 7;
  MIA_CHECK_ARG((int64_t)n * oh * ow * 4 < (1ll << 40), "trunk_conv8_dgrad_bn: input too large");
  C8Args a{reinterpret_cast<const bf16*>(dy), nullptr, nullptr, reinterpret_cast<const bf16*>(w), nullptr,
           reinterpret_cast<bf16*>(dx), partial, reinterpret_cast<const bf16*>(bx), scale, shift, mean, invstd,
           n, h, wd, 7, 7, oh, ow, (int)cdiv(ow, C8_PX), 0, 1};
  MIA_CHECK_ARG((int64_t)n * a.nchunk * 8 < (1ll << 31), "trunk_conv8_dgrad_bn: too many items");
  const int nw = 4 * nblocks, full = n * a.nchunk, rem = full % nw;
  a.nfull0 = full - rem;
  if (rem > 0) a.nsplit = (int)std::max(1, std::min(std::min(nw / rem, 4), oh / 8 > 0 ? oh / 8 : 1));
  hipStream_t s = as_stream(stream);
  conv8_kernel<false, false, true, 2><<<nblocks, C8_NT, 0, s>>>(a);
  MIA_LAUNCH_CHECK("trunk_conv8_dgrad_bn");
  // per-wave partials [nw][32][2]
  cp_final2_kernel<<<32, 256, 0, s>>>(partial, nw, 32, /*q0 = sum g*/ dbeta, /*q1 = sum g xhat*/ dgamma);
  MIA_LAUNCH_CHECK("trunk_conv8_dgrad_bn final");
  return 0;
}
