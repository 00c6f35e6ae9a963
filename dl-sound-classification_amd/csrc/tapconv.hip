// The single-channel convs of EnvNet-v2 (frontend conv1: 1x64 taps, stride 2 over the waveform; trunk
// conv3: 8x8 taps over the one-channel image) as MFMA tap kernels, gfx950: forward (mia_gemm path 4),
// weight gradient (path 3), and the conv1 weight gradient fused with the BatchNorm backward reductions
// (mia_fe_conv1_wgrad_bn, which instantiates the same weight-gradient kernel).  Section comments below.
#include <cstdlib>

#include "bn_math.h"
#include "gemm_common.h"

namespace {

using namespace mgemm;

constexpr int NT = 256;

// -------------------------------------------------------------------------- single-channel tap wgrad
// dW[n][ky][kx] = sum_{b,oy,ox} dY[b,oy,ox,n] * X[b, oy+ky, S*ox+kx]  for the 1-channel convs of
// EnvNet-v2 (frontend conv1: 1x64 taps, stride 2 over the waveform; trunk conv3: 8x8 taps over the
// 64 x Wp image).  N = 32 output channels, KH*KW = 64 taps.  Per chunk of BP output pixels the
// block stages the dY tile [BP][32] (transposed MFMA reads) and, for every (ky, parity) tap
// sequence seq[i] = X[oy+ky][S*(x0+i)+par], 8 copies shifted by 0..7 elements so that the 8
// consecutive output pixels an MFMA k-group needs (X[..][S*(ox..ox+7)+kx]) are one aligned
// 16-byte LDS read whatever the tap offset.  The 4 waves split the chunk's k-steps; partials are
// summed through LDS into one f32 slab per block (ws[z][32][64]) -> splitk_reduce.
struct TapWArgs {
  const char* x;
  const char* dy;
  int n, h, wx, oh, ow;
  int Z;
  float* ws;
  // BNB (single pass, BN-backward reductions not yet known): dy is the gradient w.r.t. relu(bn(y));
  // the kernel stages dz = mask(y) * dy and y itself as two A operands and accumulates
  //   G1 = sum dz x,  G3 = sum y x   (slabs ws[z][2][32][64])
  // and per channel sum dz, sum dz*xhat, sum y (dbp[z][32][3]).  The BN-input gradient is linear,
  //   g = A dz + B + C y  (A = gamma*invstd, B = -A*dbeta/P + A*invstd*mean*dgamma/P, C = -A*invstd*dgamma/P),
  // so dW = A G1 + B G2 + C G3 with G2[k] = sum x[2p+k] (fe_conv1_lin_final).
  const bf16* by;
  const float *bsc, *bsh, *bmean, *binvstd;
  float* dbp;
  int64_t bP;
};

template <typename TD, typename TX, int S, int KH, int KW, bool BNB = false>
// (BNB: the MIA_CONV1W_V1 oracle of conv1_wgrad_bn_kernel, its BN arithmetic written out, off bn_math.h)
__global__ __launch_bounds__(NT) void tapwgrad_kernel(TapWArgs g) {
  constexpr int BP = 256;
  constexpr int NS = KW / S;                       // taps per parity sequence
  constexpr int LP = (BP + NS + 7) / 8 * 8;        // copy length
  constexpr int LR = LP + 8;                       // raw length (covers shift 7)
  constexpr int NSEQ = KH * S;
  constexpr int CPB = LP * 2;                      // bytes per shifted copy
  constexpr int SQB = 8 * CPB + 16;                // bytes per sequence (+16: parity banks)
  constexpr int DYB = BP * 64;                     // dY tile [BP][32] bf16
  constexpr int RAWB = NSEQ * LR * 2;
  constexpr int CPYB = NSEQ * SQB;
  constexpr int MAINB0 = DYB + RAWB + CPYB;
  constexpr int MAINB = MAINB0 + (BNB ? DYB : 0);
  constexpr int REDB = 4 * 32 * 64 * 4;
  constexpr int RCH = (NSEQ * LR + NT - 1) / NT;
  constexpr int DCH = BP * 32 / 8 / NT;            // 4
  static_assert(KH * KW == 64, "64 taps");
  __shared__ __attribute__((aligned(16))) char smem[MAINB > REDB ? MAINB : REDB];
  char* dyt = smem;
  bf16* raw = reinterpret_cast<bf16*>(smem + DYB);
  char* cpy = smem + DYB + RAWB;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int z = blockIdx.x;
  const int CPR = (g.ow + BP - 1) / BP;
  const int64_t nchunks = (int64_t)g.n * g.oh * CPR;
  const TD* dys = reinterpret_cast<const TD*>(g.dy);
  const TX* xs = reinterpret_cast<const TX*>(g.x);

  u32x4 dreg[DCH];
  float rreg[RCH];
  u32x4 yreg[BNB ? DCH : 1];
  uint32_t dok = 0;
  float bsc[8], bsh[8], bmu[8], bis[8], sdz[8], sdx[8], sy[8];
  if constexpr (BNB) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int ch = (t & 3) * 8 + i;
      bsc[i] = g.bsc[ch];
      bsh[i] = g.bsh[ch];
      bis[i] = g.binvstd[ch];
      bmu[i] = g.bmean[ch];
      sdz[i] = 0.f; sdx[i] = 0.f; sy[i] = 0.f;
    }
  }
  char* yt = smem + MAINB0;  // BNB: second A tile (y), [BP][32] bf16

  auto load_chunk = [&](int64_t c) __attribute__((always_inline)) {
    const int64_t row = c / CPR;
    const int x0 = (int)(c - row * CPR) * BP;
    const int b = (int)(row / g.oh), oy = (int)(row - (int64_t)b * g.oh);
    const TD* src = dys + ((int64_t)row * g.ow + x0) * 32;
    dok = 0;
#pragma unroll
    for (int s2 = 0; s2 < DCH; ++s2) {
      const int q = t + NT * s2;
      const int p = q >> 2, cc = q & 3;
      u32x4 v = {0u, 0u, 0u, 0u};
      if constexpr (BNB) {
        const bool ok = x0 + p < g.ow;
        const int64_t off = ok ? ((int64_t)row * g.ow + x0 + p) * 32 + cc * 8 : 0;
        dreg[s2] = *reinterpret_cast<const u32x4*>(reinterpret_cast<const bf16*>(g.dy) + off);
        yreg[s2] = *reinterpret_cast<const u32x4*>(g.by + off);
        dok |= (uint32_t)ok << s2;
        continue;
      }
      if (x0 + p < g.ow) {
        if constexpr (sizeof(TD) == 2) {
          v = *reinterpret_cast<const u32x4*>(src + p * 32 + cc * 8);
        } else {
          const float4 a = reinterpret_cast<const float4*>(src + p * 32 + cc * 8)[0];
          const float4 d = reinterpret_cast<const float4*>(src + p * 32 + cc * 8)[1];
          const float f[8] = {a.x, a.y, a.z, a.w, d.x, d.y, d.z, d.w};
          uint32_t w4[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            w4[i] = pk_bf16(f[2 * i], f[2 * i + 1]);
          }
          v = u32x4{w4[0], w4[1], w4[2], w4[3]};
        }
      }
      dreg[s2] = v;
    }
#pragma unroll
    for (int s2 = 0; s2 < RCH; ++s2) {
      const int e = t + NT * s2;
      float v = 0.f;
      if (e < NSEQ * LR) {
        const int seq = e / LR, i = e - seq * LR;
        const int ky = seq / S, par = seq - ky * S;
        const int iy = oy + ky;
        const int ix = S * (x0 + i) + par;
        if (iy < g.h && ix < g.wx) v = (float)xs[((int64_t)b * g.h + iy) * g.wx + ix];
      }
      rreg[s2] = v;
    }
  };
  auto store_chunk = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int s2 = 0; s2 < DCH; ++s2) {
      const int q = t + NT * s2;
      u32x4 v = dreg[s2];
      if constexpr (BNB) {
        uint32_t w4[4] = {0u, 0u, 0u, 0u}, y4[4] = {0u, 0u, 0u, 0u};
        if ((dok >> s2) & 1u) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float gv[2], yv[2];
            gv[0] = __uint_as_float(dreg[s2][i] << 16);
            gv[1] = __uint_as_float(dreg[s2][i] & 0xffff0000u);
            yv[0] = __uint_as_float(yreg[s2][i] << 16);
            yv[1] = __uint_as_float(yreg[s2][i] & 0xffff0000u);
            uint32_t m = 0;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int c = 2 * i + h;
              const bool on = fmaf(yv[h], bsc[c], bsh[c]) > 0.f;
              const float d = on ? gv[h] : 0.f;
              sdz[c] += d;
              sdx[c] = fmaf(d, (yv[h] - bmu[c]) * bis[c], sdx[c]);
              sy[c] += yv[h];
              m |= on ? (0xffffu << (16 * h)) : 0u;
            }
            w4[i] = dreg[s2][i] & m;  // dz = mask * dy exactly (bf16 bits kept or zeroed)
            y4[i] = yreg[s2][i];
          }
        }
        v = u32x4{w4[0], w4[1], w4[2], w4[3]};
        *reinterpret_cast<u32x4*>(yt + (q >> 2) * 64 + (q & 3) * 16) = u32x4{y4[0], y4[1], y4[2], y4[3]};
      }
      *reinterpret_cast<u32x4*>(dyt + (q >> 2) * 64 + (q & 3) * 16) = v;
    }
#pragma unroll
    for (int s2 = 0; s2 < RCH; ++s2) {
      const int e = t + NT * s2;
      if (e < NSEQ * LR) raw[e] = (bf16)rreg[s2];
    }
  };
  auto build_copies = [&]() __attribute__((always_inline)) {
    constexpr int PIECES = NSEQ * 8 * (LP / 8);
    for (int pc = t; pc < PIECES; pc += NT) {
      const int seq = pc / (8 * (LP / 8));
      const int rem = pc - seq * 8 * (LP / 8);
      const int sh = rem / (LP / 8), blk = rem - sh * (LP / 8);
      const unsigned short* r = reinterpret_cast<const unsigned short*>(raw) + seq * LR + blk * 8 + sh;
      uint32_t w4[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) w4[i] = (uint32_t)r[2 * i] | ((uint32_t)r[2 * i + 1] << 16);
      *reinterpret_cast<u32x4*>(cpy + seq * SQB + sh * CPB + blk * 16) = u32x4{w4[0], w4[1], w4[2], w4[3]};
    }
  };

  f32x16 acc[2], acc3[BNB ? 2 : 1];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  if constexpr (BNB) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc3[j][r] = 0.f;
  }

  const int i16 = lane & 15, gq = lane >> 4, g2 = lane >> 5;
  // this lane's tap per n-tile: n = nt*32 + (lane&31) -> (ky, kx) -> (seq, j)
  int bseq[2], bj[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = nt * 32 + (lane & 31);
    const int ky = n / KW, kx = n - ky * KW;
    bseq[nt] = ky * S + kx % S;
    bj[nt] = kx / S;
  }

  int64_t c = z;
  if (c < nchunks) {
    load_chunk(c);
    store_chunk();
  }
  __syncthreads();
  if (c < nchunks) build_copies();
  __syncthreads();
  for (; c < nchunks; c += g.Z) {
    const int64_t cn = c + g.Z;
    const bool more = cn < nchunks;
    if (more) load_chunk(cn);
#pragma unroll
    for (int kk = 0; kk < BP / 16 / 4; ++kk) {
      const int ks = wave + 4 * kk;
      const int kr = ks * 16 + 8 * (gq >> 1) + (i16 >> 2);
      const int col = 16 * (gq & 1) + 4 * (i16 & 3);
      const char* p0 = dyt + kr * 64 + col * 2;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0 + 4 * 64));
      typedef short s16x8 __attribute__((ext_vector_type(8)));
      const s16x8 cc = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      const bf16x8 fa = __builtin_bit_cast(bf16x8, cc);
      bf16x8 fy;
      if constexpr (BNB) {
        const char* py = yt + kr * 64 + col * 2;
        const s16x4 ylo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(py));
        const s16x4 yhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(py + 4 * 64));
        const s16x8 yc = {ylo[0], ylo[1], ylo[2], ylo[3], yhi[0], yhi[1], yhi[2], yhi[3]};
        fy = __builtin_bit_cast(bf16x8, yc);
      }
      const int ox0 = ks * 16 + 8 * g2;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int q = ox0 + bj[nt];
        const int sh = q & 7;
        const bf16x8 fb = *reinterpret_cast<const bf16x8*>(cpy + bseq[nt] * SQB + sh * CPB + (q - sh) * 2);
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[nt], 0, 0, 0);
        if constexpr (BNB) acc3[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fy, fb, acc3[nt], 0, 0, 0);
      }
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
      build_copies();
      __syncthreads();
    }
  }

  // sum the 4 waves' partials, write the block's slab ws[z][32][64] (BNB: ws[z][2][32][64], G1 then G3)
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int which = 0; which < (BNB ? 2 : 1); ++which) {
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * g2;
        float v = acc[nt][r];
        if constexpr (BNB) if (which) v = acc3[nt][r];
        red[(wave * 32 + m) * 64 + nt * 32 + (lane & 31)] = v;
      }
    __syncthreads();
    float* dst = g.ws + ((int64_t)z * (BNB ? 2 : 1) + which) * 32 * 64;
    for (int e = t; e < 32 * 64; e += NT)
      dst[e] = red[e] + red[2048 + e] + red[4096 + e] + red[6144 + e];
  }
  if constexpr (BNB) {
    // per-channel sums of this block: channel c = (t&3)*8 + i summed over the 64 threads of its
    // group in thread order (deterministic) -> dbp[z][c][0..2] = (sum dz, sum dz*xhat, sum y)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      red[t * 8 + i] = sdz[i];
      red[2048 + t * 8 + i] = sdx[i];
      red[4096 + t * 8 + i] = sy[i];
    }
    __syncthreads();
    if (t < 96) {
      const int q = t / 32, ch = t % 32, cg = ch >> 3, i = ch & 7;
      float a = 0.f;
      for (int k = 0; k < NT / 4; ++k) a += red[q * 2048 + (k * 4 + cg) * 8 + i];
      g.dbp[((int64_t)z * 32 + ch) * 3 + q] = a;
    }
  }
}

template <typename TD, typename TX, int S, int KH, int KW, bool BNB = false>
hipError_t tapwgrad_launch(const TapWArgs& r, hipStream_t s) {
  tapwgrad_kernel<TD, TX, S, KH, KW, BNB><<<(unsigned)r.Z, NT, 0, s>>>(r);
  return hipGetLastError();
}

// -------------------------------------------------------------------------- conv1 wgrad + BN1 backward, wave-private
// tapwgrad_kernel<bf16, float, 2, 1, 64, true> on another schedule (the default of mia_fe_conv1_wgrad_bn; that
// kernel is the MIA_CONV1W_V1=1 form).  There, between the cook's wait on a chunk's loads and the next
// iteration's load_chunk the block has nothing in flight, three block barriers a chunk, and the eight shifted
// copies of each parity sequence are built with 2-byte LDS reads.  The pixel ownership is already wave-private
// (thread t cooks pixels (t >> 2) + 64 s2 = k-steps wave + 4 s2, the ones its own wave feeds to the MFMA), so here
// each wave stages and consumes only its own four k-steps (wave_sync, no block barrier in the loop), two chunks
// wait in registers (chunk k + 2's loads are issued before chunk k + 1 is cooked), and x goes from the load
// registers straight to the copies: a k-step reads 96 samples x[2 P0 ..], lane m holds samples 4m .. 4m + 3 as
// the packed pairs E_m = (x[4m], x[4m+2]) and O_m = (x[4m+1], x[4m+3]) (entries 2m, 2m + 1 of the two parity
// sequences); copy sh of a sequence (entry i = seq[i + sh], sh = 0 .. 3: a fragment's 8 entries at any offset are
// two aligned 8-byte reads) takes E_m as dword m (sh 0) / m - 1 (sh 2) and (hi E_m, lo E_{m+1}) as dword m (sh 1)
// / m - 1 (sh 3).  The 8 copies of a k-step lie 96 B apart: the 32 lanes of a half wave (16 tap offsets x 2
// parities) read 32 different 8-byte pieces that cover the 64 banks once.
// Same arithmetic: block z takes chunks z, z + Z, ... in order, wave w the k-steps w, w + 4, w + 8, w + 12 of each
// into the same four accumulators with the same operand bits (dz = mask & dy, y, bf16(x)); the thread that owns
// (p mod 64, channel chunk) adds its sdz / sdx / sy terms in increasing pixel order; the folds at the end are
// tapwgrad_kernel's.
struct C1WRaw {
  u32x4 d[4], y[4];
  float xa[4], xb[4];
};

__global__ __launch_bounds__(NT, 2) void conv1_wgrad_bn_kernel(TapWArgs g) {
  constexpr int BP = 256;
  constexpr int KSB = 1024;            // one k-step's dz (or y) tile: [16 px][32 ch] bf16
  constexpr int XCB = 96, XKB = 8 * XCB;  // one copy (48 entries), one k-step's 8 copies
  constexpr int WVB = 8 * KSB + 4 * XKB;  // per wave: dz, y (4 k-steps each), x copies
  constexpr int REDB = 4 * 32 * 64 * 4;
  __shared__ __attribute__((aligned(16))) char smem[4 * WVB > REDB ? 4 * WVB : REDB];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int z = blockIdx.x;
  char* wdz = smem + wave * WVB;
  char* wy = wdz + 4 * KSB;
  char* wx = wdz + 8 * KSB;
  const int CPR = (g.ow + BP - 1) / BP;
  const int64_t nchunks = (int64_t)g.n * CPR;  // oh == 1: a row is a clip
  const bf16* dys = reinterpret_cast<const bf16*>(g.dy);
  const float* xs = reinterpret_cast<const float*>(g.x);

  float bsc[8], bsh[8], bmu[8], bis[8], sdz[8], sdx[8], sy[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int ch = (t & 3) * 8 + i;
    bsc[i] = g.bsc[ch];
    bsh[i] = g.bsh[ch];
    bis[i] = g.binvstd[ch];
    bmu[i] = g.bmean[ch];
    sdz[i] = 0.f; sdx[i] = 0.f; sy[i] = 0.f;
  }

  // x lanes: slot a = (k-step lane >> 4, m = lane & 15), slot b = (k-step (lane >> 3) & 3, m = 16 + (lane & 7));
  // lanes 32 .. 63 repeat slot b's loads and do not write them
  const int ksa = lane >> 4, ma = lane & 15, ksb = (lane >> 3) & 3, mb = 16 + (lane & 7);
  // every load is issued by every lane from a clamped address (chunks past the end repeat the last one) and
  // masked when cooked: no branch around a load, so the waits on the two register sets stay counted
  auto load = [&](int64_t c) __attribute__((always_inline)) {
    C1WRaw R;
    c = c < nchunks ? c : nchunks - 1;
    const int64_t b = c / CPR;
    const int x0 = (int)(c - b * CPR) * BP;
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      const int p = 16 * wave + 64 * s2 + (lane >> 2), cc = lane & 3;
      const bool ok = x0 + p < g.ow;
      const int64_t off = ok ? (b * g.ow + x0 + p) * 32 + cc * 8 : 0;
      R.d[s2] = *reinterpret_cast<const u32x4*>(dys + off);
      R.y[s2] = *reinterpret_cast<const u32x4*>(g.by + off);
    }
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const float* xb = xs + b * g.wx;
    const int sa = 2 * (x0 + 16 * (wave + 4 * ksa)) + 4 * ma, sb = 2 * (x0 + 16 * (wave + 4 * ksb)) + 4 * mb;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // sample pairs (s, s + 1), s even: inside the clip or outside it (wx is even)
      const f32x2 va = *reinterpret_cast<const f32x2*>(xb + min(sa + 2 * h, g.wx - 2));
      const f32x2 vb = *reinterpret_cast<const f32x2*>(xb + min(sb + 2 * h, g.wx - 2));
      R.xa[2 * h] = va[0]; R.xa[2 * h + 1] = va[1];
      R.xb[2 * h] = vb[0]; R.xb[2 * h + 1] = vb[1];
    }
    return R;
  };
  // one slot's 4 samples -> the 8 copies of its k-step; nxt* = E / O of entry pair m + 1
  auto put_x = [&](int ks, int m, uint32_t e, uint32_t o, uint32_t nxte, uint32_t nxto) __attribute__((always_inline)) {
    uint32_t* cp = reinterpret_cast<uint32_t*>(wx + ks * XKB);
    const uint32_t v[2] = {e, o}, s1[2] = {(e >> 16) | (nxte << 16), (o >> 16) | (nxto << 16)};
#pragma unroll
    for (int par = 0; par < 2; ++par) {
      uint32_t* c0 = cp + par * 4 * (XCB / 4);
      c0[m] = v[par];
      if (m >= 1) c0[2 * (XCB / 4) + m - 1] = v[par];
      if (m <= 22) c0[(XCB / 4) + m] = s1[par];
      if (m >= 1 && m <= 22) c0[3 * (XCB / 4) + m - 1] = s1[par];
    }
  };
  auto cook = [&](const C1WRaw& R, int64_t c) __attribute__((always_inline)) {
    const int64_t b = c / CPR;
    const int x0 = (int)(c - b * CPR) * BP;
    wave_sync();  // the previous chunk's fragment reads are done (common.h)
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2) {
      uint32_t w4[4] = {0u, 0u, 0u, 0u}, y4[4] = {0u, 0u, 0u, 0u};
      if (x0 + 16 * wave + 64 * s2 + (lane >> 2) < g.ow) {  // the pixel exists (else zeros, and no sums)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float gv[2], yv[2];
          gv[0] = bf16_lo(R.d[s2][i]);
          gv[1] = bf16_hi(R.d[s2][i]);
          yv[0] = bf16_lo(R.y[s2][i]);
          yv[1] = bf16_hi(R.y[s2][i]);
          uint32_t m = 0;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ch = 2 * i + h;
            const bool on = bn_relu_on(yv[h], bsc[ch], bsh[ch]);
            const float d = on ? gv[h] : 0.f;
            bn_red_step(d, yv[h], bmu[ch], bis[ch], sdz[ch], sdx[ch]);
            sy[ch] += yv[h];
            m |= on ? (0xffffu << (16 * h)) : 0u;
          }
          w4[i] = R.d[s2][i] & m;  // dz = mask * dy exactly (bf16 bits kept or zeroed)
          y4[i] = R.y[s2][i];
        }
      }
      const int o = s2 * KSB + (lane >> 2) * 64 + (lane & 3) * 16;
      *reinterpret_cast<u32x4*>(wy + o) = u32x4{y4[0], y4[1], y4[2], y4[3]};
      *reinterpret_cast<u32x4*>(wdz + o) = u32x4{w4[0], w4[1], w4[2], w4[3]};
    }
    // x: zero past the clip's end (tapwgrad_kernel's rule: ix < wx), rounded to bf16 as its (bf16) cast
    const int sa = 2 * (x0 + 16 * (wave + 4 * ksa)) + 4 * ma, sb = 2 * (x0 + 16 * (wave + 4 * ksb)) + 4 * mb;
    float xa[4], xb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xa[i] = sa + (i & 2) < g.wx ? R.xa[i] : 0.f;
      xb[i] = sb + (i & 2) < g.wx ? R.xb[i] : 0.f;
    }
    const uint32_t ea = pk_bf16(xa[0], xa[2]), oa = pk_bf16(xa[1], xa[3]);
    const uint32_t eb = pk_bf16(xb[0], xb[2]), ob = pk_bf16(xb[1], xb[3]);
    // entry pair m + 1: the next lane's, or for m = 15 slot b's first lane of the same k-step
    // (every lane takes part in every exchange; the choice is made afterwards)
    const uint32_t nea = __shfl(ea, lane + 1, 64), nea15 = __shfl(eb, 8 * ksa, 64);
    const uint32_t noa = __shfl(oa, lane + 1, 64), noa15 = __shfl(ob, 8 * ksa, 64);
    const uint32_t neb = __shfl(eb, lane + 1, 64), nob = __shfl(ob, lane + 1, 64);
    put_x(ksa, ma, ea, oa, ma < 15 ? nea : nea15, ma < 15 ? noa : noa15);
    if (lane < 32) put_x(ksb, mb, eb, ob, neb, nob);
    wave_sync();
  };

  f32x16 acc[2], acc3[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[j][r] = 0.f; acc3[j][r] = 0.f; }
  const int i16 = lane & 15, gq = lane >> 4, g2 = lane >> 5;
  // this lane's tap per n-tile: kx = nt*32 + (lane & 31) -> parity sequence kx & 1, offset kx >> 1; its 8 entries
  // start at e = 8 g2 + (kx >> 1): copy e & 3, entry e - (e & 3)
  int xo[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int kx = nt * 32 + (lane & 31), e = 8 * g2 + (kx >> 1);
    xo[nt] = ((kx & 1) * 4 + (e & 3)) * XCB + (e - (e & 3)) * 2;
  }
  const int ao = (8 * (gq >> 1) + (i16 >> 2)) * 64 + (16 * (gq & 1) + 4 * (i16 & 3)) * 2;
  auto mma = [&]() __attribute__((always_inline)) {
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {  // k-step wave + 4 kk of the chunk
      const char* p0 = wdz + kk * KSB + ao;
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0 + 4 * 64));
      const s16x8 cc = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      const bf16x8 fa = __builtin_bit_cast(bf16x8, cc);
      const char* py = wy + kk * KSB + ao;
      const s16x4 ylo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(py));
      const s16x4 yhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(py + 4 * 64));
      const s16x8 yc = {ylo[0], ylo[1], ylo[2], ylo[3], yhi[0], yhi[1], yhi[2], yhi[3]};
      const bf16x8 fy = __builtin_bit_cast(bf16x8, yc);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const char* src = wx + kk * XKB + xo[nt];
        const u32x2 q0 = *reinterpret_cast<const u32x2*>(src);
        const u32x2 q1 = *reinterpret_cast<const u32x2*>(src + 8);
        const bf16x8 fb = __builtin_bit_cast(bf16x8, u32x4{q0[0], q0[1], q1[0], q1[1]});
        acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[nt], 0, 0, 0);
        acc3[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fy, fb, acc3[nt], 0, 0, 0);
      }
    }
  };

  // two chunks wait in registers; whole pairs first with no exit inside a pair (an exit there joins the loop
  // header in the compiler's flow graph and turns the counted waits into vmcnt(0)), then the odd chunk
  int64_t c = z;
  if (c < nchunks) {
    C1WRaw ra = load(c), rb = load(c + g.Z);
    for (; c + g.Z < nchunks; c += 2 * (int64_t)g.Z) {
      cook(ra, c);
      ra = load(c + 2 * (int64_t)g.Z);
      mma();
      cook(rb, c + g.Z);
      rb = load(c + 3 * (int64_t)g.Z);
      mma();
    }
    if (c < nchunks) {
      cook(ra, c);
      mma();
    }
  }

  // the folds of tapwgrad_kernel<.., BNB = true>: the 4 waves' partials -> ws[z][2][32][64] (G1 then G3), the
  // threads' channel sums in thread order -> dbp[z][32][3]
  float* red = reinterpret_cast<float*>(smem);
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * g2;
        red[(wave * 32 + m) * 64 + nt * 32 + (lane & 31)] = which ? acc3[nt][r] : acc[nt][r];
      }
    __syncthreads();
    float* dst = g.ws + ((int64_t)z * 2 + which) * 32 * 64;
    for (int e = t; e < 32 * 64; e += NT)
      dst[e] = red[e] + red[2048 + e] + red[4096 + e] + red[6144 + e];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    red[t * 8 + i] = sdz[i];
    red[2048 + t * 8 + i] = sdx[i];
    red[4096 + t * 8 + i] = sy[i];
  }
  __syncthreads();
  if (t < 96) {
    const int q = t / 32, ch = t % 32, cg = ch >> 3, i = ch & 7;
    float a = 0.f;
    for (int k = 0; k < NT / 4; ++k) a += red[q * 2048 + (k * 4 + cg) * 8 + i];
    g.dbp[((int64_t)z * 32 + ch) * 3 + q] = a;
  }
}

// A/B switch, read at call time: MIA_CONV1W_V1=1 selects tapwgrad_kernel<bf16, float, 2, 1, 64, true>
bool conv1w_v1() { const char* e = getenv("MIA_CONV1W_V1"); return e && e[0] == '1'; }

// -------------------------------------------------------------------------- single-channel tap conv (fwd)
// y[b,oy,ox,n] = sum_{ky,kx} W[n][ky][kx] * X[b, oy+ky, S*ox+kx]  (+ epilogue) for conv1 (1x64,
// stride 2 over the f32 waveform) and conv3 (8x8 over the 1-channel trunk image): K = 64 taps,
// N = 32.  A block owns BP output pixels of one row; it stages the KH input row segments it reads
// and 8 copies of each shifted by 0..7 samples, so that every MFMA A fragment (8 consecutive taps
// = 8 consecutive samples at any offset) is one aligned ds_read_b128.  Weight fragments are read
// once per wave straight from global memory (4 KB, L2-resident).  Output is HBM-write-bound.
struct TapArgs {
  const char* x;
  int n, h, wx, oh, ow;
  const bf16* wt;
  EpiDev e;
};

template <typename TX, int S, int KH, int KW>
__global__ __launch_bounds__(NT) void tapconv_kernel(TapArgs g) {
  constexpr int BP = 256;
  constexpr int RAWL = S * (BP - 1) + KW;
  constexpr int LP = (RAWL + 7) / 8 * 8;     // copy length
  constexpr int LR = LP + 8;                 // raw length
  constexpr int CPB = LP * 2 + 16;           // bytes per copy (8-dword bank offset per copy)
  constexpr int RAWB = KH * LR * 2;
  constexpr int CPYB = KH * 8 * CPB;
  constexpr int MAINB = RAWB + CPYB;
  constexpr int STB = 4 * 32 * 33 * 4;
  static_assert(KH * KW == 64, "64 taps");
  __shared__ __attribute__((aligned(16))) char smem[MAINB > STB ? MAINB : STB];
  bf16* raw = reinterpret_cast<bf16*>(smem);
  char* cpy = smem + RAWB;

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, g2 = lane >> 5;
  const int CPR = (g.ow + BP - 1) / BP;
  const int64_t row = blockIdx.x / CPR;
  const int x0 = (int)(blockIdx.x - row * CPR) * BP;
  const int b = (int)(row / g.oh), oy = (int)(row - (int64_t)b * g.oh);
  const TX* xs = reinterpret_cast<const TX*>(g.x);

  for (int e = t; e < KH * LR; e += NT) {
    const int ky = e / LR, i = e - ky * LR;
    const int iy = oy + ky, ix = S * x0 + i;
    float v = 0.f;
    if (i < RAWL && iy < g.h && ix < g.wx) v = (float)xs[((int64_t)b * g.h + iy) * g.wx + ix];
    raw[e] = (bf16)v;
  }
  // weight fragments: k-step ks covers taps ks*16 .. +15, lane holds 8 of them for column lane&31
  bf16x8 fb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    fb[ks] = *reinterpret_cast<const bf16x8*>(g.wt + (lane & 31) * 64 + ks * 16 + 8 * g2);
  __syncthreads();
  for (int pc = t; pc < KH * 8 * (LP / 8); pc += NT) {
    const int ky = pc / (8 * (LP / 8));
    const int rem = pc - ky * 8 * (LP / 8);
    const int sh = rem / (LP / 8), blk = rem - sh * (LP / 8);
    const unsigned short* r = reinterpret_cast<const unsigned short*>(raw) + ky * LR + blk * 8 + sh;
    uint32_t w4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w4[i] = (uint32_t)r[2 * i] | ((uint32_t)r[2 * i + 1] << 16);
    *reinterpret_cast<u32x4*>(cpy + (ky * 8 + sh) * CPB + blk * 16) = u32x4{w4[0], w4[1], w4[2], w4[3]};
  }
  __syncthreads();

  f32x16 acc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int rel = wave * 64 + i * 32 + (lane & 31);   // pixel within the chunk
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k0 = ks * 16 + 8 * g2;
      const int ky = k0 / KW, kx0 = k0 - ky * KW;
      const int q = S * rel + kx0;
      const int sh = q & 7;
      const bf16x8 fa = *reinterpret_cast<const bf16x8*>(cpy + (ky * 8 + sh) * CPB + (q - sh) * 2);
      acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[ks], acc[i], 0, 0, 0);
    }
  }
  __syncthreads();
  float* stage = reinterpret_cast<float*>(smem) + wave * (32 * 33);
  const int64_t mrow0 = row * g.ow;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      stage[((r & 3) + 8 * (r >> 2) + 4 * g2) * 33 + (lane & 31)] = acc[i][r];
    __syncthreads();
    const int prow = lane >> 1, c0 = (lane & 1) * 16;
    const int ox = x0 + wave * 64 + i * 32 + prow;
    if (ox < g.ow) {
      float v[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) v[c] = stage[prow * 33 + c0 + c];
      epi_store16(g.e, mrow0 + ox, c0, 32, v);
    }
    __syncthreads();
  }
}

}  // namespace

namespace mgemm {

// 1-channel conv wgrad (path 3): A = dY [P][32] as RC, B = CONVROW/RC with c == 1 (any stride
// (1,1), kh*kw == 64) or the c == 2 stride-1 pair view of a stride-2 1-D conv (kw*2 == 64).
bool tapwgrad_ok(const MiaOperand& A, const MiaOperand& B, int64_t M, int64_t N, int64_t K, int compute, int split) {
  if (compute != MIA_BF16 || split < 2 || M != 32 || N != 64) return false;
  if (A.kind != MIA_OP_DENSE || A.layout != MIA_LAYOUT_RC || A.pre != MIA_PRE_NONE) return false;
  if (A.dtype != MIA_BF16 && A.dtype != MIA_F32) return false;
  if (A.rows != K || A.cols != 32 || A.ld != 32) return false;
  if (B.kind != MIA_OP_CONVROW || B.layout != MIA_LAYOUT_RC || B.pre != MIA_PRE_NONE) return false;
  if (B.dtype != MIA_BF16 && B.dtype != MIA_F32) return false;
  if (B.sh != 1 || B.sw != 1 || B.ph != 0 || B.pw != 0) return false;
  if (K != (int64_t)B.n * B.oh * B.ow) return false;
  const bool conv1 = B.c == 2 && B.kh == 1 && B.kw == 32 && B.h == 1;
  const bool conv3 = B.c == 1 && B.kh == 8 && B.kw == 8;
  if (!conv1 && !conv3) return false;
  if (conv1 && B.dtype != MIA_F32) return false;
  if ((reinterpret_cast<uintptr_t>(A.ptr) & 15)) return false;
  return true;
}

bool tapconv_ok(const MiaOperand& A, const MiaOperand& B, int64_t M, int64_t N, int64_t K, int compute, int split) {
  if (compute != MIA_BF16 || split > 1 || N != 32 || K != 64) return false;
  if (A.kind != MIA_OP_CONVROW || A.layout != MIA_LAYOUT_KC || A.pre != MIA_PRE_NONE) return false;
  if (A.dtype != MIA_BF16 && A.dtype != MIA_F32) return false;
  if (A.sh != 1 || A.sw != 1 || A.ph != 0 || A.pw != 0) return false;
  const bool conv1 = A.c == 2 && A.kh == 1 && A.kw == 32 && A.h == 1 && A.dtype == MIA_F32;
  const bool conv3 = A.c == 1 && A.kh == 8 && A.kw == 8;
  if (!conv1 && !conv3) return false;
  if (M != (int64_t)A.n * A.oh * A.ow) return false;
  if (B.kind != MIA_OP_DENSE || B.layout != MIA_LAYOUT_KC || B.dtype != MIA_BF16) return false;
  if (B.rows != 32 || B.cols != 64 || B.ld != 64 || (reinterpret_cast<uintptr_t>(B.ptr) & 15)) return false;
  return true;
}

int tapconv_run(const MiaOperand& A, const MiaOperand& B, const MiaEpilogue& E, hipStream_t s) {
  TapArgs r;
  r.x = reinterpret_cast<const char*>(A.ptr);
  r.n = A.n; r.h = A.h; r.wx = A.w * A.c; r.oh = A.oh; r.ow = A.ow;
  r.wt = reinterpret_cast<const bf16*>(B.ptr);
  r.e = to_dev(E);
  const int64_t blocks = (int64_t)A.n * A.oh * cdiv(A.ow, 256);
  MIA_CHECK_ARG(blocks < (1ll << 31), "tapconv: too many chunks");
  if (A.c == 2) tapconv_kernel<float, 2, 1, 64><<<(unsigned)blocks, NT, 0, s>>>(r);
  else if (A.dtype == MIA_BF16) tapconv_kernel<bf16, 1, 8, 8><<<(unsigned)blocks, NT, 0, s>>>(r);
  else tapconv_kernel<float, 1, 8, 8><<<(unsigned)blocks, NT, 0, s>>>(r);
  MIA_LAUNCH_CHECK("tapconv");
  return 0;
}

int tapwgrad_run(const MiaOperand& A, const MiaOperand& B, const MiaEpilogue& E, int64_t M, int64_t N, int split,
                 void* workspace, hipStream_t s) {
  TapWArgs r{};
  r.x = reinterpret_cast<const char*>(B.ptr);
  r.dy = reinterpret_cast<const char*>(A.ptr);
  r.n = B.n; r.h = B.h; r.wx = B.w * B.c; r.oh = B.oh; r.ow = B.ow;
  r.Z = split; r.ws = reinterpret_cast<float*>(workspace);
  hipError_t err;
  if (B.c == 2) {  // frontend conv1: stride 2 over the waveform
    err = A.dtype == MIA_BF16 ? tapwgrad_launch<bf16, float, 2, 1, 64>(r, s)
                              : tapwgrad_launch<float, float, 2, 1, 64>(r, s);
  } else if (B.dtype == MIA_BF16) {
    err = A.dtype == MIA_BF16 ? tapwgrad_launch<bf16, bf16, 1, 8, 8>(r, s)
                              : tapwgrad_launch<float, bf16, 1, 8, 8>(r, s);
  } else {
    err = A.dtype == MIA_BF16 ? tapwgrad_launch<bf16, float, 1, 8, 8>(r, s)
                              : tapwgrad_launch<float, float, 1, 8, 8>(r, s);
  }
  if (err != hipSuccess) return mia::fail(-(int)err, "tapwgrad launch: %s", hipGetErrorString(err));
  launch_splitk_reduce(r.ws, split, M, N, to_dev(E), s);
  MIA_LAUNCH_CHECK("splitk_reduce");
  return 0;
}

}  // namespace mgemm

// G2[k] = sum_{b, p < w1} x[b][2p + k] (k < 64).  With r = k & 1, j0 = k >> 1 the window is
// x_r[j0 .. j0+w1) of the parity sequence x_r[j] = x[2j+r], so G2 = sum_b T_r - (head j < j0) -
// (tail j >= j0 + w1): C1_SPLIT blocks per clip sum disjoint ranges of the two parities (coalesced
// 8-byte loads), the first block of each clip also writes the per-k head/tail corrections.
constexpr int C1_SPLIT = 8;
__global__ __launch_bounds__(256) void conv1_colsum_kernel(const float* __restrict__ x, int t, int w1,
                                                           float* __restrict__ part) {
  const int b = blockIdx.x / C1_SPLIT, sp = blockIdx.x % C1_SPLIT, tid = threadIdx.x;
  const float* xb = x + (int64_t)b * t;
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const int L = t / 2, per = (L + C1_SPLIT - 1) / C1_SPLIT;
  const int j1 = min(L, (sp + 1) * per);
  float e = 0.f, o = 0.f;
  for (int j = sp * per + tid; j < j1; j += 256) {
    const f32x2 v = *reinterpret_cast<const f32x2*>(xb + 2 * j);
    e += v[0];
    o += v[1];
  }
  __shared__ float red[2][256];
  red[0][tid] = e;
  red[1][tid] = o;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) { red[0][tid] += red[0][tid + h]; red[1][tid] += red[1][tid + h]; }
    __syncthreads();
  }
  // part[b][sp][0..1] = parity totals of this range; part[b][C1_SPLIT][k] = -(head + tail) of k
  float* pb = part + (int64_t)b * (C1_SPLIT * 2 + 64);
  if (tid < 2) pb[sp * 2 + tid] = red[tid][0];
  if (sp == 0 && tid < 64) {
    const int r = tid & 1, j0 = tid >> 1;
    float a = 0.f;
    for (int j = 0; j < j0; ++j) a -= xb[2 * j + r];
    for (int j = j0 + w1; j < L; ++j) a -= xb[2 * j + r];
    pb[C1_SPLIT * 2 + tid] = a;
  }
}

// per-channel sums over the Z block partials (dbp) and per-k G2 over the clips, in double with a
// block-wide tree (one block per output quantity: 96 channel sums + 64 G2 entries)
__global__ __launch_bounds__(256) void conv1_lin_sums_kernel(const float* __restrict__ dbp, int Z,
                                                             const float* __restrict__ g2part, int n,
                                                             double* __restrict__ out) {
  const int q = blockIdx.x, tid = threadIdx.x;
  double a = 0.0;
  if (q < 96) {
    const int ch = q % 32, which = q / 32;
    for (int z = tid; z < Z; z += 256) a += (double)dbp[((int64_t)z * 32 + ch) * 3 + which];
  } else {
    const int k = q - 96, r = k & 1;
    constexpr int PS = C1_SPLIT * 2 + 64;
    for (int b = tid; b < n; b += 256) {
      const float* pb = g2part + (int64_t)b * PS;
      double s = pb[C1_SPLIT * 2 + k];
      for (int sp = 0; sp < C1_SPLIT; ++sp) s += (double)pb[sp * 2 + r];
      a += s;
    }
  }
  __shared__ double red[256];
  red[tid] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) out[q] = red[0];
}

// dgamma/dbeta, A/B/C per channel (double), dW = A G1 + B G2 + C G3, dbias = A sum dz + B P + C sum y
__global__ __launch_bounds__(256) void conv1_lin_final_kernel(const float* __restrict__ g13, const double* __restrict__ sums,
                                                              int64_t P, const float* gamma, const float* mean,
                                                              const float* invstd, float* dgamma, float* dbeta,
                                                              float* dw, float* dbias) {
  __shared__ double cA[32], cB[32], cC[32];
  const int t = threadIdx.x;
  if (t < 32) {
    const double sdz = sums[t], sdx = sums[32 + t], sy = sums[64 + t];
    dbeta[t] = (float)sdz;
    dgamma[t] = (float)sdx;
    const double is = invstd[t], A = (gamma ? (double)gamma[t] : 1.0) * is;
    const double mb = sdz / (double)P, mg = sdx / (double)P;
    const double B = -A * mb + A * is * mg * (double)mean[t], C = -A * is * mg;
    dbias[t] = (float)(A * sdz + B * (double)P + C * sy);
    cA[t] = A; cB[t] = B; cC[t] = C;
  }
  __syncthreads();
  for (int e = t; e < 32 * 64; e += 256) {
    const int ch = e / 64, k = e % 64;
    dw[e] = (float)(cA[ch] * (double)g13[e] + cB[ch] * sums[96 + k] + cC[ch] * (double)g13[2048 + e]);
  }
}

extern "C" int mia_fe_conv1_wgrad_bn(const float* x, const void* dact, const void* y1, int32_t n, int32_t t,
                                     const float* scale, const float* shift, const float* gamma, const float* mean,
                                     const float* invstd, float* dgamma, float* dbeta, float* dw,
                                     float* dbias, void* workspace, int32_t split, mia_stream_t stream) {
  MIA_CHECK_ARG(x && dact && y1 && scale && shift && mean && invstd && dgamma && dbeta && dw && dbias && workspace,
                "fe_conv1_wgrad_bn: null pointer");
  MIA_CHECK_ARG(n > 0 && t >= 64 && t % 2 == 0 && split > 0, "fe_conv1_wgrad_bn: bad sizes");
  MIA_CHECK_ARG(((reinterpret_cast<uintptr_t>(dact) | reinterpret_cast<uintptr_t>(y1)) & 15) == 0,
                "fe_conv1_wgrad_bn: dact / y1 must be 16-byte aligned");
  const int w1 = (t - 64) / 2 + 1;
  float* ws = reinterpret_cast<float*>(workspace);
  TapWArgs r{};
  r.x = reinterpret_cast<const char*>(x);
  r.dy = reinterpret_cast<const char*>(dact);
  r.n = n; r.h = 1; r.wx = t; r.oh = 1; r.ow = w1;
  r.Z = split;
  r.ws = ws;                                       // [split][2][32][64]
  r.by = reinterpret_cast<const bf16*>(y1);
  r.bsc = scale; r.bsh = shift; r.bmean = mean; r.binvstd = invstd;
  r.dbp = ws + (int64_t)split * 2 * 2048;          // [split][32][3]
  r.bP = (int64_t)n * w1;
  float* g13 = r.dbp + (int64_t)split * 96;        // [2][32][64]
  float* g2p = g13 + 2 * 2048;                     // [n][C1_SPLIT*2 + 64]
  double* sums = reinterpret_cast<double*>(g2p + (int64_t)n * (C1_SPLIT * 2 + 64) + 1);  // [160], 8-B aligned below
  sums = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(sums) + 7) & ~uintptr_t(7));
  hipStream_t s = as_stream(stream);
  hipError_t err;
  if (conv1w_v1() || (reinterpret_cast<uintptr_t>(x) & 7)) {  // the wave-private form loads x in 8-byte pairs
    err = tapwgrad_launch<bf16, float, 2, 1, 64, true>(r, s);
  } else {
    conv1_wgrad_bn_kernel<<<(unsigned)r.Z, NT, 0, s>>>(r);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return mia::fail(-(int)err, "fe_conv1_wgrad_bn launch: %s", hipGetErrorString(err));
  EpiDev e{};
  e.ptr = reinterpret_cast<char*>(g13); e.dtype = MIA_F32; e.act = MIA_ACT_NONE; e.ldc = 2 * 2048; e.alpha = 1.f;
  e.act_scale = 1.f;
  launch_splitk_reduce(ws, split, 1, 2 * 2048, e, s);  // slabs [split][4096] -> g13
  conv1_colsum_kernel<<<n * C1_SPLIT, 256, 0, s>>>(x, t, w1, g2p);
  conv1_lin_sums_kernel<<<96 + 64, 256, 0, s>>>(r.dbp, split, g2p, n, sums);
  conv1_lin_final_kernel<<<1, 256, 0, s>>>(g13, sums, r.bP, gamma, mean, invstd, dgamma, dbeta, dw, dbias);
  MIA_LAUNCH_CHECK("fe_conv1_wgrad_bn final");
  return 0;
}
