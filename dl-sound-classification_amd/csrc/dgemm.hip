// Dense bf16 GEMM with LDS-DMA staging, 128 x 128 tiles, gfx950 (mia_gemm path 5), with its two other modes:
// only the per-tile sums of squares of the product (mia_gemm_sqsum_only) and the product as a weight gradient
// consumed by an optimizer's update in the epilogue (mia_gemm_adam, mia_gemm_sgd, mia_gemm_adamw: one kernel body,
// with the rule of optim_update.h the streaming kernels of optim.hip apply); plus the sum-of-squares pass for
// outputs of other kernels.
#include <type_traits>

#include "gemm_common.h"
#include "../../include/miaudio_optim.h"

namespace {

using namespace mgemm;

constexpr int NT = 256;

// -------------------------------------------------------------------------- dense bf16 GEMM (LDS-DMA)
// C = A . B^T for bf16 DENSE operands in any KC/RC layout combination (AST linears fwd/dgrad/wgrad,
// EnvNet FC layers).  128x128x64 tiles, 4 waves (2x2, 64x64 each, MFMA 32x32x16), both operands
// staged global -> LDS with global_load_lds_dwordx4 (no register staging, no VALU address work
// in the loop beyond a pointer bump), double-buffered: the next K-tile's DMA is issued before the
// current tile's MFMAs, retired with a counted vmcnt + raw s_barrier.  LDS images are XOR-swizzled
// on the SOURCE address (the DMA destination is lane-linear): KC rows of 128 B permute their 16-B
// chunks by (row & 7) (conflict-free ds_read_b128 per 8 lanes); RC rows of 256 B permute their
// 32-B blocks by (k & 3) (conflict-free ds_read_b64_tr_b16 per 16 lanes).  Blocks are remapped so
// that neighbouring tiles share an XCD (bijective XCD swizzle) and walk M fastest (B-tile reuse).


typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

// block-wide sum of one double per thread (4 waves), written by thread 0: a tile's sum of squares.
// `red` is NT/64 doubles of the caller's LDS (inside a GEMM kernel: its one staging array -- a second
// __shared__ object there makes hipcc wait vmcnt(0) at every K-step barrier); the leading barrier
// lets the caller's last reads of that space finish first.
__device__ __forceinline__ void tile_sqsum_store(double* dst, double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    *dst = s;
  }
}

// MiaEpilogue.sqsum for a GEMM whose kernel did not produce it (other paths, split-K): one block
// per 128 x 128 tile of the f32 output C (ldc), same slots and per-tile order of accumulation
__global__ __launch_bounds__(NT) void tile_sqsum_kernel(const float* __restrict__ c, int64_t ldc, int64_t M, int64_t N,
                                                        int nbn, double* __restrict__ out) {
  const int bm = blockIdx.x / nbn, bn = blockIdx.x - (blockIdx.x / nbn) * nbn;
  const int64_t m0 = (int64_t)bm * 128, n0 = (int64_t)bn * 128;
  float sq = 0.f;
  for (int e = threadIdx.x; e < 128 * 128; e += NT) {
    const int64_t m = m0 + e / 128, n = n0 + e % 128;
    if (m < M && n < N) {
      const float v = c[m * ldc + n];
      sq = fmaf(v, v, sq);
    }
  }
  __shared__ double red[NT / 64];
  tile_sqsum_store(out + blockIdx.x, (double)sq, red);
}

// 16-B chunk swizzle of the k-contiguous (KC) 128 x 64 tile images: chunk c of row r sits at c ^ swz(r).
// A 32-row fragment's ds_read_b128 lane groups ({0-3, 12-15, 20-27} and its complement) hold rows 8 and
// 24 apart, which r & 7 maps to the same chunk of the same bank half (2-way conflicts); (r >> 1) & 7 gives
// the 8 even and the 8 odd rows of each group distinct chunks
__device__ __forceinline__ int dkc_swz(int r) { return (r >> 1) & 7; }

template <int L>
struct DLoader {
  // per-lane source pointers for this wave's 4 DMA instructions of a tile, advanced per K-tile
  const bf16* src[4];
  int64_t step;
  __device__ __forceinline__ void init(const bf16* base, int64_t ld, int64_t rows_or_cols, int64_t r0, int64_t kbeg,
                                       int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = wave * 4 + i;
      if constexpr (L == MIA_LAYOUT_KC) {
        const int r = 8 * j + (lane >> 3);
        const int c = (lane & 7) ^ dkc_swz(r);
        int64_t row = r0 + r;
        if (row >= rows_or_cols) row = rows_or_cols - 1;
        src[i] = base + row * ld + kbeg + c * 8;
      } else {
        const int kr = 4 * j + (lane >> 4);
        const int p = lane & 15;
        const int c = 2 * ((p >> 1) ^ (kr & 3)) + (p & 1);
        int64_t col = r0 + c * 8;
        if (col + 8 > rows_or_cols) col = rows_or_cols - 8;
        src[i] = base + (kbeg + kr) * ld + col;
      }
    }
    step = L == MIA_LAYOUT_KC ? 64 : 64 * ld;
  }
  __device__ __forceinline__ void issue(char* tile, int wave) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_global_load_lds((glb_vp)src[i], (lds_vp)(tile + (wave * 4 + i) * 1024), 16, 0, 0);
      src[i] += step;
    }
  }
};

template <int L>
__device__ __forceinline__ bf16x8 dfrag(const char* tile, int rbase, int ks, int lane) {
  if constexpr (L == MIA_LAYOUT_KC) {
    const int rr = rbase + (lane & 31);
    const int c = 2 * ks + (lane >> 5);
    return *reinterpret_cast<const bf16x8*>(tile + rr * 128 + ((c ^ dkc_swz(rr)) * 16));
  } else {
    const int i16 = lane & 15, gq = lane >> 4;
    const int col = rbase + 16 * (gq & 1) + 4 * (i16 & 3);
    const int kr = ks * 16 + 8 * (gq >> 1) + (i16 >> 2);
    const char* p0 = tile + kr * 256 + (((col >> 4) ^ (kr & 3)) * 32) + (col & 15) * 2;
    // (hipcc waits vmcnt(0) -- for the next tile's DMA -- before the first of these builtin reads in
    // each K-step; an inline-asm variant without that wait measured the same on the wgrad shapes)
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0 + 4 * 256));
    typedef short s16x8 __attribute__((ext_vector_type(8)));
    const s16x8 cc = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, cc);
  }
}


constexpr int TILE = 128 * 64 * 2;  // one operand's 128 x 64 bf16 K-tile; a kernel's one LDS array holds four

// The product of RC x RC operands as a weight gradient that is never stored: the epilogue applies rule R of
// optim_update.h (the arithmetic of the streaming kernels, with NS state tensors) to the parameter rows this tile is
// the gradient of.  The one body of mia_gemm_adam, mia_gemm_sgd and mia_gemm_adamw: dgemm_kernel's RC x RC main
// loop, tile order without grouping (column-block-major; row-block-major measured 2.14 -> 2.18 ms for Adam on
// EnvNet's FC1) and full-tile staging.  dgemm_kernel keeps its own text of these: sharing them through inlined
// functions reorders the address arithmetic of the plain instantiations, which the model GEMMs were tuned as.
template <int NS, class R>
__device__ __forceinline__ void dgemm_update_tile(const DArgs& g, const UpdateEpi<R>& o, char* smem) {
  constexpr int L = MIA_LAYOUT_RC;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = g.nbm * g.nbn;
  const int orig = blockIdx.x;
  const int xcd = orig % 8, q8 = nwg / 8, r8 = nwg % 8;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  const int bm = wgid % g.nbm, bn = wgid / g.nbm;
  const int64_t m0 = (int64_t)bm * 128, n0 = (int64_t)bn * 128;
  const int nk = (int)(g.K / 64);

  DLoader<L> la;
  DLoader<L> lb;
  la.init(g.a, g.lda, g.M, m0, 0, wave, lane);
  lb.init(g.b, g.ldb, g.N, n0, 0, wave, lane);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // the parameter rows of the tile's first 16-B group per lane -- p and its state -- are fetched before the main
  // loop, so their HBM latency hides under it; later groups are fetched one group ahead of their use
  f32x4 pv[2][4], av[2][4], bv[2][4];
  const int acol = (lane & 31) * 4;
  auto fetch = [&](int it0, int b) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t off = (m0 + wave * 32 + (it0 + u) * 2 + (lane >> 5)) * o.ld + n0 + acol;
      pv[b][u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(o.p + off));
      if constexpr (NS > 0) av[b][u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(o.s0 + off));
      if constexpr (NS > 1) bv[b][u] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(o.s1 + off));
    }
  };
  fetch(0, 0);

  if (nk > 0) {
    la.issue(smem, wave);
    lb.issue(smem + TILE, wave);
  }
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * 2 * TILE;
    if (kt + 1 < nk) {
      char* nxt = smem + ((kt + 1) & 1) * 2 * TILE;
      la.issue(nxt, wave);
      lb.issue(nxt + TILE, wave);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* As = cur;
    const char* Bs = cur + TILE;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = dfrag<L>(As, wm * 64 + i * 32, ks, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = dfrag<L>(Bs, wn * 64 + j * 32, ks, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  float* tile = reinterpret_cast<float*>(smem);  // [128][128], 32-dword halves swapped on row bit 2
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int col = wn * 64 + j * 32 + (lane & 31);
        tile[row * 128 + (col ^ (((row >> 2) & 1) << 5))] = acc[i][j][r];
      }
  __syncthreads();
  // the gradient is the f32 product itself, read back as whole 512-B rows, two rows per wave instruction; every
  // byte of p and its state is touched once, so loads and stores are non-temporal
  const float coef = o.coef[0];
  const bool first = o.first != 0;
#pragma unroll
  for (int grp = 0; grp < 4; ++grp) {
    const int b = grp & 1;
    if (grp + 1 < 4) fetch((grp + 1) * 4, b ^ 1);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int row = wave * 32 + (grp * 4 + u) * 2 + (lane >> 5);
      const int64_t off = (m0 + row) * o.ld + n0 + acol;
      const f32x4 gv = *reinterpret_cast<const f32x4*>(tile + row * 128 + (acol ^ (((row >> 2) & 1) << 5)));
      f32x4 p4 = pv[b][u], a4 = {0.f, 0.f, 0.f, 0.f}, b4 = a4;
      if constexpr (NS > 0) a4 = av[b][u];
      if constexpr (NS > 1) b4 = bv[b][u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float sa = a4[e], sb = b4[e];
        p4[e] = mopt::apply<NS>(o.rule, coef, first, p4[e], gv[e], sa, sb);
        a4[e] = sa;
        b4[e] = sb;
      }
      __builtin_nontemporal_store(p4, reinterpret_cast<f32x4*>(o.p + off));
      if constexpr (NS > 0) __builtin_nontemporal_store(a4, reinterpret_cast<f32x4*>(o.s0 + off));
      if constexpr (NS > 1) __builtin_nontemporal_store(b4, reinterpret_cast<f32x4*>(o.s1 + off));
      if (o.shadow) {
        const bf16x4 h4 = {(bf16)p4[0], (bf16)p4[1], (bf16)p4[2], (bf16)p4[3]};
        __builtin_nontemporal_store(h4, reinterpret_cast<bf16x4*>(o.shadow + off));
      }
    }
  }
}

// mia_gemm_sgd (NS 0 or 1) and mia_gemm_adamw
template <int NS, class R>
__global__ __launch_bounds__(NT) void dgemm_optim_kernel(DArgs g, UpdateEpi<R> o) {
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];
  dgemm_update_tile<NS>(g, o, smem);
}

template <int LA, int LB, bool ADAM = false>
__global__ __launch_bounds__(NT) void dgemm_kernel(DArgs g) {
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];
  if constexpr (ADAM) {  // mia_gemm_adam, under this kernel's name: the step profile attributes the Adam step by it
    dgemm_update_tile<2>(g, g.upd, smem);
    return;
  }
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int nwg = g.nbm * g.nbn;
  const int orig = blockIdx.x;
  const int xcd = orig % 8, q8 = nwg / 8, r8 = nwg % 8;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + orig / 8;
  int bm, bn;
  if (g.nfast) {  // grouped order: gm row blocks x all column tiles, M fastest inside a group
    const int gsize = g.gm * g.nbn;
    const int grp = wgid / gsize, rem = wgid - grp * gsize;
    const int gme = min(g.gm, g.nbm - grp * g.gm);
    bm = grp * g.gm + rem % gme;
    bn = rem / gme;
  } else {
    bm = wgid % g.nbm;
    bn = wgid / g.nbm;
  }
  const int64_t m0 = (int64_t)bm * 128, n0 = (int64_t)bn * 128;
  const int z = blockIdx.y;
  const int64_t kbeg = (int64_t)z * g.kper;
  int64_t kend = kbeg + g.kper;
  if (kend > g.K) kend = g.K;
  const int nk = kend > kbeg ? (int)((kend - kbeg) / 64) : 0;

  DLoader<LA> la;
  DLoader<LB> lb;
  la.init(g.a, g.lda, g.M, m0, kbeg, wave, lane);
  lb.init(g.b, g.ldb, g.N, n0, kbeg, wave, lane);

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    la.issue(smem, wave);
    lb.issue(smem + TILE, wave);
  }
  for (int kt = 0; kt < nk; ++kt) {
    char* cur = smem + (kt & 1) * 2 * TILE;
    if (kt + 1 < nk) {
      char* nxt = smem + ((kt + 1) & 1) * 2 * TILE;
      la.issue(nxt, wave);
      lb.issue(nxt + TILE, wave);
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    const char* As = cur;
    const char* Bs = cur + TILE;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = dfrag<LA>(As, wm * 64 + i * 32, ks, lane);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = dfrag<LB>(Bs, wn * 64 + j * 32, ks, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  }

  // plain f32 output of a full tile (the wide weight-gradient GEMMs, e.g. EnvNet FC1: 1.38 GB of f32
  // per step): the whole 128x128 tile is staged in the (now idle) 64 KB of LDS and written as whole
  // 512-B rows, two rows per wave store instruction, non-temporal (read next by the optimizer pass)
  const bool plain = g.mode != 0 ||
                     (g.split == 1 && g.e.dtype == MIA_F32 && g.e.act == MIA_ACT_NONE && !g.e.bias &&
                      !g.e.accumulate && !g.e.rm_inner && g.e.alpha == 1.f && m0 + 128 <= g.M && n0 + 128 <= g.N &&
                      (g.e.ldc & 3) == 0 && ((reinterpret_cast<uintptr_t>(g.e.ptr)) & 15) == 0);
  if (plain) {
    // the tile's sum of squares straight from the accumulators (one fixed order shared by the stored
    // and the sums-only forms, so a deferred gradient's norm equals the materialised one's bit for bit)
    float sq = 0.f;
    if (g.e.sqsum) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) sq = fmaf(acc[i][j][r], acc[i][j][r], sq);
    }
    if (g.mode == 1) {  // sums only: nothing staged, nothing stored
      tile_sqsum_store(g.e.sqsum + (int64_t)bm * g.nbn + bn, (double)sq, reinterpret_cast<double*>(smem));
      return;
    }
    float* tile = reinterpret_cast<float*>(smem);  // [128][128], 32-dword halves swapped on row bit 2
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int col = wn * 64 + j * 32 + (lane & 31);
          tile[row * 128 + (col ^ (((row >> 2) & 1) << 5))] = acc[i][j][r];
        }
    __syncthreads();
    float* out = reinterpret_cast<float*>(g.e.ptr);
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
      const int row = wave * 32 + it * 2 + (lane >> 5);
      const int col = (lane & 31) * 4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * 128 + (col ^ (((row >> 2) & 1) << 5)));
      __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out + (m0 + row) * g.e.ldc + n0 + col));
    }
    if (g.e.sqsum) tile_sqsum_store(g.e.sqsum + (int64_t)bm * g.nbn + bn, (double)sq, reinterpret_cast<double*>(smem));
    return;
  }
  // the same full-tile staging for a bf16 output with optional bias / ReLU (AST qkv forward and the
  // plain backward-data GEMMs): 16 lanes cover one 256-B output row, 4 rows per store instruction
  const bool save = g.e.act == MIA_ACT_GELU_SAVE || g.e.act == MIA_ACT_GELU_SAVE_D;
  const bool save_d = g.e.act == MIA_ACT_GELU_SAVE_D;
  // drop-mode row map (MIA_RM_DROP): plain / bias / ReLU output only
  const bool drop = g.e.rm_inner && g.e.rm_offset == MIA_RM_DROP && g.e.rm_istride == 1 &&
                    (g.e.act == MIA_ACT_NONE || g.e.act == MIA_ACT_RELU);
  const bool plain16 = g.split == 1 && g.e.dtype == MIA_BF16 &&
                       (g.e.act == MIA_ACT_NONE || g.e.act == MIA_ACT_RELU || g.e.act == MIA_ACT_GELU ||
                        (save && g.e.aux_dtype == MIA_BF16 && (g.e.ldaux & 7) == 0 &&
                         ((reinterpret_cast<uintptr_t>(g.e.aux)) & 15) == 0)) &&
                       !g.e.accumulate && (!g.e.rm_inner || drop) &&
                       g.e.alpha == 1.f && m0 + 128 <= g.M && n0 + 128 <= g.N && (g.e.ldc & 7) == 0 &&
                       ((reinterpret_cast<uintptr_t>(g.e.ptr)) & 15) == 0;
  if (plain16) {
    float* tile = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          const int col = wn * 64 + j * 32 + (lane & 31);
          tile[row * 128 + (col ^ (((row >> 2) & 1) << 5))] = acc[i][j][r];
        }
    __syncthreads();
    const int col = (lane & 15) * 8;
    float bv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) bv[c] = g.e.bias ? g.e.bias[n0 + col + c] : 0.f;
    const bool relu = g.e.act == MIA_ACT_RELU, gelu = g.e.act == MIA_ACT_GELU || save;
    bf16* out = reinterpret_cast<bf16*>(g.e.ptr);
    auto pack = [](const float* f) {
      uint32_t w4[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        w4[q] = pk_bf16(f[2 * q], f[2 * q + 1]);
      }
      return make_uint4(w4[0], w4[1], w4[2], w4[3]);
    };
#pragma unroll 4
    for (int it = 0; it < 8; ++it) {
      const int row = wave * 32 + it * 4 + (lane >> 4);
      const int sw = ((row >> 2) & 1) << 5;
      const f32x4 a = *reinterpret_cast<const f32x4*>(tile + row * 128 + (col ^ sw));
      const f32x4 b = *reinterpret_cast<const f32x4*>(tile + row * 128 + ((col + 4) ^ sw));
      float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] += bv[c];
      if (save) {  // GELU_SAVE(_D): the pre-activation or gelu' goes to aux (MLP fc1, read by the backward)
        float d[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) d[c] = save_d ? gelu_erf_grad((float)(bf16)v[c]) : v[c];  // gelu' of bf16 u
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16*>(const_cast<char*>(g.e.aux)) + (m0 + row) * g.e.ldaux +
                                  n0 + col) = pack(d);
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] = relu ? fmaxf(v[c], 0.f) : (gelu ? gelu_erf(v[c]) : v[c]);
      int64_t prow = m0 + row;
      if (drop) {
        const int64_t x = prow % g.e.rm_inner;
        if (x >= g.e.rm_outer) continue;
        prow = (prow / g.e.rm_inner) * g.e.rm_outer + x;
      }
      *reinterpret_cast<uint4*>(out + prow * g.e.ldc + n0 + col) = pack(v);
    }
    return;
  }

  float* stage = reinterpret_cast<float*>(smem) + wave * (32 * 33);
  double sqg = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        stage[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 33 + (lane & 31)] = acc[i][j][r];
      __syncthreads();
      const int row = lane >> 1, c0 = (lane & 1) * 16;
      const int64_t m = m0 + wm * 64 + i * 32 + row;
      const int64_t nb = n0 + wn * 64 + j * 32 + c0;
      if (m < g.M && nb < g.N) {
        float v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = stage[row * 33 + c0 + c];
        if (g.split > 1) {
          float* dst = g.ws + ((int64_t)z * g.M + m) * g.N + nb;
          if (nb + 16 <= g.N && (g.N & 3) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              reinterpret_cast<float4*>(dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
          } else {
            for (int c = 0; c < 16; ++c)
              if (nb + c < g.N) dst[c] = v[c];
          }
        } else {
          epi_store16(g.e, m, nb, g.N, v);
          if (g.e.sqsum) {
            float sq = 0.f;
            for (int c = 0; c < 16; ++c)
              if (nb + c < g.N) sq = fmaf(v[c], v[c], sq);
            sqg += sq;
          }
        }
      }
      __syncthreads();
    }
  if (g.e.sqsum && g.split == 1)
    tile_sqsum_store(g.e.sqsum + (int64_t)bm * g.nbn + bn, sqg, reinterpret_cast<double*>(smem));
}

template <int LA, int LB>
hipError_t dgemm_launch2(const DArgs& d, hipStream_t s) {
  dim3 grid((unsigned)(d.nbm * d.nbn), (unsigned)d.split);
  dgemm_kernel<LA, LB><<<grid, NT, 0, s>>>(d);
  return hipGetLastError();
}

hipError_t dgemm_launch(const DArgs& d, int la, int lb, hipStream_t s) {
  if (la == MIA_LAYOUT_KC && lb == MIA_LAYOUT_KC) return dgemm_launch2<MIA_LAYOUT_KC, MIA_LAYOUT_KC>(d, s);
  if (la == MIA_LAYOUT_KC) return dgemm_launch2<MIA_LAYOUT_KC, MIA_LAYOUT_RC>(d, s);
  if (lb == MIA_LAYOUT_KC) return dgemm_launch2<MIA_LAYOUT_RC, MIA_LAYOUT_KC>(d, s);
  return dgemm_launch2<MIA_LAYOUT_RC, MIA_LAYOUT_RC>(d, s);
}

// operands, extents and tiling of a launch; tile order, epilogue and mode are the caller's (zero here)
DArgs dgemm_args(const MiaOperand& A, const MiaOperand& B, int64_t M, int64_t N, int64_t K, int split) {
  DArgs d;
  memset(&d, 0, sizeof(d));
  d.a = reinterpret_cast<const bf16*>(A.ptr); d.b = reinterpret_cast<const bf16*>(B.ptr);
  d.lda = A.ld; d.ldb = B.ld; d.M = M; d.N = N; d.K = K;
  d.split = split;
  d.kper = cdiv(cdiv(K, split), 64) * 64;
  d.nbm = (int)cdiv(M, 128); d.nbn = (int)cdiv(N, 128);
  return d;
}

}  // namespace

namespace mgemm {

bool dgemm_ok(const MiaOperand& A, const MiaOperand& B, int64_t M, int64_t N, int64_t K, int compute) {
  if (compute != MIA_BF16 || K < 64 || K % 64 != 0 || M < 64 || N < 64) return false;
  if (A.kind != MIA_OP_DENSE || B.kind != MIA_OP_DENSE) return false;
  if (A.dtype != MIA_BF16 || B.dtype != MIA_BF16 || A.pre != MIA_PRE_NONE || B.pre != MIA_PRE_NONE) return false;
  if (A.ld % 8 || B.ld % 8 || (reinterpret_cast<uintptr_t>(A.ptr) & 15) || (reinterpret_cast<uintptr_t>(B.ptr) & 15))
    return false;
  if (A.layout == MIA_LAYOUT_KC) { if (A.rows != M || A.cols < K) return false; }
  else { if (A.rows < K || A.cols != M || M % 8) return false; }
  if (B.layout == MIA_LAYOUT_KC) { if (B.rows != N || B.cols < K) return false; }
  else { if (B.rows < K || B.cols != N || N % 8) return false; }
  if (cdiv(M, 128) * cdiv(N, 128) >= (1ll << 31)) return false;
  return true;
}

int dgemm_run(const MiaOperand& A, const MiaOperand& B, const MiaEpilogue& E, int64_t M, int64_t N, int64_t K,
              int split, void* workspace, hipStream_t s) {
  DArgs d = dgemm_args(A, B, M, N, K, split);
  // tall GEMMs (AST linears: M = tokens, N <= 3072): grouped tile order (DArgs::gm) so each A row
  // block is read from HBM once (at batch 256 the activations exceed the 256 MB Infinity Cache; an
  // M-fastest walk re-streamed them once per column tile: 12-15 GB per launch, rocprof FETCH_SIZE)
  // and each B column tile once per group of gm row blocks
  d.nfast = (d.split == 1 && d.nbn <= 32 && d.nbm >= 4 * d.nbn) ? 1 : 0;
  d.gm = (int)std::max<int64_t>(1, std::min<int64_t>(16, (2ll << 20) / (128 * 2 * std::max<int64_t>(K, 64))));
  d.ws = reinterpret_cast<float*>(workspace);
  d.e = to_dev(E);
  hipError_t err = dgemm_launch(d, A.layout, B.layout, s);
  if (err != hipSuccess) return mia::fail(-(int)err, "dgemm launch: %s", hipGetErrorString(err));
  if (d.split > 1) launch_splitk_reduce(d.ws, d.split, M, N, d.e, s);
  return 0;
}

// MiaEpilogue.sqsum after a GEMM whose kernel did not write the slots itself (tile_sqsum_kernel)
int tile_sqsum_run(const float* c, int64_t ldc, int64_t M, int64_t N, double* sqsum, hipStream_t s) {
  const int64_t nb = mia_gemm_sqsum_slots(M, N);
  MIA_CHECK_ARG(nb < (1ll << 31), "gemm sqsum: too many tiles");
  tile_sqsum_kernel<<<(unsigned)nb, NT, 0, s>>>(c, ldc, M, N, (int)cdiv(N, 128), sqsum);
  MIA_LAUNCH_CHECK("gemm sqsum");
  return 0;
}

}  // namespace mgemm

extern "C" int64_t mia_gemm_sqsum_slots(int64_t M, int64_t N) { return cdiv(M, 128) * cdiv(N, 128); }

// The dense 128 x 128 kernel outside mia_gemm (the sums-only and the update forms): full tiles, no split.
static int wgrad_args(const char* who, const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K,
                      DArgs* d) {
  MIA_CHECK_ARG(A && B, "%s: null descriptor", who);
  MIA_CHECK_ARG(dgemm_ok(*A, *B, M, N, K, MIA_BF16) && M % 128 == 0 && N % 128 == 0,
                "%s: needs bf16 dense operands, M and N multiples of 128, K a multiple of 64", who);
  *d = dgemm_args(*A, *B, M, N, K, 1);
  return 0;
}

extern "C" int mia_gemm_sqsum_only(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K,
                                   double* sqsum, mia_stream_t stream) {
  MIA_CHECK_ARG(sqsum, "gemm_sqsum_only: null sqsum");
  DArgs d;
  if (int rc = wgrad_args("gemm_sqsum_only", A, B, M, N, K, &d)) return rc;
  // row-block-major tile order (an XCD's concurrent tiles share their dY rows; 0.271 -> 0.259 ms for FC1)
  d.nfast = 1; d.gm = 1;
  d.e.dtype = MIA_F32; d.e.alpha = 1.f; d.e.sqsum = sqsum;
  d.mode = 1;
  hipError_t err = dgemm_launch(d, A->layout, B->layout, as_stream(stream));
  if (err != hipSuccess) return mia::fail(-(int)err, "gemm_sqsum_only launch: %s", hipGetErrorString(err));
  return 0;
}

// mia_gemm_adam, mia_gemm_sgd and mia_gemm_adamw: the checks they share and the launch
template <int NS, class R>
static int dgemm_update(const char* who, const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K,
                        const UpdateEpi<R>& o, mia_stream_t stream) {
  DArgs d;
  if (int rc = wgrad_args(who, A, B, M, N, K, &d)) return rc;
  // the weight-gradient layouts only (dY and X both K-major: RC x RC)
  MIA_CHECK_ARG(A->layout == MIA_LAYOUT_RC && B->layout == MIA_LAYOUT_RC, "%s: needs RC operands", who);
  MIA_CHECK_ARG(o.p && o.coef && (NS < 1 || o.s0) && (NS < 2 || o.s1), "%s: null pointer", who);
  MIA_CHECK_ARG(o.ld >= N && o.ld % 4 == 0 &&
                    ((reinterpret_cast<uintptr_t>(o.p) | reinterpret_cast<uintptr_t>(o.s0) |
                      reinterpret_cast<uintptr_t>(o.s1)) & 15) == 0 &&
                    (reinterpret_cast<uintptr_t>(o.shadow) & 7) == 0,
                "%s: parameter and state rows must be 16-B aligned (ld %% 4 == 0), the shadow 8-B aligned", who);
  const dim3 grid((unsigned)(d.nbm * d.nbn));
  hipStream_t s = as_stream(stream);
  if constexpr (std::is_same_v<R, mopt::AdamRule>) {
    d.upd = o;
    dgemm_kernel<MIA_LAYOUT_RC, MIA_LAYOUT_RC, true><<<grid, NT, 0, s>>>(d);
  } else {
    dgemm_optim_kernel<NS><<<grid, NT, 0, s>>>(d, o);
  }
  MIA_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int mia_gemm_adam(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K, float* param,
                             float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t ld, const float* coef,
                             float lr_over_bc1, float bc2_sqrt, float beta1, float beta2, float eps, float weight_decay,
                             mia_stream_t stream) {
  const UpdateEpi<mopt::AdamRule> o{param, exp_avg, exp_avg_sq, reinterpret_cast<bf16*>(shadow_bf16), coef, ld, 0,
                                    {lr_over_bc1, bc2_sqrt, beta1, beta2, eps, weight_decay}};
  return dgemm_update<2>("gemm_adam", A, B, M, N, K, o, stream);
}

extern "C" int mia_gemm_adamw(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K, float* param,
                              float* exp_avg, float* exp_avg_sq, void* shadow_bf16, int64_t ld, const float* coef,
                              float lr_over_bc1, float bc2_sqrt, float beta1, float beta2, float eps, float lr,
                              float weight_decay, mia_stream_t stream) {
  const UpdateEpi<mopt::AdamWRule> o{param, exp_avg, exp_avg_sq, reinterpret_cast<bf16*>(shadow_bf16), coef, ld, 0,
                                     {lr_over_bc1, bc2_sqrt, beta1, beta2, eps, mopt::adamw_decay(lr, weight_decay)}};
  return dgemm_update<2>("gemm_adamw", A, B, M, N, K, o, stream);
}

extern "C" int mia_gemm_sgd(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K, float* param,
                            float* momentum_buf, void* shadow_bf16, int64_t ld, const float* coef, float lr,
                            float momentum, float dampening, float weight_decay, int32_t nesterov, int32_t first_use,
                            mia_stream_t stream) {
  MIA_CHECK_ARG((momentum != 0.f) == (momentum_buf != nullptr), "gemm_sgd: momentum_buf goes with momentum != 0");
  MIA_CHECK_ARG(!nesterov || (momentum > 0.f && dampening == 0.f),
                "gemm_sgd: nesterov needs a momentum and zero dampening");
  const UpdateEpi<mopt::SgdRule> o{param, momentum_buf, nullptr, reinterpret_cast<bf16*>(shadow_bf16), coef, ld,
                                   first_use, mopt::sgd_rule(lr, momentum, dampening, weight_decay, nesterov)};
  return momentum_buf ? dgemm_update<1>("gemm_sgd", A, B, M, N, K, o, stream)
                      : dgemm_update<0>("gemm_sgd", A, B, M, N, K, o, stream);
}
