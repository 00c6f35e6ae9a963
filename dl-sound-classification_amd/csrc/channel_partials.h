// Per-channel partial sums: the one reduction protocol behind every BatchNorm-shaped sum of the library
// (BN statistics, dgamma / dbeta, bias gradients) over a channels-last (rows, C) map, C % 8 == 0.
//
// 1. Thread map.  A block has CP_NT = 256 threads and G = C / 8 channel groups.  Thread t owns channel group
//    cg = t % G (channels 8 cg .. 8 cg + 7) and row slot rs = t / G for the whole kernel, and keeps its sums in
//    registers: s1[8], and s2[8] where there are two quantities.  rslots = 256 / G row slots are live; threads
//    t >= G * rslots add nothing and are never read (C = 384: G = 48, rslots = 5, 240 live threads).  Where G does
//    not divide 256 the kernel must keep those threads' sums at zero or out of its loop (`if (rs < rslots)`).
// 2. Fold (cp_fold).  Every thread writes its sums to LDS, red[t * 8 Q + 8 q + i], Q = number of quantities.  After
//    one barrier, entry e < Q C -- quantity q = e / C of channel c = e % C -- is summed by thread e % 256 in f32
//    over the row slots IN SLOT ORDER r = 0, 1, .. rslots - 1, starting from 0.f, and stored to
//    partial[row][c][q].  row is the block's id, or its logical id where the kernel relabels blocks.
// 3. Layout.  partial is f32 [nblk][C][2]: slot 0 = q0, slot 1 = q1.  A one-quantity fold writes slot 0 ONLY (slot 1
//    keeps whatever the workspace held, and its final pass reads slot 0 only).  nblk <= CP_MAXBLK, so the
//    workspace every entry point asks for is CP_MAXBLK * C * 2 * 4 bytes.
// 4. Final pass (cp_final2_kernel, one 256-thread block per channel).  Thread k adds rows k, k + 256, .. in that
//    order in f64 from 0.0; the 256 sums are combined by the fixed tree of block_sum_strided (common.h: halving
//    128, 64, .. 1); the result is rounded to f32 once.  q0 first, then q1.
// Every step has a fixed order and no atomics, so results are bit-identical from run to run and do not depend
// on which block finishes first.  They do depend on nblk: the launch geometry is part of the result.
//
// The quantities: BN statistics q0 = sum (x - K), q1 = sum (x - K)^2; BN backward q0 = sum g (dbeta),
// q1 = sum g xhat (dgamma); apply passes q0 = sum dx (the bias gradient of the layer below).  How g (the ReLU-masked
// gradient), xhat and dx are formed per element, and with which roundings: bn_math.h.
//
// Producers of the layout that do not go through cp_fold, because their sums do not live in this thread map:
//   fe_conv1 / fe_conv3 (feconv.hip), trunk_conv8 (conv8.hip): wave-persistent convolutions, one partial row per
//     WAVE, reduced across lanes with shuffles; read by bn_finalize_kernel, conv8's dgrad by cp_final2_kernel.
//   pool_raw_stats_kernel (pool.hip): thread -> channel group as above, but its fold walks LDS rows t = g, g + G, ..
//     of a [256][17] buffer with the quantity interleaved per thread pair.  The order of adds per output is the
//     same; the padded buffer (bank conflicts) and its resource usage are not, so it keeps its own text.
//   colsum8_kernel (norm.hip): partial[nblk][C] (no slot dimension) for any C % 8 == 0, up to 256 channel groups
//     per blockIdx.y (Gb, not G, is the stride between row slots); idle threads hold zeros instead of being
//     skipped.  Its final pass is cp_final1_kernel, as for colsum_kernel (any C, one column per thread, no fold)
//     and conv3_wgrad_kernel's bias partials [nwaves][32] (conv3w.hip).
//   pool_bwd_sparse_kernel (pool.hip) keeps a verbatim copy of the two-quantity fold: it is the MIA_POOL_V1 side of
//     tests/test_gpu_pool_forms.py and stays independent of the code it checks.
// Consumers: bn_finalize_kernel (norm.hip; mean / invstd from q0, q1 with real work in between) and the two
// final kernels below.
#pragma once
#include "common.h"

constexpr int CP_NT = 256;
constexpr int CP_MAXBLK = MIA_COLSUM_MAXBLK;  // 1024 rows of partial at most

// Step 2.  Q = 1: s2 is not read (pass nullptr).  red: CP_NT * 8 * Q floats of LDS that nothing else uses from
// here on.  The caller guarantees that no thread still reads red's previous contents (cp_fold adds no barrier
// before its writes).
template <int Q>
__device__ __forceinline__ void cp_fold(const float (&s1)[8], const float* s2, int C, int G, int rslots, int row,
                                        float* __restrict__ partial, float* red) {
  static_assert(Q == 1 || Q == 2, "one or two quantities");
  constexpr int S = 8 * Q;  // floats per thread in red
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    red[t * S + i] = s1[i];
    if constexpr (Q == 2) red[t * S + 8 + i] = s2[i];
  }
  __syncthreads();
  for (int e = t; e < Q * C; e += CP_NT) {
    const int q = Q == 1 ? 0 : e / C, c = e - q * C, cg = c >> 3, ci = c & 7;
    float acc = 0.f;
    for (int r = 0; r < rslots; ++r) acc += red[(r * G + cg) * S + q * 8 + ci];
    partial[((int64_t)row * C + c) * 2 + q] = acc;
  }
}
// the same with an LDS buffer of its own
template <int Q>
__device__ __forceinline__ void cp_fold(const float (&s1)[8], const float* s2, int C, int G, int rslots, int row,
                                        float* __restrict__ partial) {
  __shared__ float red[CP_NT * 8 * Q];
  cp_fold<Q>(s1, s2, C, G, rslots, row, partial, red);
}

// Step 4: partial [nblk][C][2] -> out_q0[c] = sum of slot 0, out_q1[c] = sum of slot 1; either may be null.
// Grid C, block 256.
static __global__ __launch_bounds__(256) void cp_final2_kernel(const float* __restrict__ partial, int nblk, int C,
                                                               float* out_q0, float* out_q1) {
  const int c = blockIdx.x;
  const double a = block_sum_strided(partial + (int64_t)c * 2, nblk, (int64_t)C * 2);
  const double b = block_sum_strided(partial + (int64_t)c * 2 + 1, nblk, (int64_t)C * 2);
  if (threadIdx.x != 0) return;
  if (out_q0) out_q0[c] = (float)a;
  if (out_q1) out_q1[c] = (float)b;
}
// the same for a slab without the slot dimension, partial [nblk][C] -> out[c].  Grid C, block 256.
static __global__ __launch_bounds__(256) void cp_final1_kernel(const float* __restrict__ partial, int nblk, int C,
                                                               float* __restrict__ out) {
  const int c = blockIdx.x;
  const double s = block_sum_strided(partial + c, nblk, C);
  if (threadIdx.x == 0) out[c] = (float)s;
}
