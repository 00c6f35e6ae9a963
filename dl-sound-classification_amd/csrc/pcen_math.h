// PCEN arithmetic shared by the (B, F, Tp) kernels of leaf.hip and the channels-last kernels of leaftrunk.hip:
//   M[j] = mean of P[j - 2 .. j + 2] (zeros outside the row),  D = eps + M[j],  y[j] = log(P[j] / D^r + delta).
// Both files call these functions, so their f32 results carry the same bits (tests/test_gpu_leaftrunk.py::
// test_pcen_channels_last asserts it); staging, tiling and the transposed stores stay with the kernels.
// Every f32 expression below is ONE expression: do not split, reassociate or hoist a factor.
#pragma once
#include "common.h"

// row[j] = P[b][f][j] for every j the taps touch that lies in [0, Tp)
__device__ __forceinline__ float pcen_m(const float* __restrict__ row, int Tp, int j) {
  float s = 0.f;
#pragma unroll
  for (int d = -2; d <= 2; ++d) s += (j + d >= 0 && j + d < Tp) ? row[j + d] : 0.f;
  return s / 5.f;
}

__device__ __forceinline__ float pcen_fwd_value(const float* __restrict__ row, int Tp, int j, float eps, float r,
                                                float delta) {
  const float D = eps + pcen_m(row, Tp, j);
  return logf(row[j] / powf(D, r) + delta);
}

// Backward of frame i: gP[i] = sum over the taps j = i + d, d = -2 .. 2 (inside the row), of via_m, plus direct at
// d == 0, added in that order; dr / ddelta are the row's parameter-gradient terms of frame j, taken at d == 0 only.
struct PcenTap {
  float via_m;   // gy[j] / u * d u / d M[j] * d M[j] / d P[i]
  float direct;  // gy[j] / u * D^-r
  float dr, ddelta;
};
__device__ __forceinline__ PcenTap pcen_bwd_tap(const float* __restrict__ row, int Tp, int j, float eps, float gyj,
                                                float rf, float df) {
  const float D = eps + pcen_m(row, Tp, j);
  const float pw = powf(D, -rf);  // D^-r
  const float u = row[j] * pw + df;
  const float gu = gyj / u;
  return PcenTap{gu * (-rf * row[j] * pw / D) * 0.2f, gu * pw, gu * row[j] * pw * -logf(D), gu};
}

// Sums over the 256 threads of a block of R rows' (sr, sd) pairs in f64: red[q][0][0] = sum sr[q], red[q][1][0] =
// sum sd[q] (halving tree 128, 64, .. 1, the same for every R).  Ends with a barrier; the caller places one before
// it where red is still being read.
template <int R>
__device__ __forceinline__ void pcen_row_tree(double (&red)[R][2][256], const double* sr, const double* sd) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < R; ++q) { red[q][0][tid] = sr[q]; red[q][1][tid] = sd[q]; }
  __syncthreads();
  for (int wd = 128; wd > 0; wd >>= 1) {
    if (tid < wd) {
#pragma unroll
      for (int q = 0; q < R; ++q) {
        red[q][0][tid] += red[q][0][tid + wd];
        red[q][1][tid] += red[q][1][tid + wd];
      }
    }
    __syncthreads();
  }
}

// part [B][F][2] (f64 row sums) -> dr[f], ddelta[f]: clips added in order
static __global__ __launch_bounds__(256) void pcen_param_reduce_kernel(const double* __restrict__ part,
                                                                       float* __restrict__ dr,
                                                                       float* __restrict__ ddelta, int B, int F) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  double a = 0.0, c = 0.0;
  for (int b = 0; b < B; ++b) {
    a += part[((int64_t)b * F + f) * 2];
    c += part[((int64_t)b * F + f) * 2 + 1];
  }
  dr[f] = (float)a;
  ddelta[f] = (float)c;
}
