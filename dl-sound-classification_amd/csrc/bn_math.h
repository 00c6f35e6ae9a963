// BatchNorm + ReLU per-element arithmetic: the one text behind every kernel that applies relu(bn(x)) while staging,
// forms the ReLU+BN backward sums, or applies the BN backward.  This comment is the specification; a kernel that
// moves one of these steps into another kernel's staging or epilogue calls the function and keeps the bits.
//
// Per-channel state (f32, from bn_finalize_kernel, norm.hip): mean mu, invstd is, scale sc = gamma * is,
// shift sh = beta - mu * gamma * is.  All arithmetic below is f32; bf16 inputs are widened exactly (bf16_lo /
// bf16_hi, common.h) and nothing is rounded to bf16 except where a function says so.
//
//   forward      z = fmaf(x, sc, sh)                 one fused multiply-add (one rounding)
//                bn_relu = fmaxf(z, 0.f)
//                bn_relu_on = z > 0.f                the ReLU mask, recomputed from x wherever it is needed
//                bn_relu_pack: bn_relu of eight bf16, each PAIR rounded to bf16 once by pk_bf16 (round to nearest
//                even), the rounding the consumer GEMM's operand staging applies
//   reduce step  g = on ? d : 0.f                    the masked gradient (a bf16 d stays a bf16 value)
//                s1 += g                             plain add             -> dbeta  = sum g
//                s2 = fmaf(g, (x - mu) * is, s2)     xhat = (x - mu) * is rounded once, then ONE fma
//                                                                          -> dgamma = sum g xhat
//   apply        a = gamma * is (gamma null: 1.f * is), mb = dbeta * invP, mg = dgamma * invP, invP = 1.f / (float)P
//                dx = a * (g - mb - (x - mu) * is * mg)
//                a plain expression, evaluated left to right as written; the compiler's default contraction decides
//                which multiply-subtract pairs fuse, the same in every kernel because the text is the same.
// The order in which a thread visits its rows and the fold of the per-thread sums are channel_partials.h's.
//
// Parameter structs: what a thread of the channel_partials.h thread map holds in registers for its 8-channel
// group cg (channels 8 cg .. 8 cg + 7).
//
// NOT on this header, on purpose: the oracle sides of the bit-identical forms tests (pool_bwd_sparse_kernel and
// the per-pixel pool_bn_bwd_apply_kernel in pool.hip, the MIA_CONV1W_V1 / MIA_C1CH_V1 / MIA_REDUCE_V1 kernels) keep
// the expressions written out, so that those tests check this text against an independent one.
#pragma once
#include "common.h"

__device__ __forceinline__ bool bn_relu_on(float x, float sc, float sh) { return fmaf(x, sc, sh) > 0.f; }
__device__ __forceinline__ float bn_relu(float x, float sc, float sh) { return fmaxf(fmaf(x, sc, sh), 0.f); }
// g: the masked gradient
__device__ __forceinline__ void bn_red_step(float g, float x, float mu, float is, float& s1, float& s2) {
  s1 += g;
  s2 = fmaf(g, (x - mu) * is, s2);
}
__device__ __forceinline__ float bn_dx(float g, float x, float a, float mu, float is, float mb, float mg) {
  return a * (g - mb - (x - mu) * is * mg);
}

// eight bf16 of one 8-channel group -> bf16(relu(bn)), sc / sh the group's eight scales / shifts
__device__ __forceinline__ u32x4 bn_relu_pack(u32x4 u, const float* sc, const float* sh) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    o[i] = pk_bf16(bn_relu(bf16_lo(u[i]), sc[2 * i], sh[2 * i]), bn_relu(bf16_hi(u[i]), sc[2 * i + 1], sh[2 * i + 1]));
  return o;
}

struct BnFwd8 {  // forward / mask form
  float sc[8], sh[8];
  __device__ __forceinline__ void load(int cg, const float* __restrict__ scale, const float* __restrict__ shift) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = scale[cg * 8 + i]; sh[i] = shift[cg * 8 + i]; }
  }
  // a null scale / shift is the identity's (1.f / 0.f): the pool forwards of layers with no BN in front
  __device__ __forceinline__ void load_or_identity(int cg, const float* __restrict__ scale,
                                                   const float* __restrict__ shift) {
#pragma unroll
    for (int i = 0; i < 8; ++i) { sc[i] = scale ? scale[cg * 8 + i] : 1.f; sh[i] = shift ? shift[cg * 8 + i] : 0.f; }
  }
};
struct BnRed8 {  // reduce form
  float sc[8], sh[8], mu[8], is[8];
  __device__ __forceinline__ void load(int cg, const float* __restrict__ scale, const float* __restrict__ shift,
                                       const float* __restrict__ mean, const float* __restrict__ invstd) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      sc[i] = scale[cg * 8 + i]; sh[i] = shift[cg * 8 + i]; mu[i] = mean[cg * 8 + i]; is[i] = invstd[cg * 8 + i];
    }
  }
  // element i of a row: returns the masked gradient and adds it to the sums s1, s2 of channel i
  __device__ __forceinline__ float step(int i, float d, float x, float& s1, float& s2) const {
    const float g = bn_relu_on(x, sc[i], sh[i]) ? d : 0.f;
    bn_red_step(g, x, mu[i], is[i], s1, s2);
    return g;
  }
};
struct BnApply8 {  // apply form; P = the number of rows the statistics ran over
  float a[8], mu[8], is[8], mb[8], mg[8];
  __device__ __forceinline__ void load(int cg, const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ invstd, const float* __restrict__ dgamma,
                                       const float* __restrict__ dbeta, float invP) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int c = cg * 8 + i;
      is[i] = invstd[c];
      a[i] = (gamma ? gamma[c] : 1.f) * is[i];
      mu[i] = mean[c];
      mb[i] = dbeta[c] * invP;
      mg[i] = dgamma[c] * invP;
    }
  }
  __device__ __forceinline__ float dx(int i, float g, float x) const {
    return bn_dx(g, x, a[i], mu[i], is[i], mb[i], mg[i]);
  }
};

// byte i of the 8 u8 argmax positions of one (pooled cell, 8-channel group), as the pool forwards pack them
__device__ __forceinline__ int argmax_byte(uint2 am, int i) {
  const uint32_t word = i < 4 ? am.x : am.y;
  return (int)((word >> (8 * (i & 3))) & 0xffu);
}
// and the packing
__device__ __forceinline__ uint2 argmax_pack(const int (&arg)[8]) {
  uint32_t a0 = 0, a1 = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { a0 |= (uint32_t)arg[i] << (8 * i); a1 |= (uint32_t)arg[i + 4] << (8 * i); }
  return make_uint2(a0, a1);
}
