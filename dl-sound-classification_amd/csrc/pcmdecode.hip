// WAV ingestion on the device (include/miaudio_wav.h): PCM / float sample bytes -> mono f32, the clip's peak, and
// the peak division.  Pure streams: file bytes in, 4 B per frame out.
//
// One lane owns one 16-B group of four output frames.  As in cropgather.hip the groups are cut on the output
// ADDRESS: with shift = (element address of the clip's first output sample) & 3, group j holds frames
// t = 4 j - shift .. 4 j - shift + 3, so every group that lies whole inside the clip is one aligned 16-B store and
// the at most two that overhang its ends store element by element.  The four frames of a lane are one contiguous
// span of NB = 4 * channels * bytes_per_sample input bytes (a multiple of 4), which the lane brings into NB / 4
// registers in one of two ways:
//   * the span lies whole inside the clip's bytes and starts on a 4-B boundary: one memcpy of NB bytes at
//     alignment 4, which compiles to global_load_dwordx4 / x3 / x2 / x1 (16-B loads for every span >= 16 B);
//   * otherwise (the head and tail lanes of every clip, and every lane of a clip whose byte_off is not a multiple
//     of 4): the NB / 4 + 1 ALIGNED dwords that cover the span, each loaded as a dword only if all four of its
//     bytes lie inside the clip and assembled from single in-range bytes otherwise, then funnel-shifted into
//     place.  A byte outside the clip reads as 0 and belongs only to frames that are neither stored nor counted.
// In both ways every load reads src[q .. q + width) behind a check of 0 <= q and q + width <= len, with
// src[0 .. len) the clip's own bytes, so no load leaves them -- in particular not the dword read that brings in
// the last 3-byte sample of a packed s24 clip.
// Samples sit at compile-time positions of the span (the kernel is instantiated per format and channel count), so
// the unpacking is shifts and converts on registers.  A workgroup walks its groups of a clip with a running
// maximum of |mono| bits and a count of non-finite samples in registers, folds the four waves through LDS and
// issues one atomicMax (one atomicAdd) per clip.
#include "common.h"

#include "../../include/miaudio_wav.h"

namespace {


constexpr int WG = 256;

__host__ __device__ constexpr int bytes_per_sample(int fmt) {
  return fmt == MIA_PCM_U8 ? 1 : fmt == MIA_PCM_S16 ? 2 : fmt == MIA_PCM_S24 ? 3 : fmt == MIA_PCM_F64 ? 8 : 4;
}

// sample s (a compile-time position after unrolling) of a span held in w[NW], little-endian
template <int FMT, int NW> __device__ __forceinline__ float sample(const uint32_t (&w)[NW], int s) {
  if constexpr (FMT == MIA_PCM_U8) {
    const int x = (int)((w[s >> 2] >> (8 * (s & 3))) & 0xffu);
    return (float)(x - 128) * 0.0078125f;  // exact
  } else if constexpr (FMT == MIA_PCM_S16) {
    const int x = (int)(int16_t)(uint16_t)(w[s >> 1] >> (16 * (s & 1)));
    return (float)x * 0x1p-15f;  // exact
  } else if constexpr (FMT == MIA_PCM_S24) {
    const int o = 3 * s, k = o >> 2, r = o & 3;
    // r <= 1: the three bytes lie in w[k]; r >= 2: they run into w[k + 1], which exists (o + 3 <= 4 NW)
    const uint64_t two = (uint64_t)w[k] | ((uint64_t)w[k + 1 < NW ? k + 1 : k] << 32);
    const int x = (int)((uint32_t)(two >> (8 * r)) << 8) >> 8;  // sign-extend 24 -> 32
    return (float)x * 0x1p-23f;  // exact
  } else if constexpr (FMT == MIA_PCM_S32) {
    return (float)(int)w[s] * 0x1p-31f;  // v_cvt_f32_i32 rounds to nearest even; the scaling is exact
  } else if constexpr (FMT == MIA_PCM_F32) {
    return __uint_as_float(w[s]);
  } else {
    const uint64_t b = (uint64_t)w[2 * s] | ((uint64_t)w[2 * s + 1] << 32);
    return (float)__builtin_bit_cast(double, b);  // v_cvt_f32_f64: nearest even, +-Inf above FLT_MAX
  }
}

// The NB bytes at src + a -> w, reading nothing outside src[0 .. len) (bytes outside read as 0).
template <int NB> __device__ __forceinline__ void fetch_span(const uint8_t* __restrict__ src, int64_t a, int64_t len,
                                                             uint32_t (&w)[NB / 4]) {
  constexpr int NW = NB / 4;
  const int r = (int)((reinterpret_cast<uintptr_t>(src) + (uintptr_t)a) & 3);
  if (a >= 0 && a + NB <= len && r == 0) {
    __builtin_memcpy(w, __builtin_assume_aligned(src + a, 4), NB);
    return;
  }
  const int64_t q0 = a - r;  // src + q0 is 4-B aligned
  uint32_t d[NW + 1];
#pragma unroll
  for (int k = 0; k <= NW; ++k) {
    const int64_t q = q0 + 4 * k;
    uint32_t v = 0;
    if (q >= 0 && q + 4 <= len) {
      v = *reinterpret_cast<const uint32_t*>(src + q);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (q + i >= 0 && q + i < len) v |= (uint32_t)src[q + i] << (8 * i);
    }
    d[k] = v;
  }
#pragma unroll
  for (int k = 0; k < NW; ++k) w[k] = (uint32_t)((((uint64_t)d[k + 1] << 32) | d[k]) >> (8 * r));
}

// folds a mono sample into the lane's running peak / non-finite count
__device__ __forceinline__ void fold_peak(float m, uint32_t& pk, uint32_t& nf) {
  const uint32_t a = __float_as_uint(m) & 0x7fffffffu;
  if (a < 0x7f800000u) pk = a > pk ? a : pk;
  else ++nf;
}

// Workgroup fold of (pk, nf) and one atomic each for clip i.  Every thread of the workgroup calls it.
__device__ __forceinline__ void publish_peak(uint32_t pk, uint32_t nf, uint32_t* __restrict__ peak_bits,
                                             uint32_t* __restrict__ nonfinite, int64_t i) {
  __shared__ uint32_t red[2 * (WG / 64)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t p2 = (uint32_t)__shfl_xor((int)pk, o, 64);
    pk = p2 > pk ? p2 : pk;
    nf += (uint32_t)__shfl_xor((int)nf, o, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave] = pk;
    red[WG / 64 + wave] = nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t p = 0, n = 0;
#pragma unroll
    for (int k = 0; k < WG / 64; ++k) {
      p = red[k] > p ? red[k] : p;
      n += red[WG / 64 + k];
    }
    if (p) atomicMax(&peak_bits[i], p);
    if (n) atomicAdd(&nonfinite[i], n);
  }
  __syncthreads();  // red is reused by the workgroup's next clip
}

// This workgroup's share of one clip: groups blockIdx.x * WG + threadIdx.x, + gridDim.x * WG, ...
template <int FMT, int C>
__device__ __forceinline__ void decode_clip(const uint8_t* __restrict__ src, int64_t frames, float* __restrict__ dst,
                                            uint32_t& pk, uint32_t& nf) {
  constexpr int BPS = bytes_per_sample(FMT), FB = C * BPS, NB = 4 * FB, NW = NB / 4;
  const int64_t len = frames * FB;  // the clip's bytes: src[0 .. len)
  const int shift = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);
  const int64_t groups = (frames + shift + 3) / 4;
  for (int64_t j = (int64_t)blockIdx.x * WG + threadIdx.x; j < groups; j += (int64_t)gridDim.x * WG) {
    const int64_t t0 = 4 * j - shift;  // >= -3
    uint32_t w[NW];
    fetch_span<NB>(src, t0 * FB, len, w);
    float m[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      float acc = sample<FMT, NW>(w, f * C);
#pragma unroll
      for (int c = 1; c < C; ++c) acc += sample<FMT, NW>(w, f * C + c);
      m[f] = C > 1 ? acc / (float)C : acc;
    }
    float* o = dst + t0;
    if (t0 >= 0 && t0 + 4 <= frames) {
      *reinterpret_cast<f32x4*>(o) = f32x4{m[0], m[1], m[2], m[3]};
#pragma unroll
      for (int f = 0; f < 4; ++f) fold_peak(m[f], pk, nf);
    } else {
#pragma unroll
      for (int f = 0; f < 4; ++f)
        if (t0 + f >= 0 && t0 + f < frames) {
          o[f] = m[f];
          fold_peak(m[f], pk, nf);
        }
    }
  }
}

template <int FMT>
__device__ __forceinline__ void decode_clip_c(int channels, const uint8_t* __restrict__ src, int64_t frames,
                                              float* __restrict__ dst, uint32_t& pk, uint32_t& nf) {
  switch (channels) {
    case 1: decode_clip<FMT, 1>(src, frames, dst, pk, nf); break;
    case 2: decode_clip<FMT, 2>(src, frames, dst, pk, nf); break;
    case 3: decode_clip<FMT, 3>(src, frames, dst, pk, nf); break;
    case 4: decode_clip<FMT, 4>(src, frames, dst, pk, nf); break;
    case 5: decode_clip<FMT, 5>(src, frames, dst, pk, nf); break;
    case 6: decode_clip<FMT, 6>(src, frames, dst, pk, nf); break;
    case 7: decode_clip<FMT, 7>(src, frames, dst, pk, nf); break;
    default: decode_clip<FMT, 8>(src, frames, dst, pk, nf); break;
  }
}

__global__ __launch_bounds__(WG) void pcm_decode_kernel(const uint8_t* __restrict__ bytes,
                                                        const MiaWavClip* __restrict__ clips, int64_t n_clips,
                                                        const int64_t* __restrict__ out_offsets,
                                                        float* __restrict__ out, uint32_t* __restrict__ peak_bits,
                                                        uint32_t* __restrict__ nonfinite) {
  for (int64_t i = blockIdx.y; i < n_clips; i += gridDim.y) {
    const MiaWavClip clip = clips[i];  // uniform over the workgroup, as is every branch on it below
    if (clip.channels < 1 || clip.channels > MIA_WAV_MAX_CHANNELS || clip.format < MIA_PCM_U8 ||
        clip.format > MIA_PCM_F64 || clip.frames <= 0)
      continue;
    if ((int64_t)blockIdx.x * WG * 4 >= clip.frames + 3) continue;  // no group of this clip is this workgroup's
    const uint8_t* src = bytes + clip.byte_off;
    float* dst = out + out_offsets[i];
    uint32_t pk = 0, nf = 0;
    switch (clip.format) {
      case MIA_PCM_U8: decode_clip_c<MIA_PCM_U8>(clip.channels, src, clip.frames, dst, pk, nf); break;
      case MIA_PCM_S16: decode_clip_c<MIA_PCM_S16>(clip.channels, src, clip.frames, dst, pk, nf); break;
      case MIA_PCM_S24: decode_clip_c<MIA_PCM_S24>(clip.channels, src, clip.frames, dst, pk, nf); break;
      case MIA_PCM_S32: decode_clip_c<MIA_PCM_S32>(clip.channels, src, clip.frames, dst, pk, nf); break;
      case MIA_PCM_F32: decode_clip_c<MIA_PCM_F32>(clip.channels, src, clip.frames, dst, pk, nf); break;
      default: decode_clip_c<MIA_PCM_F64>(clip.channels, src, clip.frames, dst, pk, nf); break;
    }
    publish_peak(pk, nf, peak_bits, nonfinite, i);
  }
}

// The 16-B groups of store[offsets[i] .. offsets[i+1]) that are this workgroup's: f(element pointer of the group,
// first valid k, one past the last valid k); a whole group has k0 = 0, k1 = 4 and an aligned pointer.
template <typename F> __device__ __forceinline__ void walk_groups(float* base, int64_t len, F f) {
  const int shift = (int)((reinterpret_cast<uintptr_t>(base) >> 2) & 3);
  const int64_t groups = (len + shift + 3) / 4;
  for (int64_t j = (int64_t)blockIdx.x * WG + threadIdx.x; j < groups; j += (int64_t)gridDim.x * WG) {
    const int64_t t0 = 4 * j - shift;
    const int k0 = t0 < 0 ? (int)-t0 : 0;
    const int k1 = t0 + 4 <= len ? 4 : (int)(len - t0);
    f(base + t0, k0, k1);
  }
}

__global__ __launch_bounds__(WG) void clip_peak_kernel(const float* __restrict__ store,
                                                       const int64_t* __restrict__ offsets, int64_t n_clips,
                                                       uint32_t* __restrict__ peak_bits,
                                                       uint32_t* __restrict__ nonfinite) {
  for (int64_t i = blockIdx.y; i < n_clips; i += gridDim.y) {
    const int64_t b = offsets[i], len = offsets[i + 1] - b;
    if (len <= 0 || (int64_t)blockIdx.x * WG * 4 >= len + 3) continue;
    uint32_t pk = 0, nf = 0;
    walk_groups(const_cast<float*>(store) + b, len, [&](float* p, int k0, int k1) {
      if (k0 == 0 && k1 == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        fold_peak(v.x, pk, nf);
        fold_peak(v.y, pk, nf);
        fold_peak(v.z, pk, nf);
        fold_peak(v.w, pk, nf);
      } else {
        for (int k = k0; k < k1; ++k) fold_peak(p[k], pk, nf);
      }
    });
    publish_peak(pk, nf, peak_bits, nonfinite, i);
  }
}

__global__ __launch_bounds__(WG) void clip_scale_kernel(float* __restrict__ store,
                                                        const int64_t* __restrict__ offsets, int64_t n_clips,
                                                        const uint32_t* __restrict__ peak_bits) {
  for (int64_t i = blockIdx.y; i < n_clips; i += gridDim.y) {
    const int64_t b = offsets[i], len = offsets[i + 1] - b;
    const float peak = __uint_as_float(peak_bits[i]);
    if (len <= 0 || !(peak > 0.0f)) continue;  // a silent clip stays as it is
    walk_groups(store + b, len, [&](float* p, int k0, int k1) {
      if (k0 == 0 && k1 == 4) {
        f32x4 v = *reinterpret_cast<const f32x4*>(p);
        v.x /= peak;
        v.y /= peak;
        v.z /= peak;
        v.w /= peak;
        *reinterpret_cast<f32x4*>(p) = v;
      } else {
        for (int k = k0; k < k1; ++k) p[k] /= peak;
      }
    });
  }
}

// peak_bits and nonfinite start from 0: one small launch ahead of the fold (two hipMemsetAsync calls of a few
// hundred bytes cost more than the decode of a small group)
__global__ __launch_bounds__(WG) void zero_pair_kernel(uint32_t* a, uint32_t* b, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * WG + threadIdx.x;
  if (i < n) {
    a[i] = 0u;
    b[i] = 0u;
  }
}

// (chunks of 1024 samples per clip walked by grid-stride) x (clips): enough workgroups to fill the chip whatever
// the clip count, without the launcher knowing the clip lengths (they live on the device)
dim3 clip_grid(int64_t n_clips) {
  const int64_t per_clip = std::min<int64_t>(1024, std::max<int64_t>(1, cdiv(8192, n_clips)));
  return dim3((unsigned)per_clip, (unsigned)std::min<int64_t>(n_clips, 65535));
}

}  // namespace

extern "C" int mia_pcm_decode(const uint8_t* bytes, const MiaWavClip* clips, int64_t n_clips,
                              const int64_t* out_offsets, float* out, uint32_t* peak_bits, uint32_t* nonfinite,
                              mia_stream_t stream) {
  MIA_CHECK_ARG(n_clips >= 0, "pcm_decode: n_clips %lld < 0", (long long)n_clips);
  if (n_clips == 0) return 0;
  MIA_CHECK_ARG(bytes && clips && out_offsets && out && peak_bits && nonfinite, "pcm_decode: null pointer");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & 3) == 0 && (reinterpret_cast<uintptr_t>(clips) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(out_offsets) & 7) == 0,
                "pcm_decode: out must be 4-B aligned, clips and out_offsets 8-B aligned");
  zero_pair_kernel<<<(unsigned)cdiv(n_clips, WG), WG, 0, as_stream(stream)>>>(peak_bits, nonfinite, n_clips);
  pcm_decode_kernel<<<clip_grid(n_clips), WG, 0, as_stream(stream)>>>(bytes, clips, n_clips, out_offsets, out,
                                                                      peak_bits, nonfinite);
  MIA_LAUNCH_CHECK("pcm_decode");
  return 0;
}

extern "C" int mia_clip_peak(const float* store, const int64_t* offsets, int64_t n_clips, uint32_t* peak_bits,
                             uint32_t* nonfinite, mia_stream_t stream) {
  MIA_CHECK_ARG(n_clips >= 0, "clip_peak: n_clips %lld < 0", (long long)n_clips);
  if (n_clips == 0) return 0;
  MIA_CHECK_ARG(store && offsets && peak_bits && nonfinite, "clip_peak: null pointer");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(store) & 3) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0,
                "clip_peak: store must be 4-B aligned, offsets 8-B aligned");
  zero_pair_kernel<<<(unsigned)cdiv(n_clips, WG), WG, 0, as_stream(stream)>>>(peak_bits, nonfinite, n_clips);
  clip_peak_kernel<<<clip_grid(n_clips), WG, 0, as_stream(stream)>>>(store, offsets, n_clips, peak_bits, nonfinite);
  MIA_LAUNCH_CHECK("clip_peak");
  return 0;
}

extern "C" int mia_clip_scale(float* store, const int64_t* offsets, int64_t n_clips, const uint32_t* peak_bits,
                              mia_stream_t stream) {
  MIA_CHECK_ARG(n_clips >= 0, "clip_scale: n_clips %lld < 0", (long long)n_clips);
  if (n_clips == 0) return 0;
  MIA_CHECK_ARG(store && offsets && peak_bits, "clip_scale: null pointer");
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(store) & 3) == 0 && (reinterpret_cast<uintptr_t>(offsets) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(peak_bits) & 3) == 0,
                "clip_scale: store and peak_bits must be 4-B aligned, offsets 8-B aligned");
  clip_scale_kernel<<<clip_grid(n_clips), WG, 0, as_stream(stream)>>>(store, offsets, n_clips, peak_bits);
  MIA_LAUNCH_CHECK("clip_scale");
  return 0;
}
