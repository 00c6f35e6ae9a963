// Pad-and-crop gather from a device-resident clip store (include/miaudio_data.h):
//   out[c][b][t] = clip_{idx[b]}[start[b][c] + t - pad]  inside the clip,  +0.0f outside.
// A plain copy: 4 B read + 4 B written per output sample, no arithmetic on the samples (moved as 32-bit words, so
// NaN payloads and -0.0 survive).
//
// One thread owns one 16-B group of an output row.  Groups are cut on the row's ADDRESS, not on its index: with
// shift = (element address of the row's first sample) & 3, group j holds t = 4 j - shift .. 4 j - shift + 3, so
// every group that lies whole inside the row is one aligned 16-B store whatever window % 4 and the out pointer are;
// the at most two groups that overhang the row's ends (its misaligned head and tail) store element by element.
// The source side is misaligned against the groups in general (clip bases and crop starts are arbitrary): a lane
// reads four consecutive words and a wave 1 KB of consecutive addresses, which the memory pipeline coalesces by
// cache line.  Every load is guarded by 0 <= s < len of its own clip: no address is formed from an unchecked start.
//
// mia_fit_gather (clip-length fitting for the spectrogram path) is the same copy with another source index; see
// fit_gather_kernel below.
#include "common.h"

#include "../../include/miaudio_data.h"

namespace {


__global__ __launch_bounds__(256) void crop_gather_kernel(const uint32_t* __restrict__ store,
                                                          const int64_t* __restrict__ offsets, int64_t n_clips,
                                                          const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ start, int32_t B, int32_t ncrop,
                                                          int32_t pad, int32_t window, uint32_t* __restrict__ out) {
  const int64_t rows = (int64_t)B * ncrop;
  const int64_t out_elem = (int64_t)(reinterpret_cast<uintptr_t>(out) >> 2);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {  // row = c * B + b
    const int32_t c = (int32_t)(row / B), b = (int32_t)(row - (int64_t)c * B);
    const int64_t row0 = row * window;
    const int32_t shift = (int32_t)((out_elem + row0) & 3);
    const int64_t t0 = 4 * j - shift;
    if (t0 >= window) continue;
    const int64_t i = idx[b];
    int64_t base = 0, len = 0;
    if (i >= 0 && i < n_clips) {
      base = offsets[i];
      len = offsets[i + 1] - base;
    }
    const int64_t s0 = (int64_t)start[(int64_t)b * ncrop + c] + t0 - pad;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t t = t0 + k, s = s0 + k;
      v[k] = (t >= 0 && t < window && s >= 0 && s < len) ? store[base + s] : 0u;
    }
    uint32_t* o = out + row0 + t0;
    if (t0 >= 0 && t0 + 4 <= window) {
      *reinterpret_cast<u32x4*>(o) = u32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t0 + k >= 0 && t0 + k < window) o[k] = v[k];
    }
  }
}

// Clip-length fitting (mia_fit_gather): the output side above, another source index.  Per row, with n the clip's
// length: n >= length reads s = (n - length) / 2 + t (the centred trim; start 0 when n == length), MIA_FIT_ZERO on a
// shorter clip reads s = t and fails the s < n guard past the clip, MIA_FIT_WRAP reads s = t mod n.  Wrapping only
// occurs with n < length <= INT32_MAX, so the remainder is one 32-bit division per thread, for the first sample of
// its group that lies in the row; the other three step it with a compare and reset.  The read runs break at wrap
// points (a group may span one, or several when n < 4); every load is still guarded by 0 <= s < n.
__global__ __launch_bounds__(256) void fit_gather_kernel(const uint32_t* __restrict__ store,
                                                         const int64_t* __restrict__ offsets, int64_t n_clips,
                                                         const int32_t* __restrict__ idx, int32_t B, int32_t length,
                                                         int32_t mode, uint32_t* __restrict__ out) {
  const int64_t out_elem = (int64_t)(reinterpret_cast<uintptr_t>(out) >> 2);
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (int64_t row = blockIdx.y; row < B; row += gridDim.y) {
    const int64_t row0 = row * length;
    const int32_t shift = (int32_t)((out_elem + row0) & 3);
    const int64_t t0 = 4 * j - shift;
    if (t0 >= length) continue;
    const int64_t i = idx[row];
    int64_t base = 0, len = 0;
    if (i >= 0 && i < n_clips) {
      base = offsets[i];
      len = offsets[i + 1] - base;
    }
    const bool wrap = mode == MIA_FIT_WRAP && len > 0 && len < length;
    int64_t s;
    if (wrap) {
      const int32_t tf = t0 < 0 ? 0 : (int32_t)t0;  // the group's first sample inside the row
      s = (int64_t)((uint32_t)tf % (uint32_t)len) - (tf - t0);
    } else {
      s = (len > length ? (len - length) >> 1 : 0) + t0;
    }
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t t = t0 + k;
      v[k] = (t >= 0 && t < length && s >= 0 && s < len) ? store[base + s] : 0u;
      ++s;
      if (wrap && s == len) s = 0;
    }
    uint32_t* o = out + row0 + t0;
    if (t0 >= 0 && t0 + 4 <= length) {
      *reinterpret_cast<u32x4*>(o) = u32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (t0 + k >= 0 && t0 + k < length) o[k] = v[k];
    }
  }
}

}  // namespace

extern "C" int mia_fit_gather(const float* store, const int64_t* offsets, int64_t n_clips, const int32_t* idx,
                              int32_t B, int32_t length, int32_t mode, float* out, mia_stream_t stream) {
  MIA_CHECK_ARG(store && offsets && idx && out, "fit_gather: null pointer");
  MIA_CHECK_ARG(B >= 1 && length >= 1, "fit_gather: B %d, length %d must be >= 1", B, length);
  MIA_CHECK_ARG(n_clips >= 1, "fit_gather: n_clips %lld < 1", (long long)n_clips);
  MIA_CHECK_ARG(mode == MIA_FIT_WRAP || mode == MIA_FIT_ZERO, "fit_gather: mode %d is neither MIA_FIT_WRAP nor "
                "MIA_FIT_ZERO", mode);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(store) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "fit_gather: store and out must be 4-B aligned");
  const int64_t groups = ((int64_t)length + 3 + 3) / 4;  // a row misaligned by 3 elements
  const dim3 grid((unsigned)cdiv(groups, 256), (unsigned)std::min<int32_t>(B, 65535));
  fit_gather_kernel<<<grid, 256, 0, as_stream(stream)>>>(reinterpret_cast<const uint32_t*>(store), offsets, n_clips,
                                                         idx, B, length, mode, reinterpret_cast<uint32_t*>(out));
  MIA_LAUNCH_CHECK("fit_gather");
  return 0;
}

extern "C" int mia_crop_gather(const float* store, const int64_t* offsets, int64_t n_clips, const int32_t* idx,
                               const int32_t* start, int32_t B, int32_t ncrop, int32_t pad, int32_t window,
                               float* out, mia_stream_t stream) {
  MIA_CHECK_ARG(store && offsets && idx && start && out, "crop_gather: null pointer");
  MIA_CHECK_ARG(B >= 1 && ncrop >= 1 && window >= 1, "crop_gather: B %d, ncrop %d, window %d must be >= 1", B, ncrop,
                window);
  MIA_CHECK_ARG(pad >= 0 && n_clips >= 1, "crop_gather: pad %d < 0 or n_clips %lld < 1", pad, (long long)n_clips);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(store) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                "crop_gather: store and out must be 4-B aligned");
  const int64_t groups = ((int64_t)window + 3 + 3) / 4;  // a row misaligned by 3 elements
  const int64_t rows = (int64_t)B * ncrop;
  const dim3 grid((unsigned)cdiv(groups, 256), (unsigned)std::min<int64_t>(rows, 65535));
  crop_gather_kernel<<<grid, 256, 0, as_stream(stream)>>>(reinterpret_cast<const uint32_t*>(store), offsets, n_clips,
                                                          idx, start, B, ncrop, pad, window,
                                                          reinterpret_cast<uint32_t*>(out));
  MIA_LAUNCH_CHECK("crop_gather");
  return 0;
}
