// Weight gradient of the EnvNet-v2 trunk 8x8 conv (reference src/models/envnet_v2.py:34
// Conv2d(32, 32, (8, 8)), input = relu(bn(previous conv)) ), bf16 MFMA, gfx950.
//
//   dW[co][ky][kx][ci] = sum_{b, oy, ox} dY[b][oy][ox][co] * relu(bn(x))[b][oy+ky][ox+kx][ci]
//
// Rolling-window schedule: a block owns (clip, 128-column chunk) items and walks the output rows
// of an item top to bottom.  The 8 input rows an output row needs stay in a 9-slot LDS ring, so
// every input row is staged (and BN+ReLU'd) ONCE per item instead of once per kernel row, and
// every dY row once: HBM reads ~ x + dY instead of ~8x + 2 dY for a ky-partitioned grid.
// Wave w owns kernel row ky = w: its 8 accumulator tiles are dW[:, w, kx, :] (32 co x 32 ci) for
// kx = 0..7 (128 registers), kept across all items; each block writes one f32 slab and the
// split-K reducer sums the slabs.  Operands are transposed LDS reads (ds_read_b64_tr_b16) of the
// [px][32 ch] images, exactly as the row-window wgrad kernel.  Rows for step s+1 are loaded raw
// into registers while step s computes (issue early, convert + write late).
#include "bn_math.h"
#include "gemm_common.h"

namespace mgemm {

// bf16 NHWC x (n, oh+7, ow+7, 32) raw, dy (n, oh, ow, 32); writes nblk f32 slabs ws[nblk][32][2048] (OHWI
// columns) for the split-K reducer.
struct W8Args {
  const bf16* x;
  const bf16* dy;
  const float* ps;
  const float* pt;
  int n, h, w, oh, ow;
  int nblk;
  float* ws;
};

namespace {

constexpr int W8_NT = 512;
constexpr int W8_BP = 128;                  // output columns per item
constexpr int W8_WPX = W8_BP + 7;           // staged input columns
constexpr int W8_XROW = W8_WPX * 64;        // bytes per staged input row (32 ch bf16)
constexpr int W8_RING = 9;                  // 8 rows in use + the one being written
constexpr int W8_DROW = W8_BP * 64;         // bytes per staged dY row
constexpr int W8_XCH = (W8_WPX * 4 + W8_NT - 1) / W8_NT;  // 16-B chunks per thread per input row (2)

typedef short s16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 tr_frag(const char* p0, int stride) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((MIA_LDS s16x4*)(p0 + 4 * stride));
  const s16x8 c = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, c);
}

__global__ __launch_bounds__(W8_NT) void wgrad8_kernel(W8Args g) {
  __shared__ __attribute__((aligned(16))) char smem[W8_RING * W8_XROW + 2 * W8_DROW];
  char* ring = smem;
  char* dys = smem + W8_RING * W8_XROW;
  const int t = threadIdx.x, lane = t & 63;
  const int ky = __builtin_amdgcn_readfirstlane(t >> 6);
  const int i16 = lane & 15, gq = lane >> 4;
  const int cg = t & 3;  // this thread's 8-channel group in every staged 16-B chunk
  BnFwd8 bn;
  bn.load(cg, g.ps, g.pt);

  f32x16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  const int nchunk = (g.ow + W8_BP - 1) / W8_BP;
  const int items = g.n * nchunk;
  u32x4 xr[W8_XCH], dr;
  uint32_t xok = 0;
  bool dok = false;
  const u32x4* xs = reinterpret_cast<const u32x4*>(g.x);
  const u32x4* ds = reinterpret_cast<const u32x4*>(g.dy);

  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int b = item / nchunk;
    const int x0 = (item - b * nchunk) * W8_BP;
    // raw loads of input row iy / dY row oy (16-B chunk = 8 channels), unconditional addresses
    auto load_x = [&](int iy) __attribute__((always_inline)) {
      xok = 0;
#pragma unroll
      for (int i = 0; i < W8_XCH; ++i) {
        const int q = t + W8_NT * i;
        const int px = x0 + (q >> 2);
        const bool ok = (q >> 2) < W8_WPX && px < g.w && iy < g.h;
        const int64_t off = ok ? ((((int64_t)b * g.h + iy) * g.w + px) * 4 + (q & 3)) : 0;
        xr[i] = xs[off];
        xok |= (uint32_t)ok << i;
      }
    };
    auto load_dy = [&](int oy) __attribute__((always_inline)) {
      const int px = x0 + (t >> 2);
      dok = oy >= 0 && oy < g.oh && px < g.ow;
      const int64_t off = dok ? ((((int64_t)b * g.oh + oy) * g.ow + px) * 4 + (t & 3)) : 0;
      dr = ds[off];
    };
    auto store_x = [&](int slot) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < W8_XCH; ++i) {
        const int q = t + W8_NT * i;
        if ((q >> 2) < W8_WPX)
          *reinterpret_cast<u32x4*>(ring + slot * W8_XROW + q * 16) = (xok >> i) & 1u ? bn_relu_pack(xr[i], bn.sc, bn.sh) : u32x4{0u, 0u, 0u, 0u};
      }
    };
    auto store_dy = [&](int buf) __attribute__((always_inline)) {
      *reinterpret_cast<u32x4*>(dys + buf * W8_DROW + t * 16) = dok ? dr : u32x4{0u, 0u, 0u, 0u};
    };

    load_x(0);
    store_x(0);
    __syncthreads();
    for (int s = 0; s < g.h; ++s) {
      // stage s+1 in flight while step s computes
      load_x(s + 1);
      load_dy(s - 6);
      const int oy = s - 7;
      if (oy >= 0) {
        const char* xrow = ring + ((oy + ky) % W8_RING) * W8_XROW;
        const char* drow = dys + (oy & 1) * W8_DROW;
#pragma unroll
        for (int ks = 0; ks < W8_BP / 16; ++ks) {
          const int kr = ks * 16 + 8 * (gq >> 1) + (i16 >> 2);
          const int c4 = 16 * (gq & 1) + 4 * (i16 & 3);
          const bf16x8 fa = tr_frag(drow + kr * 64 + c4 * 2, 64);
#pragma unroll
          for (int kx = 0; kx < 8; ++kx) {
            const bf16x8 fb = tr_frag(xrow + (kr + kx) * 64 + c4 * 2, 64);
            acc[kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[kx], 0, 0, 0);
          }
        }
      }
      if (s + 1 < g.h) store_x((s + 1) % W8_RING);
      if (s - 6 >= 0 && s - 6 < g.oh) store_dy((s - 6) & 1);
      __syncthreads();
    }
  }

  // slab: ws[block][co][ky*256 + kx*32 + ci]
  float* dst = g.ws + (int64_t)blockIdx.x * 32 * 2048 + ky * 256;
#pragma unroll
  for (int kx = 0; kx < 8; ++kx)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      dst[(int64_t)co * 2048 + kx * 32 + (lane & 31)] = acc[kx][r];
    }
}

}  // namespace

// Among the GEMMs the row-window weight gradient takes (rowwgrad_ok): the trunk conv4 shape this kernel is for
bool wgrad8_ok(const MiaOperand& A, const MiaOperand& B, int64_t M) {
  return A.dtype == MIA_BF16 && M == 32 && B.c == 32 && B.kh == 8 && B.kw == 8 && B.sw == 1 && B.ph == 0 &&
         B.pw == 0 && B.pre == MIA_PRE_AFFINE_RELU && B.h == B.oh + 7 && B.w == B.ow + 7;
}

// rolling 8-row window per (clip, column chunk), one slab per block
int wgrad8_run(const MiaOperand& A, const MiaOperand& B, const MiaEpilogue& E, int64_t M, int64_t N, int split,
               void* workspace, hipStream_t s) {
  W8Args w8;
  w8.x = reinterpret_cast<const bf16*>(B.ptr);
  w8.dy = reinterpret_cast<const bf16*>(A.ptr);
  w8.ps = B.pre_scale; w8.pt = B.pre_shift;
  w8.n = B.n; w8.h = B.h; w8.w = B.w; w8.oh = B.oh; w8.ow = B.ow;
  const int64_t items = (int64_t)B.n * cdiv(B.ow, 128);
  w8.nblk = (int)std::min<int64_t>(std::min<int64_t>(split, 256), items);
  w8.ws = reinterpret_cast<float*>(workspace);
  wgrad8_kernel<<<w8.nblk, W8_NT, 0, s>>>(w8);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return mia::fail(-(int)err, "wgrad8 launch: %s", hipGetErrorString(err));
  launch_splitk_reduce(w8.ws, w8.nblk, M, N, to_dev(E), s);
  MIA_LAUNCH_CHECK("splitk_reduce");
  return 0;
}

}  // namespace mgemm
