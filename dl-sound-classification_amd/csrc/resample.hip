// Band-limited sinc resampling of a waveform batch (include/miaudio_resample.h): the strided FIR bank of
// torchaudio.transforms.Resample as one f32 GEMM per clip,
//   out[f * n + j] = sum_k X[f][k] * taps[j][k],   X[f][k] = xz[f * o + k - width]   (f = frame, j = phase),
// on v_mfma_f32_32x32x2_f32 (exact f32 products and sums at the vector unit's peak rate, one VGPR per operand).
//
// A workgroup (4 waves) owns 128 frames x up to 160 phases of one clip and walks the K taps in chunks of 32:
//  * the chunk of X is gathered straight from the clip while it is staged -- row f is 32 consecutive samples at
//    f * o + k0 - width, zero outside [0, L_b) -- so the Toeplitz operand never exists in memory and no x segment
//    (28 K floats for 64 frames of 441 -> 160) has to fit in LDS; the taps table (300 KB for the two shipped pairs)
//    is tiled the same way, over phases as well as over k;
//  * both chunks sit in LDS as [128][33] f32: an MFMA operand read is lane (row = l & 31, k = l >> 5) -> bank
//    (33 * row + k) % 32, conflict-free whatever o is (a segment image read at stride o words would put all 32
//    rows of o = 160 in one bank);
//  * wave w multiplies frames 32 w .. 32 w + 31 by the workgroup's 1..5 phase tiles of 32: one A read and up to
//    five B reads per five 64-cycle MFMAs, five independent accumulators;
//  * the next chunk's global loads are issued into registers before the MFMAs of the current one and written to
//    the other LDS buffer after them: one barrier per chunk.
// Sums run over k ascending in one accumulator per output: a fixed order, the same bits on every run.
// Phases n < 32 (44.1 -> 22.05 kHz and back: n = 1, 2) fill only n of a tile's 32 columns; those pairs have K <= 28
// and stay far below a millisecond for a 64-clip launch, so they share this kernel.
#include "common.h"

#include "../../include/miaudio_resample.h"

namespace {

constexpr int RS_FT = 128;  // frames per workgroup (32 per wave)
constexpr int RS_NT = 5;    // MFMA column tiles of 32 phases per workgroup: 160 phases (n = 160 whole, 441 as 5 + 5 + 4)
constexpr int RS_PT = 32 * RS_NT;
constexpr int RS_KC = 32;   // taps per staged chunk
constexpr int RS_LD = RS_KC + 1;
constexpr int RS_AI = RS_FT / 8, RS_BI = RS_PT / 8;  // rows a staging thread owns in the A / B chunk

__global__ __launch_bounds__(256, 2) void resample_kernel(const float* __restrict__ x, int64_t ldx, int64_t T,
                                                          const int32_t* __restrict__ lengths,
                                                          const float* __restrict__ taps, int o, int n, int width,
                                                          int K, float* __restrict__ out, int64_t ldo, int64_t Tout) {
  __shared__ float As[2][RS_FT * RS_LD];  // double-buffered: one barrier per chunk
  __shared__ float Bs[2][RS_PT * RS_LD];
  const int b = blockIdx.z;
  int64_t L = T;
  if (lengths) {
    const int64_t v = lengths[b];
    L = v < 0 ? 0 : (v > T ? T : v);
  }
  const int64_t olen = ((int64_t)n * L + o - 1) / o;  // the clip's own output length; +0.0f behind it
  const int64_t f0 = (int64_t)blockIdx.x * RS_FT;
  const int p0 = blockIdx.y * RS_PT;
  const int left = (n - p0 + 31) / 32;
  const int ncol = left < RS_NT ? left : RS_NT;  // phase tiles of 32 this workgroup owns
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 31, lk = lane >> 5;
  const float* __restrict__ xb = x + (int64_t)b * ldx;
  float* __restrict__ ob = out + (int64_t)b * ldo;

  f32x16 acc[RS_NT];
#pragma unroll
  for (int t = 0; t < RS_NT; ++t)
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[t][v] = 0.f;

  if (f0 * n < olen) {  // else the whole tile lies in the zero tail (a clip shorter than the launch's longest)
    const int c = tid & 31, r0 = tid >> 5;  // staging: thread -> column c of rows r0, r0 + 8, ...
    const int64_t x0 = (f0 + r0) * o + c - width, xstep = 8 * (int64_t)o;  // row i of the chunk at k0: x0 + k0 + i * xstep
    const int64_t t0 = (int64_t)(p0 + r0) * K + c, tstep = 8 * (int64_t)K;
    float ra[RS_AI], rb[RS_BI];
    auto gload = [&](int k0) {
      const bool kin = k0 + c < K;
#pragma unroll
      for (int i = 0; i < RS_AI; ++i) {
        const int64_t idx = x0 + k0 + i * xstep;
        ra[i] = (kin && idx >= 0 && idx < L) ? xb[idx] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < RS_BI; ++i)
        rb[i] = (kin && i < 4 * ncol && p0 + r0 + 8 * i < n) ? taps[t0 + k0 + i * tstep] : 0.f;
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int i = 0; i < RS_AI; ++i) As[buf][(r0 + 8 * i) * RS_LD + c] = ra[i];
#pragma unroll
      for (int i = 0; i < RS_BI; ++i) Bs[buf][(r0 + 8 * i) * RS_LD + c] = rb[i];
    };
    gload(0);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < K; k0 += RS_KC, buf ^= 1) {
      const bool more = k0 + RS_KC < K;
      if (more) gload(k0 + RS_KC);  // in flight under this chunk's MFMAs
      const float* a_row = As[buf] + (32 * w + li) * RS_LD + lk;
      const float* b_row = Bs[buf] + li * RS_LD + lk;
#pragma unroll
      for (int ks = 0; ks < RS_KC / 2; ++ks) {
        const float a = a_row[2 * ks];
#pragma unroll
        for (int t = 0; t < RS_NT; ++t)
          if (t < ncol) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b_row[32 * t * RS_LD + 2 * ks], acc[t], 0, 0, 0);
      }
      // the other buffer was last read in the previous iteration, which every wave left through the barrier below
      if (more) stage(buf ^ 1);
      __syncthreads();
    }
  }

  // C/D map of the 32x32 MFMA: column = lane & 31 (phase), row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5) (frame)
#pragma unroll
  for (int t = 0; t < RS_NT; ++t) {
    const int j = p0 + 32 * t + li;
    if (t < ncol && j < n) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int64_t f = f0 + 32 * w + (v & 3) + 8 * (v >> 2) + 4 * lk;
        const int64_t m = f * n + j;
        if (m < Tout) ob[m] = m < olen ? acc[t][v] : 0.f;
      }
    }
  }
}

int64_t gcd64(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int64_t mia_resample_out_len(int64_t T, int32_t o, int32_t n) {
  if (T < 0 || o < 1 || n < 1) return -22;
  return (T * n + o - 1) / o;
}

extern "C" int mia_resample(const float* x, int64_t ldx, int32_t B, int64_t T, const int32_t* lengths,
                            const float* taps, int32_t o, int32_t n, int32_t width, float* out, int64_t ldo,
                            int64_t Tout, mia_stream_t stream) {
  MIA_CHECK_ARG(o >= 1 && n >= 1 && width >= 0, "resample: o %d, n %d, width %d", o, n, width);
  MIA_CHECK_ARG(gcd64(o, n) == 1, "resample: o %d and n %d are not coprime", o, n);
  const int64_t K = 2 * (int64_t)width + o;
  MIA_CHECK_ARG(K <= MIA_RESAMPLE_MAX_TAPS && n <= MIA_RESAMPLE_MAX_PHASES,
                "resample: K %lld, n %d over the limits %d, %d", (long long)K, n, MIA_RESAMPLE_MAX_TAPS,
                MIA_RESAMPLE_MAX_PHASES);
  MIA_CHECK_ARG(B >= 0 && B <= MIA_RESAMPLE_MAX_BATCH && T >= 0 && T <= (INT64_MAX >> 13), "resample: B %d, T %lld", B,
                (long long)T);
  MIA_CHECK_ARG(Tout == mia_resample_out_len(T, o, n), "resample: Tout %lld, expected %lld", (long long)Tout,
                (long long)mia_resample_out_len(T, o, n));
  MIA_CHECK_ARG(ldx >= T && ldo >= Tout, "resample: ldx %lld < T or ldo %lld < Tout", (long long)ldx, (long long)ldo);
  if (B == 0 || Tout == 0) return 0;
  MIA_CHECK_ARG(x && taps && out, "resample: null");
  const int64_t frames = cdiv(Tout, n);
  const int64_t gx = cdiv(frames, RS_FT);
  MIA_CHECK_ARG(gx <= 0x7fffffff, "resample: %lld frame tiles", (long long)gx);
  const dim3 grid((unsigned)gx, (unsigned)cdiv(n, RS_PT), (unsigned)B);
  resample_kernel<<<grid, 256, 0, as_stream(stream)>>>(x, ldx, T, lengths, taps, o, n, width, (int)K, out, ldo, Tout);
  MIA_LAUNCH_CHECK("resample");
  return 0;
}
