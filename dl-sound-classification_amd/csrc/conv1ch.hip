// Backward-data of the single-input-channel 8x8 conv (EnvNet-v2 trunk conv3, reference
// src/models/envnet_v2.py:31 Conv2d(1, 32, (8, 8))), bf16 MFMA, gfx950.
//
//   dx[b][y][x] = sum_{ky,kx,co} dy[b][y-ky][x-kx][co] * w[co][0][ky][kx]
//
// With one input channel the contraction has no output-channel axis to put on the MFMA N side, so
// the kernel puts the kernel row ky there instead: for one staged dY row r,
//   Q_r[x][ky] = sum_{kx,co} dy[b][r][x-kx][co] * w[co][ky][kx]        (M = x, N = ky, K = (kx, co) = 256)
// and dx[b][r+ky][x] += Q_r[x][ky].  A block owns one clip and 128 output columns and sweeps every
// dY row once (each dY byte is read from HBM once); the 64 output rows x 128 columns accumulate in
// LDS (f32, one writer per address, program order => deterministic; rows 129 floats apart so a dY row's
// scatter into its 8 output rows is conflict-free: at 128 it was 8-way, 0.48 of the kernel's LDS cycles
// in SQ_LDS_BANK_CONFLICT) and are stored once as bf16.
// dY rows are register-staged two rows ahead (issue early, write late) into a 2-deep LDS ring whose
// pixel stride (80 B) makes every 16-lane ds_read_b128 group conflict-free.  N = 8 of the MFMA's 32
// columns carry data: the op is 58 GFLOP/step of real work, HBM-bound on the dY read either way.
#include <cstdlib>

#include "common.h"

namespace {

constexpr int C1_C = 32, C1_K = 8;
constexpr int C1_BW = 128;                 // output columns per block
constexpr int C1_SLOTS = C1_BW + C1_K - 1; // staged dY pixels per row
constexpr int C1_PSB = 80;                 // LDS bytes per staged pixel (64 B data + 16 B skew)
constexpr int C1_HMAX = 64;                // output rows held in LDS
// output row stride in LDS: 129 floats, so the 8 kernel rows ky a dY row scatters into (lanes 0-7 of a
// half wave, same column) fall on 8 different banks (a 128-float stride put all 8 on one bank: 8-way)
constexpr int C1_OLD = C1_BW + 1;
constexpr int C1_LD = (C1_SLOTS * 4 + 255) / 256;  // 16-B chunks per thread per row (3)

struct C1Args {
  const bf16* dy;
  const float* w;
  bf16* dx;
  int n, oh, ow, h, wd, nchunk;
};

// the MIA_C1CH_V1 form (an oracle of the bit-identical forms tests: its text stays written out and off the shared headers)
__global__ __launch_bounds__(256) void conv1ch_dgrad_kernel(C1Args g) {
  __shared__ __attribute__((aligned(16))) char rows[2][C1_SLOTS * C1_PSB];
  __shared__ __attribute__((aligned(16))) float outs[C1_HMAX * C1_OLD];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x / g.nchunk;
  const int w0 = (blockIdx.x - b * g.nchunk) * C1_BW;

  for (int i = t; i < C1_HMAX * C1_OLD; i += 256) outs[i] = 0.f;

  // B fragments (whole K = 256 in registers): lane column n = ky, k = 16 ks + 8 (lane >> 5) + j
  // with kx = ks >> 1, co = 16 (ks & 1) + 8 (lane >> 5) + j.
  bf16x8 bw[16];
  const int ky = lane & 31;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const int kx = ks >> 1, co0 = 16 * (ks & 1) + 8 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      bw[ks][j] = ky < C1_K ? (bf16)g.w[((co0 + j) * C1_K + ky) * C1_K + kx] : (bf16)0.f;
  }

  // thread slot q -> (staged pixel s, 16-B chunk c): each 8-lane group of a ds_write_b128 takes the 4
  // chunks of pixels p and p + 4 (80 B x 4 = 320 B = 16 banks apart: conflict-free; pixels p, p + 1 were
  // 2-way), a wave still loads 16 consecutive pixels
  auto slot_of = [](int q, int& s, int& c) __attribute__((always_inline)) {
    const int gq = q >> 3, j = q & 7;
    s = (gq >> 2) * 8 + (gq & 3) + 4 * (j >> 2);
    c = j & 3;
  };
  const bf16* dyb = g.dy + (int64_t)b * g.oh * g.ow * C1_C;
  auto load_row = [&](int r, uint4 (&reg)[C1_LD]) __attribute__((always_inline)) {
    const bf16* src = dyb + (int64_t)r * g.ow * C1_C;
#pragma unroll
    for (int i = 0; i < C1_LD; ++i) {
      int s, c;
      slot_of(t + 256 * i, s, c);
      const int px = w0 - (C1_K - 1) + s;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (r < g.oh && s < C1_SLOTS && px >= 0 && px < g.ow)
        v = *reinterpret_cast<const uint4*>(src + px * C1_C + c * 8);
      reg[i] = v;
    }
  };
  auto store_row = [&](char* dst, const uint4 (&reg)[C1_LD]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < C1_LD; ++i) {
      int s, c;
      slot_of(t + 256 * i, s, c);
      if (s < C1_SLOTS) *reinterpret_cast<uint4*>(dst + s * C1_PSB + c * 16) = reg[i];
    }
  };
  const int m = lane & 31, half = lane >> 5;
  // one dY row: MFMAs on the staged row r, then scatter Q_r into the LDS output rows r..r+7
  auto compute_row = [&](int r) __attribute__((always_inline)) {
    const char* cur = rows[r & 1];
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const int slot = 32 * wave + m - (ks >> 1) + (C1_K - 1);
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(cur + slot * C1_PSB + (16 * (ks & 1) + 8 * half) * 2);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[ks], acc, 0, 0, 0);
    }
    if (ky < C1_K) {
      float* o = outs + (r + ky) * C1_OLD + 32 * wave + 4 * half;
#pragma unroll
      for (int i = 0; i < 16; ++i) o[(i & 3) + 8 * (i >> 2)] += acc[i];
    }
  };

  // rows are loaded two ahead into alternating register sets (the HBM latency spans two rows of
  // MFMA work) and written to the LDS ring one row ahead
  uint4 ra[C1_LD], rb[C1_LD];
  load_row(0, ra);
  load_row(1, rb);
  store_row(rows[0], ra);
  __syncthreads();
  for (int r = 0; r < g.oh; r += 2) {
    load_row(r + 2, ra);
    compute_row(r);
    store_row(rows[(r + 1) & 1], rb);
    __syncthreads();
    if (r + 1 >= g.oh) break;
    load_row(r + 3, rb);
    compute_row(r + 1);
    store_row(rows[r & 1], ra);
    __syncthreads();
  }

  // store rows of 128 columns as bf16, 4 columns (8 B) per thread-step
  bf16* dxb = g.dx + (int64_t)b * g.h * g.wd;
  for (int q = t; q < g.h * (C1_BW / 4); q += 256) {
    const int y = q / (C1_BW / 4), x4 = (q - y * (C1_BW / 4)) * 4;
    const int x = w0 + x4;
    if (x >= g.wd) continue;
    const float* o = outs + y * C1_OLD + x4;
    if (x + 4 <= g.wd) {
      bf16x4 v = {(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
      *reinterpret_cast<bf16x4*>(dxb + (int64_t)y * g.wd + x) = v;
    } else {
      for (int i = 0; x + i < g.wd; ++i) dxb[(int64_t)y * g.wd + x + i] = (bf16)o[i];
    }
  }
}

// ------------------------------------------------------------------------------ wave-persistent form (default)
// The same arithmetic on another schedule.  conv1ch_dgrad_kernel above (MIA_C1CH_V1=1) waits at every dY row for a
// load issued one row earlier behind a block barrier, starts every block by zeroing its output tile and ends it
// with the tile's store, nothing in flight in either phase: 2.6 TB/s, half the rate streaming kernels reach in the
// same step.  Here a wave owns a (clip, 32 output columns) item end to end -- its own 39-pixel dY strip (2-row LDS
// ring), its own 64 x 32 f32 output strip -- so the kernel has no block barrier at all, and the waves of a
// persistent grid (two blocks per CU) walk the items gw, gw + nw, ...  The wave's dY rows form one stream across
// its items, loaded C2_D rows ahead into a register ring: the conversion, store and re-zeroing of one item's
// output strip run under the loads of the next item's first rows.  Row r's 16 accumulator values stay in
// registers and are added into the output strip between the MFMAs of row r + 1.
// Bit-identity with the form above: Q_r[x][ky] is the same 16-MFMA chain over ks on the same operands (the column
// tiling only decides which wave computes it); out[r + ky][x] takes Q_r in increasing r (one wave per strip, program
// order; the +0 added to a freshly zeroed row when an item starts changes nothing, a sum that starts from +0 is
// never -0); the same f32 -> bf16 cast at the store.
constexpr int C2_SW = 32;                      // output columns per item
constexpr int C2_SLOTS = C2_SW + C1_K - 1;     // staged dY pixels per row (39)
constexpr int C2_ROWB = C2_SLOTS * C1_PSB;     // bytes per staged row
constexpr int C2_LD = (C2_SLOTS * 4 + 63) / 64;  // 16-B chunks per lane per row (3)
constexpr int C2_D = 4;                        // register ring: dY rows in flight per wave
// output strip row stride, floats: 16-byte aligned rows whose 8 kernel rows ky (lanes 0-7 of a half wave, one
// float4 each) start 4 banks apart: the float4 read-modify-write is conflict-free
constexpr int C2_OLD = C2_SW + 4;

__global__ __launch_bounds__(256, 2) void conv1ch_dgrad_wave_kernel(C1Args g, int nstrip, int items) {
  __shared__ __attribute__((aligned(16))) char rows_s[4][2][C2_ROWB];
  __shared__ __attribute__((aligned(16))) float outs_s[4][C1_HMAX * C2_OLD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  if (gw >= items) return;  // no block barrier below
  const int total = (items - gw + nw - 1) / nw * g.oh;  // dY rows of this wave's stream
  char* rows = &rows_s[wave][0][0];
  float* outs = outs_s[wave];

  for (int i = lane; i < C1_HMAX * C2_OLD / 4; i += 64) reinterpret_cast<float4*>(outs)[i] = make_float4(0.f, 0.f, 0.f, 0.f);

  // B fragments, as in conv1ch_dgrad_kernel (every lane loads, from the row ky & 7, so that the 128 loads are
  // issued back to back; the columns ky >= 8 are then zeroed)
  bf16x8 bw[16];
  const int ky = lane & 31;
#pragma unroll
  for (int ks = 0; ks < 16; ++ks) {
    const int kx = ks >> 1, co0 = 16 * (ks & 1) + 8 * (lane >> 5);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float wv = g.w[((co0 + j) * C1_K + (ky & (C1_K - 1))) * C1_K + kx];
      bw[ks][j] = ky < C1_K ? (bf16)wv : (bf16)0.f;
    }
  }

  // lane slot q -> (staged pixel s, 16-B chunk c) as in conv1ch_dgrad_kernel: each 8-lane group of a ds_write_b128
  // takes the 4 chunks of pixels p and p + 4 (conflict-free at the 80-byte pixel stride)
  int sl[C2_LD], lofs[C2_LD];
#pragma unroll
  for (int i = 0; i < C2_LD; ++i) {
    const int q = lane + 64 * i, gq = q >> 3, j = q & 7;
    sl[i] = (gq >> 2) * 8 + (gq & 3) + 4 * (j >> 2);
    lofs[i] = sl[i] * C1_PSB + (j & 3) * 16;
  }

  // Load cursor: the next dY row of the stream to issue.  Every lane always loads, from an address clamped into
  // the row (and the cursor stops on the stream's last row), and what lies outside the image is zeroed when the
  // row goes to LDS (bit i of the row's mask): with no branch around a load the waits stay counted (vmcnt(n)),
  // with one they degrade to vmcnt(0), which drains the ring.
  int lq = 0, lr = 0, lit = gw, lmask = 0;
  const bf16* lsrc = nullptr;
  int gofs[C2_LD];
  auto load_item = [&]() __attribute__((always_inline)) {
    const int b = lit / nstrip, w0 = (lit - b * nstrip) * C2_SW;
    lsrc = g.dy + (int64_t)b * g.oh * g.ow * C1_C;
    lmask = 0;
#pragma unroll
    for (int i = 0; i < C2_LD; ++i) {
      const int px = w0 - (C1_K - 1) + sl[i];
      lmask |= (int)(sl[i] < C2_SLOTS && px >= 0 && px < g.ow) << i;
      gofs[i] = min(max(px, 0), g.ow - 1) * C1_C + ((lane + 64 * i) & 3) * 8;
    }
  };
  load_item();
  auto load_next = [&](uint4 (&reg)[C2_LD], int& mask) __attribute__((always_inline)) {
    const bf16* src = lsrc + (int64_t)lr * g.ow * C1_C;
#pragma unroll
    for (int i = 0; i < C2_LD; ++i) reg[i] = *reinterpret_cast<const uint4*>(src + gofs[i]);
    mask = lmask;
    if (lq + 1 < total) {
      ++lq;
      if (++lr == g.oh) {
        lr = 0;
        lit += nw;
        load_item();
      }
    }
  };
  auto store_row = [&](char* dst, const uint4 (&reg)[C2_LD], int mask) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < C2_LD; ++i) {
      const bool ok = (mask >> i) & 1;
      const uint4 v = make_uint4(ok ? reg[i].x : 0u, ok ? reg[i].y : 0u, ok ? reg[i].z : 0u, ok ? reg[i].w : 0u);
      if (sl[i] < C2_SLOTS) *reinterpret_cast<uint4*>(dst + lofs[i]) = v;
    }
  };

  const int m = lane & 31, half = lane >> 5;
  // compute cursor
  int cit = gw, cr = 0, prow = 0;
  f32x16 accp;  // Q of the previous row, not yet added into the output strip (rows prow .. prow + 7)
#pragma unroll
  for (int i = 0; i < 16; ++i) accp[i] = 0.f;
  // out[prow + ky][4 half + 8 gi + 0..3] += accp[4 gi .. 4 gi + 3]
  auto add_group = [&](int gi) __attribute__((always_inline)) {
    if (ky < C1_K) {
      float4* o = reinterpret_cast<float4*>(outs + (prow + ky) * C2_OLD + 4 * half + 8 * gi);
      float4 v = *o;
      v.x += accp[4 * gi];
      v.y += accp[4 * gi + 1];
      v.z += accp[4 * gi + 2];
      v.w += accp[4 * gi + 3];
      *o = v;
    }
  };
  // the finished item's strip: h rows of 32 columns as bf16, 4 columns (8 B) per lane-step; zeroed for the next item
  auto finish_item = [&]() __attribute__((always_inline)) {
    const int b = cit / nstrip, w0 = (cit - b * nstrip) * C2_SW;
    bf16* dxb = g.dx + (int64_t)b * g.h * g.wd;
#pragma unroll
    for (int k = 0; k < C1_HMAX / 8; ++k) {  // 8 rows of 8 pieces per pass
      const int y = 8 * k + (lane >> 3), x4 = (lane & 7) * 4, x = w0 + x4;
      float4* o = reinterpret_cast<float4*>(outs + y * C2_OLD + x4);
      const float4 v = *o;
      *o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (y < g.h && x + 4 <= g.wd) {  // wd is a multiple of 4: a 4-column piece is inside the image or outside it
        bf16x4 c = {(bf16)v.x, (bf16)v.y, (bf16)v.z, (bf16)v.w};
        *reinterpret_cast<bf16x4*>(dxb + (int64_t)y * g.wd + x) = c;
      }
    }
  };
  // one dY row of the stream: MFMAs on the staged row (ring slot par) with the previous row's adds between them,
  // then the next row moves from its registers (nxt) to the other ring slot and its registers take a new load
  auto step = [&](uint4 (&nxt)[C2_LD], int& nmask, int par) __attribute__((always_inline)) {
    const char* cur = rows + par * C2_ROWB;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      const int slot = m - (ks >> 1) + (C1_K - 1);
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(cur + slot * C1_PSB + (16 * (ks & 1) + 8 * half) * 2);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bw[ks], acc, 0, 0, 0);
      if ((ks & 3) == 3) add_group(ks >> 2);
    }
    wave_sync();  // this row's fragment reads and strip adds are done (common.h)
    store_row(rows + (par ^ 1) * C2_ROWB, nxt, nmask);
    load_next(nxt, nmask);
    accp = acc;
    prow = cr;
    if (++cr == g.oh) {  // last dY row of the item
#pragma unroll
      for (int gi = 0; gi < 4; ++gi) add_group(gi);
      wave_sync();
      finish_item();
#pragma unroll
      for (int i = 0; i < 16; ++i) accp[i] = 0.f;
      prow = 0;
      cr = 0;
      cit += nw;
    }
    wave_sync();
  };

  uint4 rg[C2_D][C2_LD];
  int rmask[C2_D];
#pragma unroll
  for (int j = 0; j < C2_D; ++j) load_next(rg[j], rmask[j]);
  store_row(rows, rg[0], rmask[0]);
  load_next(rg[0], rmask[0]);
  wave_sync();
  static_assert(C2_D == 4, "the loop below is unrolled over the ring");
  // stream row q: ring slot q & 1, the next row in rg[(q + 1) % C2_D].  Whole turns of the ring first, with no exit
  // inside a turn (an exit there joins the loop header in the compiler's flow graph and turns the header's
  // counted waits into vmcnt(0)), then the at most three rows left over.
  int q = 0;
  for (; q + C2_D <= total; q += C2_D) {
    step(rg[1], rmask[1], 0);
    step(rg[2], rmask[2], 1);
    step(rg[3], rmask[3], 0);
    step(rg[0], rmask[0], 1);
  }
  if (q < total) step(rg[1], rmask[1], 0);
  if (q + 1 < total) step(rg[2], rmask[2], 1);
  if (q + 2 < total) step(rg[3], rmask[3], 0);
}

// A/B switch, read at call time: MIA_C1CH_V1=1 selects conv1ch_dgrad_kernel
bool c1ch_v1() { const char* e = getenv("MIA_C1CH_V1"); return e && e[0] == '1'; }

}  // namespace

extern "C" int mia_conv1ch_dgrad(const void* dy, const float* w, void* dx, int32_t n, int32_t oh, int32_t ow,
                                 mia_stream_t stream) {
  MIA_CHECK_ARG(dy && w && dx && n > 0 && oh > 0 && ow > 0, "conv1ch_dgrad: bad arguments");
  const int h = oh + C1_K - 1, wd = ow + C1_K - 1;
  MIA_CHECK_ARG(h <= C1_HMAX, "conv1ch_dgrad: at most %d output rows (got %d)", C1_HMAX, h);
  MIA_CHECK_ARG(wd % 4 == 0, "conv1ch_dgrad: output width must be a multiple of 4 (got %d)", wd);
  MIA_CHECK_ARG((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx)) % 16 == 0,
                "conv1ch_dgrad: dy/dx must be 16-byte aligned");
  MIA_CHECK_ARG((int64_t)oh * ow * C1_C < (1ll << 31), "conv1ch_dgrad: clip too large for 32-bit indexing");
  C1Args a{reinterpret_cast<const bf16*>(dy), w, reinterpret_cast<bf16*>(dx), n, oh, ow, h, wd,
           (int)cdiv(wd, C1_BW)};
  if (c1ch_v1()) {
    const int64_t blocks = (int64_t)n * a.nchunk;
    MIA_CHECK_ARG(blocks < (1ll << 31), "conv1ch_dgrad: grid too large");
    conv1ch_dgrad_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(a);
    MIA_LAUNCH_CHECK("conv1ch_dgrad");
    return 0;
  }
  // one item per (clip, 32 columns), 4 waves a block, at most two blocks per CU; MIA_C1CH_GRID (read at call time)
  // caps the grid further, so that small shapes can be made to walk several items per wave
  const int nstrip = (int)cdiv(wd, C2_SW);
  const int64_t items = (int64_t)n * nstrip;
  MIA_CHECK_ARG(items < (1ll << 31), "conv1ch_dgrad: grid too large");
  int64_t blocks = cdiv(items, 4);
  if (blocks > 2 * mia::cu_count()) blocks = 2 * mia::cu_count();
  if (const char* e = getenv("MIA_C1CH_GRID")) {
    const long cap = strtol(e, nullptr, 10);
    if (cap > 0 && cap < blocks) blocks = cap;
  }
  MIA_CHECK_ARG(cdiv(items, blocks * 4) * oh < (1ll << 31), "conv1ch_dgrad: too many rows per wave");
  conv1ch_dgrad_wave_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(a, nstrip, (int)items);
  MIA_LAUNCH_CHECK("conv1ch_dgrad");
  return 0;
}
