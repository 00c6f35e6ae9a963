// mia_gemm: the dispatcher of the dense contractions of the hot path, gfx950.
//
// One selector (gemm_select) decides which kernel family runs a call; mia_gemm, mia_gemm_path and
// mia_gemm_workspace_bytes_ex all ask it.  Each family lives in its own file beside its eligibility
// predicate and its launcher (gemm_common.h): igemm.hip (0, the implicit-GEMM tile kernel every shape can
// take), rowconv.hip (1, 2), tapconv.hip (3, 4), dgemm.hip (5), wgrad8.hip (the 8x8 case of 2), mgemm.hip (7).
// Here besides: the split-K reducers that apply the epilogue to the f32 partial slabs, and the operand checks.
#include "gemm_common.h"

#include <cstdlib>

namespace {

using namespace mgemm;

__global__ void splitk_reduce_kernel(const float* ws, int split, int64_t M, int64_t N, EpiDev e) {
  const int64_t total = M * N;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < split; ++z) s += ws[z * total + idx];
    epi_store(e, idx / N, idx % N, s);
  }
}

// Many-slab reduction (split >= 32): 16 outputs x 16 slab lanes per block, fixed per-lane slab
// order and a fixed LDS tree -> deterministic; the plain kernel walks all slabs per thread.
__global__ __launch_bounds__(256) void splitk_reduce_wide_kernel(const float* ws, int split, int64_t M, int64_t N,
                                                                 EpiDev e) {
  __shared__ float red[16][17];
  const int64_t total = M * N;
  const int o = threadIdx.x & 15, zl = threadIdx.x >> 4;
  const int64_t idx = (int64_t)blockIdx.x * 16 + o;
  float s = 0.f;
  if (idx < total)
    for (int z = zl; z < split; z += 16) s += ws[(int64_t)z * total + idx];
  red[zl][o] = s;
  __syncthreads();
  if (threadIdx.x < 16) {
    float a = 0.f;
    for (int k = 0; k < 16; ++k) a += red[k][threadIdx.x];
    const int64_t id = (int64_t)blockIdx.x * 16 + threadIdx.x;
    if (id < total) epi_store(e, id / N, id % N, a);
  }
}

}  // namespace

namespace mgemm {

void launch_splitk_reduce(const float* ws, int split, int64_t M, int64_t N, const EpiDev& e, hipStream_t s) {
  const int64_t total = M * N;
  if (split >= 32 && total <= (1ll << 22)) {
    splitk_reduce_wide_kernel<<<(unsigned)cdiv(total, 16), 256, 0, s>>>(ws, split, M, N, e);
  } else {
    int blocks = (int)std::min<int64_t>(cdiv(total, 256), 8192);
    splitk_reduce_kernel<<<blocks, 256, 0, s>>>(ws, split, M, N, e);
  }
}

EpiDev to_dev(const MiaEpilogue& e) {
  EpiDev d;
  d.ptr = reinterpret_cast<char*>(e.ptr);
  d.dtype = e.dtype; d.act = e.act; d.accumulate = e.accumulate; d.aux_dtype = e.aux_dtype;
  d.ldc = e.ldc; d.rm_inner = e.rm_inner; d.rm_outer = e.rm_outer; d.rm_istride = e.rm_istride;
  d.rm_offset = e.rm_offset; d.bias = e.bias; d.aux = reinterpret_cast<const char*>(e.aux);
  d.ldaux = e.ldaux; d.alpha = e.alpha; d.act_scale = e.act_scale;
  d.sqsum = e.sqsum;
  return d;
}

}  // namespace mgemm

static int check_operand(const MiaOperand& o, const char* name) {
  MIA_CHECK_ARG(o.ptr != nullptr, "gemm: operand %s is null", name);
  MIA_CHECK_ARG(o.dtype == MIA_F32 || o.dtype == MIA_BF16, "gemm: operand %s dtype %d", name, o.dtype);
  MIA_CHECK_ARG(o.layout == MIA_LAYOUT_KC || o.layout == MIA_LAYOUT_RC, "gemm: operand %s layout", name);
  if (o.pre == MIA_PRE_AFFINE || o.pre == MIA_PRE_AFFINE_RELU)
    MIA_CHECK_ARG(o.pre_scale && o.pre_shift && o.kind != MIA_OP_CONVROW,
                  "gemm: operand %s affine pre-op needs scale/shift and a DENSE/CONV source", name);
  if (o.kind == MIA_OP_DENSE) {
    // ld < cols is allowed: overlapping rows are a valid read-only view (the (1, 2)-conv im2col of
    // a channels-last map is the map itself with ld = C, cols = 2C)
    MIA_CHECK_ARG(o.rows >= 0 && o.cols >= 0 && o.ld > 0, "gemm: operand %s dense extents", name);
  } else {
    MIA_CHECK_ARG(o.n > 0 && o.h > 0 && o.w > 0 && o.c > 0 && o.oh > 0 && o.ow > 0 && o.kh > 0 &&
                      o.kw > 0 && o.sh > 0 && o.sw > 0,
                  "gemm: operand %s conv geometry", name);
    MIA_CHECK_ARG((int64_t)o.n * o.oh * o.ow < (1ll << 31), "gemm: operand %s too many pixels", name);
    if (o.kind == MIA_OP_CONV) {
      MIA_CHECK_ARG(o.c % 8 == 0, "gemm: operand %s CONV needs c %% 8 == 0 (c=%d)", name, o.c);
    } else {
      MIA_CHECK_ARG((o.kw * o.c) % 8 == 0 && o.pw == 0, "gemm: operand %s CONVROW needs kw*c %% 8 == 0, pw == 0", name);
      MIA_CHECK_ARG((int64_t)(o.ow - 1) * o.sw + o.kw <= o.w, "gemm: operand %s CONVROW row overruns input", name);
    }
  }
  return 0;
}

extern "C" int64_t mia_gemm_workspace_bytes(int64_t M, int64_t N, int32_t split_k) {
  return split_k > 1 ? (int64_t)split_k * M * N * 4 : 0;
}

// -------------------------------------------------------------------------- dispatch
// The path numbers mia_gemm_path reports (include/miaudio.h); 6 is the rolling-window 8x8 case of the
// row-window weight gradient (wgrad8.hip), reported as 2.
enum GemmPath {
  PATH_TILE = 0, PATH_ROWCONV = 1, PATH_ROWWGRAD = 2, PATH_TAPWGRAD = 3, PATH_TAPCONV = 4, PATH_DENSE = 5,
  PATH_WGRAD8 = 6, PATH_MG = 7
};

// Which kernel family takes this GEMM: the one place that asks the families' *_ok predicates.  The 256x256
// kernel first (it alone depends on the epilogue); the others exclude each other through their operand kinds
// (dense x dense; CONVROW / CONV forward with split 1; CONVROW / CONV weight gradient with split >= 2).
static GemmPath gemm_select(const MiaOperand& A, const MiaOperand& B, const MiaEpilogue& E, int64_t M, int64_t N,
                            int64_t K, int compute, int split) {
  if (E.ptr && M > 0 && N > 0 && K > 0 && mg_ok(A, B, E, M, N, K, compute)) return PATH_MG;
  if (dgemm_ok(A, B, M, N, K, compute)) return PATH_DENSE;
  if (tapconv_ok(A, B, M, N, K, compute, split)) return PATH_TAPCONV;
  if (rowconv_ok(A, B, M, N, K, compute, split)) return PATH_ROWCONV;
  if (tapwgrad_ok(A, B, M, N, K, compute, split)) return PATH_TAPWGRAD;
  if (rowwgrad_ok(A, B, M, N, K, compute, split)) return wgrad8_ok(A, B, M) ? PATH_WGRAD8 : PATH_ROWWGRAD;
  return PATH_TILE;
}

// The argument checks of paths 0-6, then the selected family's launch.
static int gemm_run(GemmPath path, const MiaOperand* A, const MiaOperand* B, const MiaEpilogue* E, int64_t M,
                    int64_t N, int64_t K, int32_t compute_dtype, int32_t split_k, void* workspace,
                    mia_stream_t stream) {
  MIA_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "gemm: negative extent");
  MIA_CHECK_ARG(M < (1ll << 31) * 128 && N < 65535ll * 128, "gemm: extent too large");
  if (int r = check_operand(*A, "A")) return r;
  if (int r = check_operand(*B, "B")) return r;
  MIA_CHECK_ARG(E->ptr != nullptr, "gemm: output is null");
  MIA_CHECK_ARG(compute_dtype == MIA_F32 || compute_dtype == MIA_BF16, "gemm: compute dtype");
  if (E->act == MIA_DACT_NZ || E->act == MIA_DACT_GELU || E->act == MIA_ACT_ADD_AUX || E->act == MIA_ACT_GELU_SAVE ||
      E->act == MIA_ACT_GELU_SAVE_D || E->act == MIA_DACT_MUL)
    MIA_CHECK_ARG(E->aux != nullptr, "gemm: this epilogue needs aux");
  if (split_k < 1) split_k = 1;
  if (split_k > 1) MIA_CHECK_ARG(workspace != nullptr, "gemm: split_k needs workspace");
  if (M == 0 || N == 0) return 0;
  hipStream_t s = as_stream(stream);
  switch (path) {
    case PATH_DENSE: return dgemm_run(*A, *B, *E, M, N, K, split_k, workspace, s);
    case PATH_TAPCONV: return tapconv_run(*A, *B, *E, s);
    case PATH_ROWCONV: return rowconv_run(*A, *B, *E, M, N, s);
    case PATH_TAPWGRAD: return tapwgrad_run(*A, *B, *E, M, N, split_k, workspace, s);
    case PATH_WGRAD8: return wgrad8_run(*A, *B, *E, M, N, split_k, workspace, s);
    case PATH_ROWWGRAD: return rowwgrad_run(*A, *B, *E, M, N, split_k, workspace, s);
    default: return igemm_run(*A, *B, *E, M, N, K, compute_dtype, split_k, workspace, s);
  }
}

// workspace layout of one mia_gemm call on paths 0-5: [split-K slabs][column-sum partials]
static int64_t colsum_ws_offset(int64_t M, int64_t N, int32_t split_k) {
  return cdiv(mia_gemm_workspace_bytes(M, N, split_k), 256) * 256;
}

extern "C" int64_t mia_gemm_workspace_bytes_ex(const MiaOperand* A, const MiaOperand* B, const MiaEpilogue* E,
                                               int64_t M, int64_t N, int64_t K, int32_t compute_dtype,
                                               int32_t split_k) {
  if (!A || !B || !E) return 0;
  if (gemm_select(*A, *B, *E, M, N, K, compute_dtype, split_k) == PATH_MG)
    return mg_workspace_bytes(M, N, K, E->colsum != nullptr, E->a_colsum != nullptr);
  if (E->a_colsum) {  // the GEMM's own workspace, then the column-sum pass over A
    MiaEpilogue e = *E;
    e.a_colsum = nullptr;
    return cdiv(mia_gemm_workspace_bytes_ex(A, B, &e, M, N, K, compute_dtype, split_k), 256) * 256 +
           (int64_t)MIA_COLSUM_MAXBLK * M * 4;
  }
  int64_t b = mia_gemm_workspace_bytes(M, N, split_k);
  if (E->colsum) b = colsum_ws_offset(M, N, split_k) + (int64_t)MIA_COLSUM_MAXBLK * N * 4;
  return b;
}

extern "C" int mia_gemm(const MiaOperand* A, const MiaOperand* B, const MiaEpilogue* E, int64_t M,
                        int64_t N, int64_t K, int32_t compute_dtype, int32_t split_k, void* workspace,
                        mia_stream_t stream) {
  MIA_CHECK_ARG(A && B && E, "gemm: null descriptor");
  const GemmPath path = gemm_select(*A, *B, *E, M, N, K, compute_dtype, split_k);
  if (path == PATH_MG) return mg_run(*A, *B, *E, M, N, K, workspace, as_stream(stream));
  MIA_CHECK_ARG(!E->mx_q, "gemm: an MX-fp8 output copy needs the 256x256 kernel (bf16 dense operands, "
                "plain / GELU / GELU_SAVE bf16 output, ldc == N, N %% 32 == 0)");
  if (E->a_colsum) {  // other paths: the GEMM, then a column-sum pass over the k-by-m A
    MIA_CHECK_ARG(A->kind == MIA_OP_DENSE && A->layout == MIA_LAYOUT_RC && A->pre == MIA_PRE_NONE &&
                      (A->dtype == MIA_BF16 || A->dtype == MIA_F32) && A->rows >= K && A->cols == M,
                  "gemm: a_colsum needs a dense k-by-m (RC) A without pre-op");
    MIA_CHECK_ARG(workspace || M == 0 || K == 0, "gemm a_colsum: needs the workspace of mia_gemm_workspace_bytes_ex");
    MiaEpilogue e = *E;
    e.a_colsum = nullptr;
    if (int r = mia_gemm(A, B, &e, M, N, K, compute_dtype, split_k, workspace, stream)) return r;
    if (M == 0) return 0;
    void* ws = static_cast<char*>(workspace) +
               cdiv(mia_gemm_workspace_bytes_ex(A, B, &e, M, N, K, compute_dtype, split_k), 256) * 256;
    return mia_colsum(A->ptr, A->dtype, K, (int32_t)M, A->ld, E->a_colsum, ws, stream);
  }
  if (E->colsum) {
    MIA_CHECK_ARG(!E->sqsum && !E->accumulate && !E->rm_inner && E->ldc >= N &&
                      (E->dtype == MIA_BF16 || E->dtype == MIA_F32),
                  "gemm: colsum needs a plain row-major output");
    MIA_CHECK_ARG(workspace || M == 0 || N == 0, "gemm colsum: needs the workspace of mia_gemm_workspace_bytes_ex");
    if (int r = gemm_run(path, A, B, E, M, N, K, compute_dtype, split_k, workspace, stream)) return r;
    if (M > 0 && N > 0) {
      void* ws = static_cast<char*>(workspace) + colsum_ws_offset(M, N, split_k);
      if (int r = mia_colsum(E->ptr, E->dtype, M, (int32_t)N, E->ldc, E->colsum, ws, stream)) return r;
    }
    return 0;
  }
  if (!E->sqsum) return gemm_run(path, A, B, E, M, N, K, compute_dtype, split_k, workspace, stream);
  MIA_CHECK_ARG(E->dtype == MIA_F32 && E->act == MIA_ACT_NONE && !E->bias && !E->accumulate && !E->rm_inner &&
                    E->alpha == 1.f,
                "gemm: sqsum needs a plain f32 output");
  if (int r = gemm_run(path, A, B, E, M, N, K, compute_dtype, split_k, workspace, stream)) return r;
  // the dense kernel writes the slots itself when it runs unsplit; every other path gets the pass
  if ((path == PATH_DENSE && split_k <= 1) || M == 0 || N == 0) return 0;
  return tile_sqsum_run(reinterpret_cast<const float*>(E->ptr), E->ldc, M, N, E->sqsum, as_stream(stream));
}

extern "C" int mia_gemm_path(const MiaOperand* A, const MiaOperand* B, int64_t M, int64_t N, int64_t K,
                             int32_t compute_dtype, int32_t split_k) {
  if (!A || !B) return -1;
  MiaEpilogue e{};
  e.ptr = reinterpret_cast<void*>(256); e.dtype = MIA_BF16; e.ldc = N; e.alpha = 1.f;
  const GemmPath path = gemm_select(*A, *B, e, M, N, K, compute_dtype, split_k);
  return path == PATH_WGRAD8 ? PATH_ROWWGRAD : path;
}

extern "C" int mia_splitk_reduce(const float* ws, int32_t split_k, int64_t M, int64_t N,
                                 const MiaEpilogue* E, mia_stream_t stream) {
  MIA_CHECK_ARG(ws && E && E->ptr, "splitk_reduce: null pointer");
  EpiDev e = to_dev(*E);
  const int64_t total = M * N;
  if (total == 0) return 0;
  launch_splitk_reduce(ws, split_k, M, N, e, as_stream(stream));
  MIA_LAUNCH_CHECK("splitk_reduce");
  return 0;
}
