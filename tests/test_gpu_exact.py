"""GPU: every GEMM and conv kernel path with integer-valued operands, compared bit for bit with float64.

The exact-domain rule (tests/_exact.py, checked on the CPU for every case before the launch): every operand is
an integer with |v| <= 256 -- exact in bf16 and f32, so every product is exact in f32 -- and the float64
magnitude bound of the case (|A| |B|^T, or |x| and |w| through conv2d, plus the |bias| / |aux| / |base| maxima,
times act_scale) is < 2^24, so the f32 accumulation is exact in any order, over any tiling and under any
split-K.  An f32 output must equal the float64 reference bit for bit, a bf16 output its round-to-nearest-even
cast; every bf16 comparison also requires the reference to hold a value that needs rounding and an exact tie.
A dropped, doubled or misplaced product, a stale tile, a wrong tail, a double bias or a truncating store changes
at least one output (unless the affected product is zero).  Operands are uniform in [-h, h], h = 3 widened by
_exact.operand_hi where K is short, so that bf16 outputs reach the range where integers round; pre-op scale is
in {1, 2}, shift in {-2 .. 2}; biases, aux tensors and accumulate bases are integers in [-8, 8]; act_scale = 2,
alpha = 1.

Covered entry points
  mia_gemm path 0 (generic tile kernel): four layout pairs; f32 compute, bf16 compute, bf16 compute over
    f32-stored operands; f32 and bf16 (+bias) outputs; split-K 1 and 3.
  mia_gemm path 5 (dense 128x128): four layout pairs, split-K 4, padded operand ld, ldc > N.
  mia_gemm path 7 (256x256): plain f32, bias -> bf16, ACT_ADD_AUX f32, DACT_MUL + colsum; N % 8 == 4; the
    long-K weight-gradient form with its own split-K and a_colsum.
  mia_gemm path 1 (row-window conv) forward and padded dgrad; path 2 (row-window wgrad) and its wgrad8 special
    case; path 3 (tap wgrad) and path 4 (tap conv) for conv1 and conv3.
  Linear epilogues on paths 0 and 5: bias + ReLU, ACT_ADD_AUX, DACT_NZ with act_scale and accumulate, DACT_MUL,
    colsum; the (Tp, W1, 2, par) row map of the stride-2 parity dgrad; RM_DROP through conv_w2_fwd.
  One documented rounding rule is asserted instead of "rounded once": the 256x256 kernel applies DACT_MUL to
    the bf16-rounded accumulator ("Rounding of the 256x256 kernel's bf16 epilogues"), paths 0 and 5
    to the f32 accumulator; each is asserted exactly.
  mia_fe_conv1_fwd, mia_fe_conv2_{fwd,dgrad,wgrad}, mia_fe_conv3_fwd, mia_trunk_conv8 (forward and the padded
    backward-data form), mia_conv3_wgrad, mia_conv1ch_dgrad, conv_w2_fwd / trunk_bwd_w2 (both backward forms).
  Where such a kernel also emits BN statistics only its conv output is compared here.

Exclusions (they stay on their existing tolerance tests)
  sqsum slots: sums of squares leave 2^24 in f32.
  ACT_GELU, ACT_GELU_SAVE, ACT_GELU_SAVE_D, DACT_GELU epilogues: erf has no integer-exact form.
  The BN-backward terms of mia_conv3_wgrad_bn, mia_trunk_conv8_dgrad_bn and mia_fe_conv1_wgrad_bn (mean, invstd
    and the 1/P-scaled sums are not integers); their conv parts run the kernels covered above and are tied to
    them bit for bit by tests/test_gpu_norm.py.
  The BN statistics of fe_conv1_fwd / fe_conv3_fwd / trunk_conv8 (sums of squares, reciprocal square roots).
  The MX-fp8 GEMM (the scaled MFMA's internal sum is inexact in hardware), mia_gemm_adam / mia_gemm_sqsum_only
    (Adam arithmetic, sums of squares), attention, LayerNorm, BN, pooling, LEAF and log-mel.

mia_gemm_path probes with a plain bf16 epilogue, so for N % 8 == 4 it reports path 5 although an f32 output
stays on the 256x256 kernel (test_path7_ragged_n); every other case asserts its intended path."""
import pytest
import torch
import torch.nn.functional as F

from src.miaudio import kernels as K
from src.miaudio import lib as L
from tests._exact import (assert_bit_equal, assert_exact_domain, conv_bound, gemm_bound, int_tensor, operand_hi,
                          pre_affine)

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
LAYOUTS = [(L.KC, L.KC), (L.KC, L.RC), (L.RC, L.KC), (L.RC, L.RC)]


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _path(A, Bo, M, N, Kd, split):
    return L.load().mia_gemm_path(A, Bo, M, N, Kd, L.BF16, split)


def _operand(src, layout, dev, store, pad=0):
    """Dense operand of the logical [rows][k] integer matrix ``src`` stored per layout in dtype ``store``; ``pad``
    extra NaN elements per stored row (ld = row length + pad)."""
    rows, k = src.shape
    t = (src if layout == L.KC else src.t()).to(store)
    full = torch.full((t.shape[0], t.shape[1] + pad), NAN, dtype=store)
    full[:, :t.shape[1]] = t
    full = full.to(dev)
    if layout == L.KC:
        return K.dense(full, L.KC, rows, k, ld=k + pad)
    return K.dense(full, L.RC, k, rows, ld=rows + pad)


def _ab(M, N, Kd, g, h=None):
    h = operand_hi(Kd) if h is None else h
    return int_tensor((M, Kd), -h, h, g), int_tensor((N, Kd), -h, h, g)


def _guarded(M, N, ldc, dt, dev):
    """A NaN-filled (M + 1, ldc) buffer and its (M, N) output view."""
    full = torch.full((M + 1, ldc), NAN, dtype=dt, device=dev)
    return full, full[:M, :N]


def _assert_untouched(full, M, N, what):
    assert bool(torch.isnan(full[M:].float()).all()) and bool(torch.isnan(full[:, N:].float()).all()), \
        f"{what}: wrote outside the {M} x {N} output"


# ------------------------------------------------------------------------------------ path 0
MODES = {"f32": (L.F32, F32), "bf16": (L.BF16, BF16), "staged": (L.BF16, F32)}  # compute, operand storage


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("M,N,Kd", [(37, 50, 200), (130, 70, 8), (300, 32, 64), (64, 600, 40)])
def test_path0_generic(cuda, mode, la, lb, M, N, Kd):
    cd, store = MODES[mode]
    g = _gen(M, N, Kd, la, lb)
    a, b = _ab(M, N, Kd, g)
    bias = int_tensor((N,), -8, 8, g)
    assert_exact_domain(gemm_bound(a, b, bias), a, b, bias)
    A, Bo = _operand(a, la, cuda, store), _operand(b, lb, cuda, store)
    z = a.double() @ b.double().t()
    tb = bias.to(cuda)
    for split in (1, 3):
        if cd == L.BF16:
            assert _path(A, Bo, M, N, Kd, split) == 0
        out = torch.full((M, N), NAN, dtype=F32, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N), M, N, Kd, cd, split_k=split)
        outb = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        K.gemm(A, Bo, K.epilogue(outb, N, bias=tb), M, N, Kd, cd, split_k=split)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), z, F32, f"path 0 {mode} split {split} f32")
        assert_bit_equal(outb.cpu(), z + bias.double(), BF16, f"path 0 {mode} split {split} bf16+bias")


# ------------------------------------------------------------------------------------ path 5
@pytest.mark.parametrize("la,lb", LAYOUTS)
@pytest.mark.parametrize("M,N,Kd,split", [(64, 72, 64, 1), (296, 200, 192, 1), (256, 384, 4096, 4)])
def test_path5_dense(cuda, la, lb, M, N, Kd, split):
    g = _gen(5, M, N, Kd, la, lb)
    a, b = _ab(M, N, Kd, g)
    bias = int_tensor((N,), -8, 8, g)
    assert_exact_domain(gemm_bound(a, b, bias), a, b, bias)
    A, Bo = _operand(a, la, cuda, BF16), _operand(b, lb, cuda, BF16)
    assert _path(A, Bo, M, N, Kd, split) == 5
    ref = a.double() @ b.double().t() + bias.double()
    for odt in (F32, BF16):
        out = torch.full((M, N), NAN, dtype=odt, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, bias=bias.to(cuda)), M, N, Kd, L.BF16, split_k=split)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), ref, odt, f"path 5 split {split} {odt}")


@pytest.mark.parametrize("what", ["ld", "ldc"])
@pytest.mark.parametrize("la,lb", [(L.KC, L.RC), (L.RC, L.KC)])
def test_path5_padded(cuda, what, la, lb):
    """Operand rows padded with NaN (ld = row length + 8), and an output with ldc = N + 8 in a NaN-filled
    buffer: nothing is written past column N or row M, and no pad element reaches a stored output."""
    M, N, Kd = 296, 200, 192
    g = _gen(55, la, lb)
    a, b = _ab(M, N, Kd, g)
    assert_exact_domain(gemm_bound(a, b), a, b)
    pad = 8 if what == "ld" else 0
    A, Bo = _operand(a, la, cuda, BF16, pad), _operand(b, lb, cuda, BF16, pad)
    assert _path(A, Bo, M, N, Kd, 1) == 5
    ref = a.double() @ b.double().t()
    ldc = N + (8 if what == "ldc" else 0)
    for odt in (F32, BF16):
        full, out = _guarded(M, N, ldc, odt, cuda)
        K.gemm(A, Bo, K.epilogue(out, ldc), M, N, Kd, L.BF16, split_k=1)
        torch.cuda.synchronize()
        _assert_untouched(full, M, N, f"path 5 {what}")
        assert_bit_equal(out.cpu().contiguous(), ref, odt, f"path 5 padded {what} {odt}")


# ------------------------------------------------------------------------------------ linear epilogues, paths 0 and 5
EPI_CASES = {  # shape, compute, operand storage, path
    "p0_f32_small": ((64, 96, 48), L.F32, F32, 0),
    "p0_bf16_small": ((64, 96, 48), L.BF16, BF16, 0),
    "p0_staged": ((296, 200, 192), L.BF16, F32, 0),
    "p5": ((296, 200, 192), L.BF16, BF16, 5),
}


@pytest.mark.parametrize("epi", ["bias_relu", "add_aux", "dact_nz_acc", "dact_mul", "colsum"])
@pytest.mark.parametrize("case", list(EPI_CASES))
def test_linear_epilogues(cuda, case, epi):
    (M, N, Kd), cd, store, path = EPI_CASES[case]
    g = _gen(M, Kd, len(epi), len(case))
    a, b = _ab(M, N, Kd, g)
    bias = int_tensor((N,), -8, 8, g)
    A, Bo = _operand(a, L.KC, cuda, store), _operand(b, L.KC, cuda, store)
    if cd == L.BF16:
        assert _path(A, Bo, M, N, Kd, 1) == path
    z = a.double() @ b.double().t()
    what = f"{case} {epi}"
    if epi == "bias_relu":
        assert_exact_domain(gemm_bound(a, b, bias), a, b, bias)
        for odt in (F32, BF16):
            out = torch.full((M, N), NAN, dtype=odt, device=cuda)
            K.gemm(A, Bo, K.epilogue(out, N, act=L.ACT_RELU, bias=bias.to(cuda)), M, N, Kd, cd, split_k=1)
            torch.cuda.synchronize()
            assert_bit_equal(out.cpu(), torch.relu(z + bias.double()), odt, f"{what} {odt}")
    elif epi == "add_aux":
        aux = int_tensor((M, N), -8, 8, g)
        assert_exact_domain(gemm_bound(a, b, bias, aux), a, b, bias, aux)
        out = torch.full((M, N), NAN, dtype=F32, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, act=L.ACT_ADD_AUX, bias=bias.to(cuda), aux=aux.to(cuda), ldaux=N), M, N, Kd,
               cd, split_k=1)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), z + bias.double() + aux.double(), F32, what)
    elif epi == "dact_nz_acc":
        aux = int_tensor((M, N), 0, 2, g)  # a third of the mask is zero
        base = int_tensor((M, N), -8, 8, g)
        assert_exact_domain(gemm_bound(a, b, factor=2.0) + 8, a, b, aux, base)
        out = base.clone().to(cuda)
        K.gemm(A, Bo, K.epilogue(out, N, act=L.DACT_NZ, aux=aux.to(cuda), ldaux=N, act_scale=2.0, accumulate=True),
               M, N, Kd, cd, split_k=1)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), base.double() + z * (aux != 0).double() * 2.0, F32, what)
    elif epi == "dact_mul":  # the f32 accumulator times aux, rounded once (the 256x256 kernel differs: see there)
        aux = int_tensor((M, N), -8, 8, g, BF16)
        assert_exact_domain(gemm_bound(a, b, factor=8.0), a, b, aux)
        out = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, act=L.DACT_MUL, aux=aux.to(cuda), ldaux=N), M, N, Kd, cd, split_k=1)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), z * aux.double(), BF16, what)
    else:
        assert_exact_domain(gemm_bound(a, b), a, b)
        out = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        cs = torch.full((N,), NAN, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, colsum=cs), M, N, Kd, cd, split_k=1)
        torch.cuda.synchronize()
        assert_bit_equal(out.cpu(), z, BF16, what)
        stored = z.float().to(BF16).double()  # the sums are of the stored values: integers, hence exact
        assert float(stored.abs().sum(0).max()) < 2 ** 24
        assert_bit_equal(cs.cpu(), stored.sum(0), F32, f"{what} sums")


@pytest.mark.parametrize("cd", [L.F32, L.BF16])
def test_rowmap_parity_dgrad(cuda, cd):
    """The (Tp, W1, 2, par) row map: frontend conv2 backward-data as two stride-1 parity convolutions whose
    epilogues interleave their rows (bf16 compute: the row-window kernel, path 1; f32: the generic gather)."""
    n, cin, cout, W1, kw = 2, 32, 64, 301, 16
    W2 = (W1 - kw) // 2 + 1
    g = _gen(31, cd)
    dt = F32 if cd == L.F32 else BF16
    h = operand_hi(512)
    wt = int_tensor((cout, cin, 1, kw), -h, h, g)
    dy = int_tensor((n, 1, W2, cout), -h, h, g)
    dyc = dy.permute(0, 3, 1, 2)
    assert_exact_domain(conv_bound(dyc, wt, stride=(1, 2), transposed=True), wt, dy)
    ref = F.conv_transpose2d(dyc.double(), wt.double(), stride=(1, 2))  # (n, cin, 1, 2 * (W2 - 1) + kw)
    ref = F.pad(ref, (0, W1 - ref.shape[-1]))[:, :, 0].permute(0, 2, 1).reshape(n * W1, cin)
    tdy = dy.to(dt).contiguous().to(cuda)
    wpar = K.pack_weight(wt.contiguous().to(cuda), cd, 2).view(2, -1)
    dx = torch.full((n * W1, cin), NAN, dtype=F32, device=cuda)
    for par in (0, 1):
        Tp = (W1 - par + 1) // 2
        A = K.conv(tdy, L.KC, n, 1, W2, cout, 1, Tp, 1, kw // 2, pw=kw // 2 - 1)
        Bo = K.dense(wpar[par], L.KC, cin, 512)
        if cd == L.BF16:
            assert _path(A, Bo, n * Tp, cin, 512, 1) == 1
        K.gemm(A, Bo, K.epilogue(dx, cin, rowmap=(Tp, W1, 2, par)), n * Tp, cin, 512, cd, split_k=1)
    torch.cuda.synchronize()
    assert_bit_equal(dx.cpu(), ref, F32, "parity dgrad row map")


# ------------------------------------------------------------------------------------ path 7
@pytest.mark.parametrize("epi", ["plain_f32", "bias_bf16", "add_aux_f32", "dact_mul_colsum"])
def test_path7_epilogues(cuda, epi):
    """The smallest grid the 256x256 kernel accepts (9 x 4 tiles, M with an 8-row tail tile), K = 128."""
    M, N, Kd = 2048 + 8, 1024, 128
    g = _gen(7, len(epi))
    a, b = _ab(M, N, Kd, g)
    bias = int_tensor((N,), -8, 8, g)
    A, Bo = _operand(a, L.KC, cuda, BF16), _operand(b, L.KC, cuda, BF16)
    assert _path(A, Bo, M, N, Kd, 1) == 7
    z = a.double() @ b.double().t()
    tb = bias.to(cuda)
    if epi == "plain_f32":
        assert_exact_domain(gemm_bound(a, b), a, b)
        out = torch.full((M, N), NAN, dtype=F32, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N), M, N, Kd, L.BF16)
        ref = z
    elif epi == "bias_bf16":
        assert_exact_domain(gemm_bound(a, b, bias), a, b, bias)
        out = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, bias=tb), M, N, Kd, L.BF16)
        ref = z + bias.double()
    elif epi == "add_aux_f32":
        res = int_tensor((M, N), -8, 8, g)
        assert_exact_domain(gemm_bound(a, b, bias, res), a, b, bias, res)
        out = torch.full((M, N), NAN, dtype=F32, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, act=L.ACT_ADD_AUX, bias=tb, aux=res.to(cuda), ldaux=N), M, N, Kd, L.BF16)
        ref = z + bias.double() + res.double()
    else:
        # The documented rounding rule of this kernel (csrc/mgemm.hip header, DESIGN.md "Rounding of the 256x256
        # kernel's bf16 epilogues"): a bf16 output is rounded as autocast rounds a Linear's output BEFORE its
        # activation backward, so DACT_MUL stores bf16(bf16(acc) * aux) -- two roundings, where the epi_store of
        # paths 0 and 5 stores bf16(acc * aux) (test_linear_epilogues[dact_mul]).  That rule is asserted
        # exactly: bf16(acc) * aux is exact in f32 (8 bits x 4 bits), and the case must tell the two rules apart.
        d = int_tensor((M, N), -8, 8, g, BF16)
        assert_exact_domain(gemm_bound(a, b, factor=8.0), a, b, d)
        out = torch.full((M, N), NAN, dtype=BF16, device=cuda)
        cs = torch.full((N,), NAN, device=cuda)
        K.gemm(A, Bo, K.epilogue(out, N, act=L.DACT_MUL, aux=d.to(cuda), ldaux=N, colsum=cs), M, N, Kd, L.BF16)
        ref = z.float().to(BF16).double() * d.double()
        once = (z * d.double()).float().to(BF16)
        assert bool((ref.float().to(BF16) != once).any()), "the case does not tell the two rounding rules apart"
        stored = ref.float().to(BF16).double()
        assert float(stored.abs().sum(0).max()) < 2 ** 24
        torch.cuda.synchronize()
        assert_bit_equal(cs.cpu(), stored.sum(0), F32, "path 7 dact_mul column sums")
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, out.dtype, f"path 7 {epi}")


@pytest.mark.parametrize("odt", [F32, BF16])
def test_path7_ragged_n(cuda, odt):
    """N % 8 == 4 with a k-contiguous B: an f32 output stays on the 256x256 kernel (4 columns per lane), a bf16
    output must leave it (mia_gemm_path probes with a bf16 epilogue: 5); exact either way, nothing past N."""
    M, N, Kd = 2048 + 8, 1028, 128
    g = _gen(77)
    a, b = _ab(M, N, Kd, g)
    assert_exact_domain(gemm_bound(a, b), a, b)
    A, Bo = _operand(a, L.KC, cuda, BF16), _operand(b, L.KC, cuda, BF16)
    assert _path(A, Bo, M, N, Kd, 1) == 5
    assert _path(A, _operand(b[:1024], L.KC, cuda, BF16), M, 1024, Kd, 1) == 7  # the same grid at N % 8 == 0
    ref = a.double() @ b.double().t()
    full, out = _guarded(M, N, N + 12, odt, cuda)
    K.gemm(A, Bo, K.epilogue(out, N + 12), M, N, Kd, L.BF16)
    out2 = torch.full((M, N), NAN, dtype=odt, device=cuda)  # ldc = N: the columns past a row's end are the next row
    K.gemm(A, Bo, K.epilogue(out2, N), M, N, Kd, L.BF16)
    torch.cuda.synchronize()
    _assert_untouched(full, M, N, "path 7 ragged N")
    assert_bit_equal(out.cpu().contiguous(), ref, odt, f"path 7 ragged N, ldc > N, {odt}")
    assert_bit_equal(out2.cpu(), ref, odt, f"path 7 ragged N, ldc = N, {odt}")


@pytest.mark.parametrize("Kd", [16384 + 64, 16384 + 72])
def test_path7_long_k_wgrad(cuda, Kd):
    """The weight-gradient form (both operands k-by-m, M and N just above one tile, long K): the kernel's own
    split-K into f32 slabs and the A column sums; K a multiple of 64 and not."""
    M, N = 264, 264
    g = _gen(79, Kd)
    a, b = _ab(M, N, Kd, g)
    assert_exact_domain(gemm_bound(a, b), a, b)
    assert float(a.abs().sum(1).max()) < 2 ** 24
    A, Bo = _operand(a, L.RC, cuda, BF16), _operand(b, L.RC, cuda, BF16)
    assert _path(A, Bo, M, N, Kd, 1) == 7
    ref = a.double() @ b.double().t()
    full, out = _guarded(M, N, N + 64, F32, cuda)
    cs = torch.full((M,), NAN, device=cuda)
    K.gemm(A, Bo, K.epilogue(out, N + 64, a_colsum=cs), M, N, Kd, L.BF16)
    outb = torch.full((M, N), NAN, dtype=BF16, device=cuda)
    K.gemm(A, Bo, K.epilogue(outb, N), M, N, Kd, L.BF16)
    torch.cuda.synchronize()
    _assert_untouched(full, M, N, "path 7 long K")
    assert_bit_equal(out.cpu().contiguous(), ref, F32, "path 7 long K f32")
    assert_bit_equal(cs.cpu(), a.double().sum(1), F32, "path 7 a_colsum")
    assert_bit_equal(outb.cpu(), ref, BF16, "path 7 long K bf16")


# ------------------------------------------------------------------------------------ paths 1-4 (conv gathers)
def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _conv_inputs(g, n, cin, cout, h, w, kh, kw, pre):
    hi = operand_hi(kh * kw * cin)
    x = int_tensor((n, h, w, cin), -hi, hi, g)
    wt = int_tensor((cout, cin, kh, kw), -hi, hi, g)
    sc, sh = pre_affine(cin, g)
    xin = torch.relu(x * sc + sh) if pre else x
    return x, wt, sc, sh, xin


@pytest.mark.parametrize("store", [BF16, F32])
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("case", [(2, 32, 32, 9, 300, 8, 8, 1), (2, 32, 64, 1, 601, 1, 16, 2),
                                  (2, 64, 32, 2, 555, 1, 8, 1)])
def test_path1_rowconv(cuda, case, pre, store):
    n, cin, cout, h, w, kh, kw, sw = case
    g = _gen(1, h, w, cin, cout, pre)
    x, wt, sc, sh, xin = _conv_inputs(g, n, cin, cout, h, w, kh, kw, pre)
    bias = int_tensor((cout,), -8, 8, g)
    assert_exact_domain(conv_bound(_nchw(xin), wt, bias, stride=(1, sw)), x, xin, wt, sc, sh, bias)
    oh, ow = h - kh + 1, (w - kw) // sw + 1
    P, Kd = n * oh * ow, kh * kw * cin
    z = F.conv2d(_nchw(xin).double(), wt.double(), stride=(1, sw)).permute(0, 2, 3, 1).reshape(P, cout)
    wp = K.pack_weight(wt.contiguous().to(cuda), L.BF16, 0)
    A = K.conv(x.to(store).contiguous().to(cuda), L.KC, n, h, w, cin, oh, ow, kh, kw, sw=sw,
               pre=L.PRE_AFFINE_RELU if pre else L.PRE_NONE, scale=sc.to(cuda), shift=sh.to(cuda))
    Bo = K.dense(wp, L.KC, cout, Kd)
    assert _path(A, Bo, P, cout, Kd, 1) == 1
    out = torch.full((P, cout), NAN, dtype=F32, device=cuda)
    K.gemm(A, Bo, K.epilogue(out, cout), P, cout, Kd, L.BF16, split_k=1)
    outb = torch.full((P, cout), NAN, dtype=BF16, device=cuda)
    K.gemm(A, Bo, K.epilogue(outb, cout, bias=bias.to(cuda)), P, cout, Kd, L.BF16, split_k=1)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), z, F32, "row conv f32")
    assert_bit_equal(outb.cpu(), z + bias.double(), BF16, "row conv bf16 + bias")


def test_path1_padded_dgrad(cuda):
    """conv4 backward-data through the row-window kernel: dY zero-padded by 7 against the flipped weights."""
    n, cin, cout, h, w, kh, kw = 2, 32, 32, 12, 300, 8, 8
    oh, ow = h - kh + 1, w - kw + 1
    g = _gen(11)
    wt = int_tensor((cout, cin, kh, kw), -3, 3, g)
    dy = int_tensor((n, oh, ow, cout), -3, 3, g)
    assert_exact_domain(conv_bound(_nchw(dy), wt, transposed=True), wt, dy)
    ref = F.conv_transpose2d(_nchw(dy).double(), wt.double()).permute(0, 2, 3, 1).reshape(n * h * w, cin)
    wf = K.pack_weight(wt.contiguous().to(cuda), L.BF16, 1)
    A = K.conv(dy.to(BF16).contiguous().to(cuda), L.KC, n, oh, ow, cout, h, w, kh, kw, ph=kh - 1, pw=kw - 1)
    Bo = K.dense(wf, L.KC, cin, kh * kw * cout)
    assert _path(A, Bo, n * h * w, cin, kh * kw * cout, 1) == 1
    for odt in (F32, BF16):
        dx = torch.full((n * h * w, cin), NAN, dtype=odt, device=cuda)
        K.gemm(A, Bo, K.epilogue(dx, cin), n * h * w, cin, kh * kw * cout, L.BF16, split_k=1)
        torch.cuda.synchronize()
        assert_bit_equal(dx.cpu(), ref, odt, f"row conv padded dgrad {odt}")


def _wgrad_ref(xin_nchw, dy_nchw, wshape, stride=(1, 1)):
    """float64 weight gradient in OHWI order, flattened (cout, kh * kw * cin)."""
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin_nchw.double(), w, stride=stride).backward(dy_nchw.double())
    return w.grad.permute(0, 2, 3, 1).reshape(wshape[0], -1)


def _rowwgrad(cuda, case, pre, store):
    n, cin, cout, h, w, kh, kw, sw = case
    g = _gen(2, h, w, cin, cout)
    oh, ow = h - kh + 1, (w - kw) // sw + 1
    x = int_tensor((n, h, w, cin), -3, 3, g)
    dy = int_tensor((n, oh, ow, cout), -3, 3, g)
    sc, sh = pre_affine(cin, g)
    xin = torch.relu(x * sc + sh) if pre else x
    wshape = (cout, cin, kh, kw)
    assert_exact_domain(float(_wgrad_ref(_nchw(xin).abs(), _nchw(dy).abs(), wshape, (1, sw)).max()), x, xin, dy, sc, sh)
    ref = _wgrad_ref(_nchw(xin), _nchw(dy), wshape, (1, sw))
    P, Kc = n * oh * ow, kh * kw * cin
    A = K.dense(dy.to(store).contiguous().to(cuda), L.RC, P, cout)
    Bo = K.conv(x.to(store).contiguous().to(cuda), L.RC, n, h, w, cin, oh, ow, kh, kw, sw=sw,
                pre=L.PRE_AFFINE_RELU if pre else L.PRE_NONE, scale=sc.to(cuda), shift=sh.to(cuda))
    assert _path(A, Bo, cout, Kc, P, 2) == 2
    dW = torch.full((cout, Kc), NAN, dtype=F32, device=cuda)
    K.gemm(A, Bo, K.epilogue(dW, Kc), cout, Kc, P, L.BF16)
    torch.cuda.synchronize()
    assert_bit_equal(dW.cpu(), ref, F32, "row-window wgrad")


@pytest.mark.parametrize("case,pre,store", [((3, 32, 64, 4, 300, 1, 4, 1), True, BF16),
                                            ((2, 32, 32, 9, 333, 8, 8, 1), False, F32),
                                            ((2, 32, 32, 1, 901, 1, 16, 2), False, BF16)])
def test_path2_rowwgrad(cuda, case, pre, store):
    _rowwgrad(cuda, case, pre, store)


def test_path2_wgrad8(cuda):
    """The rolling-window special case (M = 32, c = 32, 8x8, bf16, BN+ReLU pre-op): ow = 293 is two whole
    128-pixel chunks and a 37-pixel tail."""
    _rowwgrad(cuda, (2, 32, 32, 12, 300, 8, 8, 1), True, BF16)


@pytest.mark.parametrize("dydt", [BF16, F32])
def test_path3_tapwgrad_conv1(cuda, dydt):
    n, T = 3, 2 * 701 + 64
    W1 = (T - 64) // 2 + 1
    g = _gen(3, 1)
    x = int_tensor((n, T), -3, 3, g)
    dy = int_tensor((n, W1, 32), -3, 3, g)
    xc, dyc = x.view(n, 1, 1, T), dy.permute(0, 2, 1).unsqueeze(2)
    assert_exact_domain(float(_wgrad_ref(xc.abs(), dyc.abs(), (32, 1, 1, 64), (1, 2)).max()), x, dy)
    ref = _wgrad_ref(xc, dyc, (32, 1, 1, 64), (1, 2))
    A = K.dense(dy.to(dydt).contiguous().to(cuda), L.RC, n * W1, 32)
    Bo = K.conv(x.to(cuda), L.RC, n, 1, T // 2, 2, 1, W1, 1, 32, row_kind=True)
    assert _path(A, Bo, 32, 64, n * W1, 2) == 3
    dW = torch.full((32, 64), NAN, dtype=F32, device=cuda)
    K.gemm(A, Bo, K.epilogue(dW, 64), 32, 64, n * W1, L.BF16)
    torch.cuda.synchronize()
    assert_bit_equal(dW.cpu(), ref, F32, "tap wgrad conv1")


@pytest.mark.parametrize("xdt", [BF16, F32])
@pytest.mark.parametrize("dydt", [BF16, F32])
def test_path3_tapwgrad_conv3(cuda, dydt, xdt):
    n, H, W = 2, 12, 300
    ha, wa = H - 7, W - 7
    g = _gen(3, 3)
    x = int_tensor((n, H, W), -3, 3, g)
    dy = int_tensor((n, ha, wa, 32), -3, 3, g)
    assert_exact_domain(float(_wgrad_ref(x.unsqueeze(1).abs(), _nchw(dy).abs(), (32, 1, 8, 8)).max()), x, dy)
    ref = _wgrad_ref(x.unsqueeze(1), _nchw(dy), (32, 1, 8, 8))
    A = K.dense(dy.to(dydt).contiguous().to(cuda), L.RC, n * ha * wa, 32)
    Bo = K.conv(x.to(xdt).contiguous().to(cuda), L.RC, n, H, W, 1, ha, wa, 8, 8, row_kind=True)
    assert _path(A, Bo, 32, 64, n * ha * wa, 2) == 3
    dW = torch.full((32, 64), NAN, dtype=F32, device=cuda)
    K.gemm(A, Bo, K.epilogue(dW, 64), 32, 64, n * ha * wa, L.BF16)
    torch.cuda.synchronize()
    assert_bit_equal(dW.cpu(), ref, F32, "tap wgrad conv3")


@pytest.mark.parametrize("odt", [BF16, F32])
def test_path4_tapconv_conv1(cuda, odt):
    n, T = 3, 2 * 701 + 64
    W1 = (T - 64) // 2 + 1
    g = _gen(4, 1)
    hi = operand_hi(64)
    x = int_tensor((n, T), -hi, hi, g)
    wt = int_tensor((32, 1, 1, 64), -hi, hi, g)
    bias = int_tensor((32,), -8, 8, g)
    assert_exact_domain(conv_bound(x.view(n, 1, 1, T), wt, bias, stride=(1, 2)), x, wt, bias)
    ref = F.conv2d(x.double().view(n, 1, 1, T), wt.double(), bias.double(), stride=(1, 2))
    ref = ref[:, :, 0].permute(0, 2, 1).reshape(n * W1, 32)
    wp = K.pack_weight(wt.contiguous().to(cuda), L.BF16, 0)
    A = K.conv(x.to(cuda), L.KC, n, 1, T // 2, 2, 1, W1, 1, 32, row_kind=True)
    Bo = K.dense(wp, L.KC, 32, 64)
    assert _path(A, Bo, n * W1, 32, 64, 1) == 4
    out = torch.full((n * W1, 32), NAN, dtype=odt, device=cuda)
    K.gemm(A, Bo, K.epilogue(out, 32, bias=bias.to(cuda)), n * W1, 32, 64, L.BF16, split_k=1)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, odt, "tap conv conv1")


@pytest.mark.parametrize("xdt", [BF16, F32])
@pytest.mark.parametrize("odt", [BF16, F32])
def test_path4_tapconv_conv3(cuda, odt, xdt):
    n, H, W = 2, 12, 300
    ha, wa = H - 7, W - 7
    g = _gen(4, 3)
    hi = operand_hi(64)
    x = int_tensor((n, H, W), -hi, hi, g)
    wt = int_tensor((32, 1, 8, 8), -hi, hi, g)
    bias = int_tensor((32,), -8, 8, g)
    assert_exact_domain(conv_bound(x.unsqueeze(1), wt, bias), x, wt, bias)
    ref = F.conv2d(x.double().unsqueeze(1), wt.double(), bias.double()).permute(0, 2, 3, 1).reshape(-1, 32)
    wp = K.pack_weight(wt.contiguous().to(cuda), L.BF16, 0)
    A = K.conv(x.to(xdt).contiguous().to(cuda), L.KC, n, H, W, 1, ha, wa, 8, 8, row_kind=True)
    Bo = K.dense(wp, L.KC, 32, 64)
    assert _path(A, Bo, n * ha * wa, 32, 64, 1) == 4
    out = torch.full((n * ha * wa, 32), NAN, dtype=odt, device=cuda)
    K.gemm(A, Bo, K.epilogue(out, 32, bias=bias.to(cuda)), n * ha * wa, 32, 64, L.BF16, split_k=1)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, odt, "tap conv conv3")


# ------------------------------------------------------------------------------------ dedicated conv kernels
def _fe_conv2_inputs(n, w1, pre, seed):
    g = _gen(seed, n, w1, pre)
    h = operand_hi(512)
    y1 = int_tensor((n, w1, 32), -h, h, g)
    W = int_tensor((64, 32, 1, 16), -h, h, g)
    sc, sh = pre_affine(32, g)
    a = torch.relu(y1 * sc + sh) if pre else y1
    return g, h, y1, W, sc, sh, a


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("n,w1", [(1, 300), (3, 4112)])
def test_fe_conv2_fwd(cuda, n, w1, pre):
    w2 = (w1 - 16) // 2 + 1
    g, h, y1, W, sc, sh, a = _fe_conv2_inputs(n, w1, pre, 20)
    bias = int_tensor((64,), -8, 8, g)
    ac = a.permute(0, 2, 1).unsqueeze(2)  # (n, 32, 1, w1)
    assert_exact_domain(conv_bound(ac, W, bias, stride=(1, 2)), y1, a, W, sc, sh, bias)
    ref = F.conv2d(ac.double(), W.double(), bias.double(), stride=(1, 2))[:, :, 0].permute(0, 2, 1).reshape(n * w2, 64)
    wp = K.pack_weight(W.to(cuda), L.BF16, 0)
    out = torch.full((n * w2, 64), NAN, dtype=BF16, device=cuda)
    K.fe_conv2_fwd(y1.to(BF16).to(cuda).reshape(-1, 32), sc.to(cuda) if pre else None, sh.to(cuda) if pre else None,
                   wp, bias.to(cuda), out, n, w1, w2)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, BF16, "fe_conv2_fwd")


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("n,w1", [(1, 300), (3, 4112)])
def test_fe_conv2_wgrad(cuda, n, w1, pre):
    w2 = (w1 - 16) // 2 + 1
    g, h, y1, W, sc, sh, a = _fe_conv2_inputs(n, w1, pre, 21)
    dy = int_tensor((n, w2, 64), -3, 3, g)
    ac, dyc = a.permute(0, 2, 1).unsqueeze(2), dy.permute(0, 2, 1).unsqueeze(2)
    assert_exact_domain(float(_wgrad_ref(ac.abs(), dyc.abs(), (64, 32, 1, 16), (1, 2)).max()), y1, a, dy, sc, sh)
    ref = _wgrad_ref(ac, dyc, (64, 32, 1, 16), (1, 2))  # [co][kx][ci]
    dw = torch.full((64, 512), NAN, device=cuda)
    K.fe_conv2_wgrad(dy.to(BF16).to(cuda).reshape(-1, 64), y1.to(BF16).to(cuda).reshape(-1, 32),
                     sc.to(cuda) if pre else None, sh.to(cuda) if pre else None, dw, n, w1, w2)
    torch.cuda.synchronize()
    assert_bit_equal(dw.cpu(), ref, F32, "fe_conv2_wgrad")


def test_fe_conv2_dgrad(cuda):
    n, w1 = 3, 4112
    w2 = (w1 - 16) // 2 + 1
    g = _gen(22)
    h = operand_hi(512)
    dy = int_tensor((n, w2, 64), -h, h, g)
    W = int_tensor((64, 32, 1, 16), -h, h, g)
    dyc = dy.permute(0, 2, 1).unsqueeze(2)
    assert_exact_domain(conv_bound(dyc, W, stride=(1, 2), transposed=True), dy, W)
    ref = F.conv_transpose2d(dyc.double(), W.double(), stride=(1, 2))[:, :, 0]
    ref = F.pad(ref, (0, w1 - ref.shape[-1])).permute(0, 2, 1).reshape(n * w1, 32)  # unreached pixels: zero gradient
    wpar = K.pack_weight(W.to(cuda), L.BF16, 2)
    out = torch.full((n * w1, 32), NAN, dtype=BF16, device=cuda)
    K.fe_conv2_dgrad(dy.to(BF16).to(cuda).reshape(-1, 64), wpar, out, n, w1, w2)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, BF16, "fe_conv2_dgrad")


def test_fe_conv1_fwd(cuda):
    n, t = 2, 9000
    w1 = (t - 64) // 2 + 1
    g = _gen(23)
    h = operand_hi(64)
    x = int_tensor((n, t), -h, h, g)
    W = int_tensor((32, 1, 1, 64), -h, h, g)
    bias = int_tensor((32,), -8, 8, g)
    assert_exact_domain(conv_bound(x.view(n, 1, 1, t), W, bias, stride=(1, 2)), x, W, bias)
    ref = F.conv2d(x.double().view(n, 1, 1, t), W.double(), bias.double(), stride=(1, 2))
    ref = ref[:, :, 0].permute(0, 2, 1).reshape(n * w1, 32)
    wp = K.pack_weight(W.to(cuda), L.BF16, 0)
    y1 = torch.full((n * w1, 32), NAN, dtype=BF16, device=cuda)
    K.fe_conv1_fwd(x.to(cuda), wp, bias.to(cuda), y1, n, t, stats=True)
    torch.cuda.synchronize()
    assert_bit_equal(y1.cpu(), ref, BF16, "fe_conv1_fwd")


def test_fe_conv3_fwd(cuda):
    n, h, wd = 5, 12, 100
    oh, ow = h - 7, wd - 7
    g = _gen(24)
    hi = operand_hi(64)
    x = int_tensor((n, h, wd), -hi, hi, g)
    W = int_tensor((32, 1, 8, 8), -hi, hi, g)
    bias = int_tensor((32,), -8, 8, g)
    assert_exact_domain(conv_bound(x.unsqueeze(1), W, bias), x, W, bias)
    ref = F.conv2d(x.double().unsqueeze(1), W.double(), bias.double()).permute(0, 2, 3, 1).reshape(n * oh * ow, 32)
    wp = K.pack_weight(W.to(cuda), L.BF16, 0)
    y = torch.full((n * oh * ow, 32), NAN, dtype=BF16, device=cuda)
    K.fe_conv3_fwd(x.to(BF16).to(cuda), wp, bias.to(cuda), y, n, h, wd, stats=True)
    torch.cuda.synchronize()
    assert_bit_equal(y.cpu(), ref, BF16, "fe_conv3_fwd")


@pytest.mark.parametrize("n,h,wd", [(2, 9, 12), (3, 10, 40)])
def test_trunk_conv8_fwd(cuda, n, h, wd):
    oh, ow = h - 7, wd - 7
    g = _gen(25, n, h, wd)
    x, W, sc, sh, xin = _conv_inputs(g, n, 32, 32, h, wd, 8, 8, True)
    bias = int_tensor((32,), -8, 8, g)
    assert_exact_domain(conv_bound(_nchw(xin), W, bias), x, xin, W, sc, sh, bias)
    ref = F.conv2d(_nchw(xin).double(), W.double(), bias.double()).permute(0, 2, 3, 1).reshape(n * oh * ow, 32)
    wp = K.pack_weight(W.to(cuda), L.BF16, 0)
    y = torch.full((n * oh * ow, 32), NAN, dtype=BF16, device=cuda)
    K.trunk_conv8(x.to(BF16).to(cuda), wp, y, n, h, wd, scale=sc.to(cuda), shift=sh.to(cuda), bias=bias.to(cuda),
                  stats=True)
    torch.cuda.synchronize()
    assert_bit_equal(y.cpu(), ref, BF16, "trunk_conv8 forward")


def test_trunk_conv8_dgrad(cuda):
    """The same kernel in its backward-data form (dY zero-padded by 7, flipped weights); a dY map shorter than
    the kernel."""
    n, h, wd = 3, 3, 30
    g = _gen(26)
    dy = int_tensor((n, h, wd, 32), -3, 3, g)
    W = int_tensor((32, 32, 8, 8), -3, 3, g)
    assert_exact_domain(conv_bound(_nchw(dy), W, transposed=True), dy, W)
    ref = F.conv_transpose2d(_nchw(dy).double(), W.double()).permute(0, 2, 3, 1).reshape(-1, 32)
    wf = K.pack_weight(W.to(cuda), L.BF16, 1)
    dx = torch.full((n * (h + 7) * (wd + 7), 32), NAN, dtype=BF16, device=cuda)
    K.trunk_conv8(dy.to(BF16).to(cuda), wf, dx, n, h, wd, ph=7, pw=7)
    torch.cuda.synchronize()
    assert_bit_equal(dx.cpu(), ref, BF16, "trunk_conv8 backward-data")


@pytest.mark.parametrize("n,h,wd", [(1, 8, 12), (3, 9, 40)])
def test_conv3_wgrad(cuda, n, h, wd):
    oh, ow = h - 7, wd - 7
    g = _gen(27, n, h, wd)
    x = int_tensor((n, h, wd), -3, 3, g)
    dy = int_tensor((n, oh, ow, 32), -3, 3, g)
    assert_exact_domain(float(_wgrad_ref(x.unsqueeze(1).abs(), _nchw(dy).abs(), (32, 1, 8, 8)).max()), x, dy)
    ref = _wgrad_ref(x.unsqueeze(1), _nchw(dy), (32, 1, 8, 8))
    dw = torch.full((32, 64), NAN, device=cuda)
    K.conv3_wgrad(x.to(BF16).to(cuda), dy.to(BF16).to(cuda).reshape(-1, 32), dw, n, h, wd)
    torch.cuda.synchronize()
    assert_bit_equal(dw.cpu(), ref, F32, "conv3_wgrad")


def test_conv1ch_dgrad(cuda):
    n, oh, ow = 3, 10, 121
    g = _gen(28)
    dy = int_tensor((n, oh, ow, 32), -3, 3, g)
    w = int_tensor((32, 1, 8, 8), -3, 3, g)
    assert_exact_domain(conv_bound(_nchw(dy), w, transposed=True), dy, w)
    ref = F.conv_transpose2d(_nchw(dy).double(), w.double())[:, 0].contiguous()
    out = torch.full((n, oh + 7, ow + 7), NAN, dtype=BF16, device=cuda)
    K.conv1ch_dgrad(dy.to(BF16).to(cuda).reshape(-1, 32), w.to(cuda), n, oh, ow, out)
    torch.cuda.synchronize()
    assert_bit_equal(out.cpu(), ref, BF16, "conv1ch_dgrad")


def test_trunk_w2(cuda):
    """The (1, 2) conv as dense GEMMs: forward through the drop-mode row map (RM_DROP), backward in both forms
    (dY laid on the input grid + overlapping views, and the interleaved shifted copy)."""
    B, H, W, cin, cout = 3, 4, 37, 64, 128
    rows, P = B * H, B * H * W
    g = _gen(29)
    ha, hd = operand_hi(2 * cin), operand_hi(2 * cout)
    a = int_tensor((rows, W, cin), -ha, ha, g)
    dy = int_tensor((rows, W - 1, cout), -hd, hd, g)
    Wt = int_tensor((cout, cin, 1, 2), -ha, ha, g)
    bias = int_tensor((cout,), -8, 8, g)
    ac, dyc = a.permute(2, 0, 1).unsqueeze(0), dy.permute(2, 0, 1).unsqueeze(0)  # (1, c, rows, W)
    assert_exact_domain(conv_bound(ac, Wt, bias), a, Wt, bias)
    assert_exact_domain(conv_bound(dyc, Wt, transposed=True), dy)
    assert_exact_domain(float(_wgrad_ref(ac.abs(), dyc.abs(), (cout, cin, 1, 2)).max()))
    yref = F.conv2d(ac.double(), Wt.double(), bias.double())[0].permute(1, 2, 0).reshape(rows * (W - 1), cout)
    dxref = F.conv_transpose2d(dyc.double(), Wt.double())[0].permute(1, 2, 0).reshape(P, cin)
    dwref = _wgrad_ref(ac, dyc, (cout, cin, 1, 2))  # (cout, [kx][ci])
    ta = torch.empty(P + 1, cin, dtype=BF16, device=cuda)[:P]  # one pad pixel behind the map
    ta.copy_(a.reshape(P, cin))
    apad = ta.as_strided((cin,), (1,), ta.storage_offset() + P * cin)
    apad.fill_(NAN)  # read only by the dropped last output of the forward
    wpk = K.pack_weight(Wt.to(cuda), L.BF16, 0)
    assert _path(K.dense(ta, L.KC, P, 2 * cin, ld=cin), K.dense(wpk, L.KC, cout, 2 * cin), P, cout, 2 * cin, 1) == 5
    y = torch.full((rows * (W - 1), cout), NAN, dtype=BF16, device=cuda)
    K.conv_w2_fwd(ta, rows, W, cin, wpk, bias.to(cuda), y)
    tdy = dy.to(BF16).to(cuda).reshape(-1, cout)
    dw = torch.full((cout, 2 * cin), NAN, device=cuda)
    dx = torch.full((P, cin), NAN, dtype=BF16, device=cuda)
    K.trunk_bwd_w2(tdy, ta, rows, W, cout, cin, wpk, dw, dx)  # shifted-copy form
    dw2 = torch.full((cout, 2 * cin), NAN, device=cuda)
    dx2 = torch.full((P, cin), NAN, dtype=BF16, device=cuda)
    apad.fill_(NAN)  # the input-grid form zeroes the pad pixel it multiplies by a zero gradient
    K.trunk_bwd_w2(tdy, ta, rows, W, cout, cin, wpk, dw2, dx2, wflip=K.pack_weight(Wt.to(cuda), L.BF16, 1))
    torch.cuda.synchronize()
    assert_bit_equal(y.cpu(), yref, BF16, "conv_w2_fwd")
    for form, dwx, dxx in (("shifted copy", dw, dx), ("input grid", dw2, dx2)):
        assert_bit_equal(dwx.cpu(), dwref, F32, f"trunk_bwd_w2 dW, {form}")
        assert_bit_equal(dxx.cpu(), dxref, BF16, f"trunk_bwd_w2 dX, {form}")
