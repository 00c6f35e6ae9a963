"""Integer-operand exactness helpers (tests/test_gpu_exact.py, tests/test_exact_cpu.py).

With integer operands that bf16 holds exactly (|v| <= 256) every product is exact in f32, and while every
partial sum stays below 2^24 in magnitude the f32 accumulation is exact in any order, over any tiling and under
any split-K.  An f32 output must then equal the float64 reference bit for bit and a bf16 output its
round-to-nearest-even cast: one dropped, doubled or misplaced product, a stale tile, a double bias or a
truncating store changes at least one element."""
import math

import torch
import torch.nn.functional as F

EXACT_LIMIT = float(2 ** 24)
MAX_OPERAND = 256
LO, HI = -3, 3  # default operand range; operand_hi() widens it where K is short and the output is bf16


def int_tensor(shape, lo, hi, gen, dtype=torch.float32):
    """Uniform integers in [lo, hi] as f32 or bf16 (every such value with |v| <= 256 is exact in both)."""
    assert dtype in (torch.float32, torch.bfloat16) and -MAX_OPERAND <= lo <= hi <= MAX_OPERAND
    return torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=gen.device).to(dtype)


def operand_hi(k, sigma=150.0):
    """Smallest h >= 3 for which a K-term product sum of operands uniform in [-h, h] has a standard deviation of
    at least ``sigma``: var(operand) = h(h+1)/3, so std(C) = sqrt(K) h(h+1)/3.  With sigma = 150 a few hundred
    outputs already reach [256, 1024), where bf16 spaces integers by 2 and 4 -- the store's rounding and its
    ties are then exercised.  [-3, 3] as soon as K >= 1407."""
    h = 3
    while math.sqrt(k) * h * (h + 1) / 3.0 < sigma:
        h += 1
    return h


def pre_affine(cin, gen):
    """Pre-op scale in {1, 2} and shift in {-2 .. 2} as floats: relu(x * s + t) of an integer x is an integer."""
    return int_tensor((cin,), 1, 2, gen), int_tensor((cin,), -2, 2, gen)


def gemm_bound(a, b, *addends, factor=1.0):
    """Float64 magnitude bound of C = A B^T (+ addends) for logical a [M][K], b [N][K]: (|A| |B|^T).max() plus
    the maxima of |bias| / |aux| / |base|, times ``factor`` (act_scale, or the largest |aux| of a DACT_MUL)."""
    bound = float((a.double().abs() @ b.double().abs().t()).max())
    bound += sum(float(t.double().abs().max()) for t in addends if t is not None)
    return bound * float(factor)


def conv_bound(x_nchw, w, *addends, stride=(1, 1), padding=(0, 0), factor=1.0, transposed=False):
    """The same bound for a convolution: |x| and |w| through conv2d (conv_transpose2d for a backward-data)."""
    xa, wa = x_nchw.double().abs(), w.double().abs()
    y = F.conv_transpose2d(xa, wa, stride=stride) if transposed else F.conv2d(xa, wa, stride=stride, padding=padding)
    bound = float(y.max()) + sum(float(t.double().abs().max()) for t in addends if t is not None)
    return bound * float(factor)


def assert_exact_domain(abs_sum_bound, *inputs):
    """The case stays in the exact domain: magnitude bound < 2^24 and every input an integer with |v| <= 256 (so
    its bf16 cast is the identity).  Runs on the CPU before the launch: a failure here is a broken test case,
    not a kernel failure."""
    assert abs_sum_bound < EXACT_LIMIT, f"exact domain: magnitude bound {abs_sum_bound:.0f} >= 2^24"
    for i, t in enumerate(inputs):
        if t is None:
            continue
        v = t.detach().double()
        assert bool((v == v.round()).all()), f"exact domain: input {i} holds a non-integer"
        assert float(v.abs().max()) <= MAX_OPERAND, f"exact domain: input {i} exceeds |v| <= {MAX_OPERAND}"
        assert torch.equal(v.to(torch.bfloat16).double(), v), f"exact domain: input {i} is not exact in bf16"


def is_bf16_tie(ref64):
    """Integers halfway between two bf16 neighbours: odd in [256, 512), or = 2 mod 4 in [512, 1024)."""
    r = ref64.abs()
    return ((r >= 256) & (r < 512) & (r % 2 == 1)) | ((r >= 512) & (r < 1024) & (r % 4 == 2))


def assert_bit_equal(got, ref64, out_dtype, what):
    """``got`` equals the float64 reference cast to ``out_dtype`` (float64 -> f32 -> bf16 is round-to-nearest-
    even; integers below 2^24 pass through f32 unchanged), bit for bit.  A mismatch reports the count, the
    bounding box of the differing (row, col) indices and the first five (index, got, want) triples.  A bf16
    reference must itself hold a value that needs rounding and an exact tie, else the case would not test the
    store's rounding."""
    assert ref64.dtype == torch.float64 and got.dtype == out_dtype, (what, got.dtype, ref64.dtype)
    assert float(ref64.abs().max()) < EXACT_LIMIT, f"{what}: reference leaves the exact domain"
    ref64 = ref64.to(got.device)
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs reference {tuple(ref64.shape)}"
    ref = ref64.to(torch.float32).to(out_dtype)
    if out_dtype == torch.bfloat16:
        assert bool((ref.double() != ref64).any()), f"{what}: no reference value needs bf16 rounding"
        assert bool(is_bf16_tie(ref64).any()), f"{what}: no reference value is an exact bf16 tie"
    if torch.equal(got, ref):
        return
    g2 = got.reshape(-1, got.shape[-1]) if got.dim() > 1 else got.reshape(1, -1)
    r2 = ref.reshape(g2.shape)
    bad = ~((g2 == r2) | (torch.isnan(g2) & torch.isnan(r2)))
    idx = bad.nonzero()
    rows, cols = idx[:, 0], idx[:, 1]
    first = [((int(r), int(c)), float(g2[r, c]), float(r2[r, c])) for r, c in idx[:5].tolist()]
    raise AssertionError(
        f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact reference; rows "
        f"[{int(rows.min())}, {int(rows.max())}] x cols [{int(cols.min())}, {int(cols.max())}] of "
        f"{tuple(g2.shape)}; first (index, got, want): {first}")
