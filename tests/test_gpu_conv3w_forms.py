"""GPU: the rescheduled conv3 weight gradient + BN3 backward (conv3_wgrad_bn2_kernel, csrc/conv3w.hip: position carried
from item to item, two items of loads ahead, BN constants in registers) against the kernel before it
(MIA_C3W_V1=1, read at call time).  Same items per wave, same MFMAs, same bn_chunk arithmetic and add orders: dW,
dbias and the dY written out must be `torch.equal`.  MIA_C3W_BNLDS=1 (the new schedule with the constants read from
LDS) is held to the same.

Shapes (n, h, wd): (1, 9, 40) has one ragged second segment (ow = 33) and 4 items; (2, 12, 44) has 20; (1, 64, 860)
is one clip of the trunk's map (1539 items over the 4096 waves of the natural grid: at most one each).
MIA_C3W_GRID=1 leaves one block of four waves: (2, 12, 44) then gives every wave five items, so the ring of three
register sets wraps and ends at each of its three exits across the shapes ((3, 9, 40): three items a wave;
(1, 9, 40): one).  So that both forms cannot be wrong together, the default is also compared with float64 torch: dW of
the dY it wrote at the bound tests/test_gpu_norm.py::test_conv3_wgrad uses (1e-4 of the largest entry), dY within one
bf16 rounding of the float64 BN backward, dbias (the sum of the unrounded values) against the float64 column sums of
that reference."""
import pytest
import torch
import torch.nn.functional as F

from src.miaudio import kernels as K

pytestmark = pytest.mark.gpu

SWITCHES = ("MIA_C3W_V1", "MIA_C3W_BNLDS", "MIA_C3W_GRID")


def _inputs(cuda, n, h, wd):
    g = torch.Generator(device=cuda).manual_seed(h * 5 + wd + n)
    x = torch.randn(n, h, wd, generator=g, device=cuda).to(torch.bfloat16)
    P = n * (h - 7) * (wd - 7)
    da = torch.randn(P, 32, generator=g, device=cuda).to(torch.bfloat16)
    ya = (torch.randn(P, 32, generator=g, device=cuda) * 1.2 + 0.1).to(torch.bfloat16)
    gamma = torch.rand(32, generator=g, device=cuda) + 0.5
    gamma[3] = -gamma[3]
    beta = torch.randn(32, generator=g, device=cuda) * 0.5
    bn = K.bn_fwd_stats(ya, P, 32, gamma, beta, None, None, 0.1, 1e-5, True)
    dg, db = K.bn_relu_bwd_reduce(da, None, ya, P, 32, bn)
    return x, da, ya, gamma, bn, dg, db


def _run(inp, n, h, wd):
    x, da, ya, gamma, bn, dg, db = inp
    dy = torch.full_like(da, float("nan"))
    dw = torch.full((32, 64), float("nan"), device=x.device)
    dbias = torch.full((32,), float("nan"), device=x.device)
    K.conv3_wgrad_bn(x, da, ya, dy, dw, dbias, n, h, wd, gamma, bn, dg, db)
    torch.cuda.synchronize()
    return dw, dbias, dy


CASES = [(1, 9, 40, None), (2, 12, 44, None), (1, 64, 860, None), (1, 9, 40, 1), (2, 12, 44, 1), (3, 9, 40, 1)]


@pytest.mark.parametrize("n,h,wd,grid", CASES)
def test_conv3w_forms_bit_identical(cuda, monkeypatch, n, h, wd, grid):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    if grid:
        monkeypatch.setenv("MIA_C3W_GRID", str(grid))
    inp = _inputs(cuda, n, h, wd)
    new = _run(inp, n, h, wd)
    monkeypatch.setenv("MIA_C3W_BNLDS", "1")
    lds = _run(inp, n, h, wd)
    monkeypatch.delenv("MIA_C3W_BNLDS")
    monkeypatch.setenv("MIA_C3W_V1", "1")
    old = _run(inp, n, h, wd)
    for what, a, b, c in zip(("dW", "dbias", "dY"), new, old, lds):
        assert torch.isfinite(a.float()).all(), what
        bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(a.view(bits), b.view(bits)), f"{what} differs from the MIA_C3W_V1 form"
        assert torch.equal(a.view(bits), c.view(bits)), f"{what} differs with the BN constants in LDS"


@pytest.mark.parametrize("n,h,wd", [(1, 9, 40), (2, 12, 44), (1, 64, 860)])
def test_conv3w_default_vs_float64(cuda, monkeypatch, n, h, wd):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    inp = _inputs(cuda, n, h, wd)
    x, da, ya, gamma, bn, dg, db = inp
    dw, dbias, dy = _run(inp, n, h, wd)
    oh, ow = h - 7, wd - 7
    P = n * oh * ow
    # dW of the dY that was written, on the same bf16 operands
    w = torch.zeros(32, 1, 8, 8, dtype=torch.float64, device=cuda, requires_grad=True)
    F.conv2d(x.double()[:, None], w).backward(dy.double().view(n, oh, ow, 32).permute(0, 3, 1, 2))
    ref = w.grad.view(32, 64)
    assert float((dw.double() - ref).abs().max() / ref.abs().max()) < 1e-4
    # dY: dx = gamma * invstd * (g - dbeta / P - xhat * dgamma / P), g masked by relu'(scale * ya + shift)
    yd, gd = ya.double(), da.double()
    gd = torch.where(yd * bn.scale.double() + bn.shift.double() > 0, gd, torch.zeros_like(gd))
    xhat = (yd - bn.mean.double()) * bn.invstd.double()
    dy_ref = gamma.double() * bn.invstd.double() * (gd - db.double() / P - xhat * dg.double() / P)
    # one bf16 rounding (8-bit significand: 2^-8 relative) of a value formed in f32 by six roundings of terms of this size (each 2^-24
    # of them: 2^-20 of their sum bounds it with room)
    terms = (gamma.double() * bn.invstd.double()).abs() * (gd.abs() + db.double().abs() / P + (xhat * dg.double() / P).abs())
    assert ((dy.double() - dy_ref).abs() <= 2.0 ** -8 * dy_ref.abs() + 2.0 ** -20 * terms).all()
    # dbias sums the f32 values before their bf16 rounding (the exact ones sum to ~0 per channel: BN backward), in f32
    # chains of at most 20 adds per lane at this grid: 1e-5 of the sum of |dY| bounds the chains, the per-element
    # f32 error (above) adds up to 2^-20 of the summed terms
    tol = 1e-5 * dy_ref.abs().sum(0) + 2.0 ** -20 * terms.sum(0) + 1e-6
    assert ((dbias.double() - dy_ref.sum(0)).abs() <= tol).all()
