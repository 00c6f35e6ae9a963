"""GPU: the per-channel partial-sum protocol of csrc/channel_partials.h (thread -> (channel group, row slot), the
in-block fold over row slots, partial[nblk][C][2], the one-block-per-channel final pass in f64) driven through every
entry point that uses it, against float64 torch on the kernel's own input bits.

Shapes are the smallest at which the fold or the final pass can go wrong: one block, a few blocks, more than 256
blocks (the final pass's k += 256 loop), row counts that are no multiple of the row slots, C = 8 (one channel group,
256 row slots), C = 256 (8 row slots), C = 384 (48 groups: 5 row slots, 16 idle threads).  Tolerances are the ones
tests/test_gpu_norm.py and tests/test_gpu_leaftrunk.py already use for the same entry point.  Every case runs twice
and the two runs must agree bit for bit: the protocol has a fixed order of adds and no atomics.
"""
import pytest
import torch

from src.miaudio import kernels as K
from src.miaudio import lib as L
from tests import _leaf_model_ref as M
from tests._util import rel_err

pytestmark = pytest.mark.gpu

NT = 256


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _twice(run):
    """run() -> tuple of tensors; two runs give the same bits.  Returns the first run's outputs."""
    a, b = run(), run()
    torch.cuda.synchronize()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    return a


def _alternating(c, device):
    """+1 on even channels, -1 on odd ones."""
    return (1 - 2 * (torch.arange(c, device=device) % 2)).float()


def _bn_rows(C, blocks):
    """P for which nblocks_for (norm.hip) launches 1 block, 6 blocks, 257 blocks; none a multiple of rslots."""
    per = (NT // (C // 8)) * 8  # rows per block: rslots * 8
    return {"one": per - 3, "few": 5 * per + 1, "many": 256 * per + 1}[blocks]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("blocks", ["one", "few", "many"])
@pytest.mark.parametrize("C", [8, 32, 256])
def test_bn_stats_reduce_apply_row_counts(cuda, C, blocks, dt):
    """mia_bn_fwd_stats, mia_bn_relu_bwd_reduce, mia_bn_relu_bwd_apply (dbias) across the block-count classes."""
    P = _bn_rows(C, blocks)
    g = torch.Generator(device=cuda).manual_seed(1000 * C + P % 997)
    x = (torch.randn(P, C, generator=g, device=cuda) * 3 + 2).to(dt)
    dact = torch.randn(P, C, generator=g, device=cuda).to(dt)
    gamma = torch.rand(C, generator=g, device=cuda) + 0.5
    beta = torch.randn(C, generator=g, device=cuda) * 0.2

    def fwd():
        rm, rv = torch.zeros(C, device=cuda), torch.ones(C, device=cuda)
        st = K.bn_fwd_stats(x, P, C, gamma, beta, rm, rv, 0.1, 1e-5, True)
        return st.mean, st.invstd, st.scale, st.shift, rm, rv

    mean, invstd, scale, shift, rm, rv = _twice(fwd)
    xd = x.double()
    mu, var = xd.mean(0), xd.var(0, unbiased=False)
    assert rel(mean, mu) < 1e-5
    assert rel(1.0 / invstd.double() ** 2 - 1e-5, var) < 1e-4
    assert rel(rv, 0.9 + 0.1 * xd.var(0, unbiased=True)) < 1e-4

    st = K.BNState(mean, invstd, scale, shift)
    dg, db = _twice(lambda: K.bn_relu_bwd_reduce(dact, None, x, P, C, st))
    xhat = (xd - mean.double()) * invstd.double()
    gd = dact.double() * (xd * scale.double() + shift.double() > 0)
    ref_b, ref_g = gd.sum(0), (gd * xhat).sum(0)
    tol_b = 1e-5 * gd.abs().sum(0) + 1e-6
    tol_g = 1e-5 * (gd * xhat).abs().sum(0) + 1e-6
    assert ((db.double() - ref_b).abs() <= tol_b).all(), (db.double() - ref_b).abs().max()
    assert ((dg.double() - ref_g).abs() <= tol_g).all(), (dg.double() - ref_g).abs().max()

    # apply: dgamma / dbeta are inputs; ones that are not the sums of this gradient keep sum dx away from 0
    dg_in, db_in = (dg * 1.5).contiguous(), (db * 0.5).contiguous()

    def apply():
        dx = torch.empty_like(x)
        dbias = torch.empty(C, device=cuda)
        K.bn_relu_bwd_apply(dact, x, dx, P, C, gamma, st, dg_in, db_in, dbias)
        return dx, dbias

    dx, dbias = _twice(apply)
    ref_dx = gamma.double() * invstd.double() * (gd - db_in.double() / P - xhat * dg_in.double() / P)
    assert rel(dbias, ref_dx.sum(0)) < (1e-4 if dt == torch.float32 else 2e-2)


# (kh, kw) -> layout -> (n, h, w): a few thousand pooled cells, h and w no multiples of the window (layout 1 is
# (n, c, ow) and needs one pooled row)
POOL_GEOMS = {
    (1, 2): {0: (2, 3, 1001), 1: (3, 1, 2001), 2: (2, 3, 1001)},
    (5, 3): {0: (2, 23, 901), 1: (4, 7, 2102), 2: (2, 23, 901)},
    (1, 64): {0: (2, 3, 25617), 1: (3, 1, 57617), 2: (2, 3, 25617)},
}


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("kh,kw", list(POOL_GEOMS))
def test_pool_backward_sums(cuda, kh, kw, layout, dt):
    """mia_pool_bwd_gather (dgamma, dbeta) and mia_pool_bn_relu_bwd_apply (dbias): layouts 1 and 2 take the staged
    gather, bf16 takes the octet (kw = 64) and run (kw = 2, 3) apply kernels, f32 the per-pixel one."""
    n, h, w = POOL_GEOMS[(kh, kw)][layout]
    c = 32
    oh, ow = h // kh, w // kw
    g = torch.Generator(device=cuda).manual_seed(100 * kw + 10 * layout + kh)
    x = torch.randn(n, h, w, c, generator=g, device=cuda).to(dt)
    scale = torch.rand(c, generator=g, device=cuda) + 0.5
    shift = torch.randn(c, generator=g, device=cuda) * 0.3
    # a mean beyond every value of x, +6 on even and -6 on odd channels: xhat has one sign per channel and a
    # per-channel size, so sum g and sum g xhat differ in sign and magnitude and a swapped pair cannot pass
    mean = _alternating(c, cuda) * 6.0 + torch.randn(c, generator=g, device=cuda) * 0.1
    invstd = torch.rand(c, generator=g, device=cuda) * 2 + 0.5
    st = K.BNState(mean, invstd, scale, shift)
    out = torch.empty({0: (n, oh, ow, c), 1: (n, c, ow), 2: (n, c, oh, ow)}[layout], device=cuda, dtype=dt)
    am = torch.empty(n, oh, ow, c, dtype=torch.uint8, device=cuda)
    win = torch.empty(n, oh, ow, c, dtype=dt, device=cuda)
    K.pool_fwd(x, n, h, w, c, kh, kw, st, out, layout, am, win)
    dout = (torch.randn(out.shape, generator=g, device=cuda) + 0.3).to(dt)

    gm, dg, db = _twice(lambda: K.pool_bwd_gather(dout, layout, am, x, n, h, w, c, kh, kw, st, win))
    # dout as (n, oh, ow, c) cells
    dcell = (dout if layout == 0 else dout.movedim(1, -1).reshape(n, oh, ow, c)).double()
    wd = win.double()
    gm_r = dcell * (wd * scale.double() + shift.double() > 0)
    xhat_w = (wd - mean.double()) * invstd.double()
    ref_b, ref_g = gm_r.sum((0, 1, 2)), (gm_r * xhat_w).sum((0, 1, 2))
    assert torch.equal(gm.view(n, oh, ow, c).double(), gm_r)  # dout or 0
    tol = 1e-5 if dt == torch.float32 else 1e-4
    assert rel(db, ref_b) < tol and rel(dg, ref_g) < tol
    # the check can tell the two apart: per channel they differ by far more than the tolerance
    assert ((ref_g - ref_b).abs() > 100 * tol * torch.maximum(ref_g.abs().max(), ref_b.abs().max())).all()
    assert (torch.sign(ref_g) != torch.sign(ref_b)).any() and (torch.sign(ref_g) == torch.sign(ref_b)).any()

    gamma = torch.rand(c, generator=g, device=cuda) + 0.5
    dg_in, db_in = (dg * 1.5).contiguous(), (db * 0.5).contiguous()

    def apply():
        dx = torch.empty_like(x)
        dbias = torch.empty(c, device=cuda)
        K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, gamma, st, dg_in, db_in, dx, dbias)
        return dx, dbias

    dx, dbias = _twice(apply)
    # float64 restatement: gm scattered to the argmax pixel of each cell, BN backward with the given dgamma / dbeta
    gw = torch.zeros(n, oh, ow, kh * kw, c, dtype=torch.float64, device=cuda)
    gw.scatter_(3, am.long().unsqueeze(3), gm_r.unsqueeze(3))
    gfull = torch.zeros(n, h, w, c, dtype=torch.float64, device=cuda)
    gfull[:, :oh * kh, :ow * kw] = gw.view(n, oh, ow, kh, kw, c).permute(0, 1, 3, 2, 4, 5).reshape(n, oh * kh, ow * kw, c)
    P = n * h * w
    xhat = (x.double() - mean.double()) * invstd.double()
    ref_dx = gamma.double() * invstd.double() * (gfull - db_in.double() / P - xhat * dg_in.double() / P)
    assert rel(dx, ref_dx) < (1e-5 if dt == torch.float32 else 1e-2)
    assert rel(dbias, ref_dx.sum((0, 1, 2))) < 1e-4


# (n, t, c, k): one block and several blocks of mia_lt_pool_stats / _bwd_gather / _bwd_apply; t % k != 0
LT_SHAPES = [(2, 9, 8, 4), (3, 4001, 8, 4), (1, 17, 384, 4), (2, 203, 384, 4)]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LT_SHAPES, ids=str)
def test_leaf_trunk_sums(cuda, shape, dt):
    n, t, c, k = shape
    ot = t // k
    g = torch.Generator(device=cuda).manual_seed(c + t)
    z = (torch.rand(n, t, c, generator=g, device=cuda) * 4 - 2).to(dt)
    gamma = torch.rand(c, generator=g, device=cuda) * 3 - 1.5
    gamma[1::5] = 0.0
    beta = torch.rand(c, generator=g, device=cuda) * 2 - 1
    kshift = torch.rand(c, generator=g, device=cuda) * 2 - 1

    def fwd():
        win, am, part, nblk = K.lt_pool_stats(z, n, t, c, k, gamma, kshift)
        rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
        bn = K.bn_finalize_shifted(part, nblk, n * t, c, kshift, gamma, beta, rm, rv, 0.1, M.BN_EPS)
        return win, am, bn.mean, bn.invstd, bn.scale, bn.shift

    win, am, mean, invstd, scale, shift = _twice(fwd)
    blocks = int(L.load().mia_lt_stats_blocks(n, t, c, k))
    assert (blocks == 1) == (shape in (LT_SHAPES[0], LT_SHAPES[2]))
    d = lambda u: u.detach().float().cpu().double()  # noqa: E731
    mean_r, var_r = M.bn_batch_stats(d(z))
    assert rel_err(mean.cpu(), mean_r) <= 1e-4
    assert rel_err(invstd.cpu(), 1.0 / torch.sqrt(var_r + M.BN_EPS)) <= 1e-4

    # backward statistics that are not the map's own, so that sum gm and sum gm xhat differ in sign and size
    bn = K.BNState(_alternating(c, cuda) * 6.0, invstd, scale, shift)
    dout = (torch.rand(n, ot, c, generator=g, device=cuda) * 2 - 0.7).to(dt)
    gm, dg, db = _twice(lambda: K.lt_pool_bwd_gather(dout, win, n, ot, c, bn))
    gm_k = d(gm)  # dout under the kernel's own ReLU decisions (those are checked in test_gpu_leaftrunk.py)
    xhat_w = (d(win) - d(bn.mean)) * d(invstd)
    assert rel_err(dg.cpu(), (gm_k * xhat_w).sum((0, 1))) <= 1e-4
    assert rel_err(db.cpu(), gm_k.sum((0, 1))) <= 1e-4

    dg_in, db_in = (dg * 1.5).contiguous(), (db * 0.5).contiguous()
    dz, dbias = _twice(lambda: K.lt_pool_bwd_apply(gm, am, z, n, t, c, k, gamma, bn, dg_in, db_in))
    dz_r, dbias_r = M.bwd_apply(gm_k, am.cpu().long(), d(z), d(gamma), d(bn.mean), d(invstd), d(dg_in), d(db_in), k)
    tol = 1e-5 if dt == torch.float32 else 2.0 ** -8
    lim = tol * dz_r.abs().sum((0, 1))
    assert bool(((d(dbias) - dbias_r).abs() <= lim).all()), float((d(dbias) - dbias_r).abs().max())


@pytest.mark.parametrize("n,h,wd", [(1, 1, 1), (65, 2, 250)])
def test_conv8_dgrad_bn_sums(cuda, n, h, wd):
    """mia_trunk_conv8_dgrad_bn: the per-wave partial rows and the shared final pass; the second geometry gives more
    than 64 blocks (256 waves) an item."""
    g = torch.Generator(device=cuda).manual_seed(3 * h + wd + n)
    dy = torch.randn(n, h, wd, 32, generator=g, device=cuda).to(torch.bfloat16)
    W = torch.randn(32, 32, 8, 8, generator=g, device=cuda) * 0.03
    wf = K.pack_weight(W, L.BF16, 1)
    P = n * (h + 7) * (wd + 7)
    bx = (torch.randn(P, 32, generator=g, device=cuda) * 1.3 + 0.2).to(torch.bfloat16)
    bn = K.BNState(_alternating(32, cuda) * 1.5,
                   torch.rand(32, generator=g, device=cuda) * 2 + 0.5,
                   torch.rand(32, generator=g, device=cuda) + 0.5, torch.randn(32, generator=g, device=cuda) * 0.5)

    def run():
        dx = torch.full((P, 32), float("nan"), dtype=torch.bfloat16, device=cuda)
        dg, db = K.trunk_conv8_dgrad_bn(dy, wf, dx, n, h, wd, bx, bn)
        return dx, dg, db

    dx, dg, db = _twice(run)
    xd = bx.double()
    gd = dx.double() * (xd * bn.scale.double() + bn.shift.double() > 0)
    xhat = (xd - bn.mean.double()) * bn.invstd.double()
    ref_b, ref_g = gd.sum(0), (gd * xhat).sum(0)
    tol_b = 1e-5 * dx.double().abs().sum(0) + 1e-6
    tol_g = 1e-5 * (gd * xhat).abs().sum(0) + 1e-6
    assert ((db.double() - ref_b).abs() <= tol_b).all(), (db.double() - ref_b).abs().max()
    assert ((dg.double() - ref_g).abs() <= tol_g).all(), (dg.double() - ref_g).abs().max()


@pytest.mark.parametrize("n,h,wd", [(1, 8, 12), (3, 40, 104)])
def test_conv3_wgrad_bias_sum(cuda, n, h, wd):
    """mia_conv3_wgrad_bn's bias gradient: the waves' partials [nwaves][32] through the one-quantity final pass; the
    second geometry gives more than 64 blocks (256 waves) an item."""
    g = torch.Generator(device=cuda).manual_seed(h * 5 + wd + n)
    x = torch.randn(n, h, wd, generator=g, device=cuda).to(torch.bfloat16)
    P = n * (h - 7) * (wd - 7)
    da = torch.randn(P, 32, generator=g, device=cuda).to(torch.bfloat16)
    ya = (torch.randn(P, 32, generator=g, device=cuda) * 1.2 + 0.1).to(torch.bfloat16)
    gamma = torch.rand(32, generator=g, device=cuda) + 0.5
    beta = torch.randn(32, generator=g, device=cuda) * 0.5
    bn = K.bn_fwd_stats(ya, P, 32, gamma, beta, None, None, 0.1, 1e-5, True)
    dg, db = K.bn_relu_bwd_reduce(da, None, ya, P, 32, bn)
    dg_in, db_in = (dg * 1.5).contiguous(), (db * 0.5).contiguous()  # keep sum dy away from 0

    def run():
        dy = torch.empty_like(da)
        dw = torch.full((32, 64), float("nan"), device=cuda)
        dbias = torch.full((32,), float("nan"), device=cuda)
        K.conv3_wgrad_bn(x, da, ya, dy, dw, dbias, n, h, wd, gamma, bn, dg_in, db_in)
        return dy, dw, dbias

    dy, dw, dbias = _twice(run)
    yd = ya.double()
    gd = da.double() * (yd * bn.scale.double() + bn.shift.double() > 0)
    xhat = (yd - bn.mean.double()) * bn.invstd.double()
    ref_dy = gamma.double() * bn.invstd.double() * (gd - db_in.double() / P - xhat * dg_in.double() / P)
    tol = 1e-5 * ref_dy.abs().sum(0) + 1e-6
    assert ((dbias.double() - ref_dy.sum(0)).abs() <= tol).all(), (dbias.double() - ref_dy.sum(0)).abs().max()
