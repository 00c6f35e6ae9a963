"""GPU: the LEAF trunk glue kernels (csrc/leaftrunk.hip, mia_lt_*) one at a time against the float64 formulas of
tests/_leaf_model_ref.py fed each kernel's own input bits, in f32 and bf16.

Bounds (tests/test_gpu_leaf.py's): 1e-5 forward, 1e-4 gradients and reductions, on the f32 value a kernel computes.
Where a kernel stores bf16, the stored value must be the bf16 rounding of that f32 value: checked bit for bit
against the same kernel's f32 output where it has one (apply, PCEN), else within one bf16 ulp (2^-8 relative) of
the float64 value on top of the bound (the dense backward's dz).  Winners, argmax and masks are compared exactly;
a ReLU decision may differ from float64 only where |scale win + shift| < 1e-6 (|shift| + |scale win|), counted and
capped at 0.1 % of the entries.
"""
import numpy as np
import pytest
import torch

from oracle.synth import hash_uniform
from tests import _leaf_model_ref as M
from tests import _leaf_ref as R
from tests._util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(2, 9, 8, 4), (1, 4, 384, 4), (3, 11, 256, 2), (2, 6, 512, 2), (2, 37, 1024, 4)]
DTYPES = [torch.float32, torch.bfloat16]
PCEN_SHAPES = [(2, 5, 7), (1, 186, 94), (2, 128, 3)]


def _u(seed, shape, lo=-1.0, hi=1.0):
    return torch.from_numpy(hash_uniform(seed, shape, lo, hi).astype(np.float32))


def _gamma(seed, c):
    """Positive, negative and exactly zero entries in one call."""
    g = _u(seed, (c,), -1.5, 1.5)
    g[1::5] = 0.0
    return g


def _d(t):
    return t.detach().float().cpu().double()


def _chain(cuda, shape, dtype, seed, ties=False):
    """Forward chain on one map: stats -> finalize -> apply; returns everything the checks need."""
    from src.miaudio import kernels as K
    n, t, c, k = shape
    z = _u(seed, (n, t, c), -2.0, 2.0)
    if ties:
        z = torch.round(z * 2) / 2  # nine levels: every window has repeated values
    z = z.to(dtype).to(cuda)
    gamma, beta, kshift = _gamma(seed + 1, c).to(cuda), _u(seed + 2, (c,)).to(cuda), _u(seed + 3, (c,)).to(cuda)
    rm, rv = torch.zeros(c, device=cuda), torch.ones(c, device=cuda)
    win, am, part, nblk = K.lt_pool_stats(z, n, t, c, k, gamma, kshift)
    bn = K.bn_finalize_shifted(part, nblk, n * t, c, kshift, gamma, beta, rm, rv, 0.1, M.BN_EPS)
    return dict(z=z, gamma=gamma, beta=beta, kshift=kshift, rm=rm, rv=rv, win=win, am=am, bn=bn, part=part)


def _check_mask(v_ref, got_mask, scale, win, shift):
    """ReLU decisions against float64: disagreements only where the argument is within 1e-6 of cancelling."""
    bad = (v_ref > 0) != got_mask
    margin = 1e-6 * (shift.abs() + (scale * win).abs())
    assert bool((v_ref.abs()[bad] < margin.expand_as(v_ref)[bad]).all()), "a ReLU decision differs away from 0"
    n_bad = int(bad.sum())
    print(f"ReLU decisions excluded: {n_bad} of {bad.numel()}")
    assert n_bad <= 1e-3 * bad.numel()
    return bad


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("ties", [False, True], ids=["rand", "ties"])
def test_stats_winners_apply(cuda, shape, dtype, ties):
    from src.miaudio import kernels as K
    n, t, c, k = shape
    s = _chain(cuda, shape, dtype, 100 + c + t, ties)
    z, gamma = _d(s["z"]), _d(s["gamma"])
    assert bool((gamma > 0).any() and (gamma < 0).any() and (gamma == 0).any()) or c == 8
    win_r, arg_r = M.winners(z, gamma, k)
    assert torch.equal(_d(s["win"]), win_r)              # exact: the winner is one of z's own values
    assert torch.equal(s["am"].cpu().long(), arg_r)      # first occurrence on ties, position 0 for gamma == 0
    # statistics over every frame (the t % k tail included), running buffers with momentum and unbiased variance
    mean_r, var_r = M.bn_batch_stats(z)
    scale_r, shift_r, invstd_r = M.scale_shift(gamma, _d(s["beta"]), mean_r, var_r)
    bn = s["bn"]
    assert rel_err(bn.mean.cpu(), mean_r) <= 1e-4 and rel_err(bn.invstd.cpu(), invstd_r) <= 1e-4
    assert rel_err(bn.scale.cpu(), scale_r) <= 1e-4 and rel_err(bn.shift.cpu(), shift_r) <= 1e-4
    P = n * t
    assert rel_err(s["rm"].cpu(), 0.1 * mean_r) <= 1e-4
    assert rel_err(s["rv"].cpu(), 0.9 + 0.1 * var_r * P / (P - 1)) <= 1e-4
    # eval mode: the same winners without statistics
    win_e, am_e, part_e, _ = K.lt_pool_stats(s["z"], n, t, c, k, s["gamma"], None, stats=False)
    assert part_e is None and torch.equal(win_e, s["win"]) and torch.equal(am_e, s["am"])
    # apply on the kernel's own scale / shift bits
    ot = t // k
    sc, sh = _d(bn.scale), _d(bn.shift)
    out32 = K.lt_pool_apply(s["win"], n, ot, c, bn, torch.float32)
    ref = M.apply(win_r, sc, sh)
    bad = _check_mask(win_r * sc + sh, out32.cpu() > 0, sc, win_r, sh)
    assert rel_err(torch.where(bad, ref.float(), out32.cpu()), ref) <= 1e-5
    out16 = K.lt_pool_apply(s["win"], n, ot, c, bn, torch.bfloat16)
    assert torch.equal(out16, out32.to(torch.bfloat16))  # the stored bf16 is the rounding of the same f32 value


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("ot,c", [(1, 512), (43, 512), (43, 384)])
def test_time_mean(cuda, dtype, ot, c):
    from src.miaudio import kernels as K
    n = 3
    win = _u(300 + ot, (n, ot, c), -2.0, 2.0).to(dtype).to(cuda)
    bn = K.BNState(torch.zeros(c, device=cuda), torch.ones(c, device=cuda), _gamma(301, c).to(cuda),
                   _u(302, (c,), -0.5, 0.5).to(cuda))
    h = K.lt_pool_apply(win, n, ot, c, bn, torch.float32, mean=True)
    ref = M.time_mean(_d(win), _d(bn.scale), _d(bn.shift))
    assert h.shape == (n, c) and rel_err(h.cpu(), ref) <= 1e-5
    h16 = K.lt_pool_apply(win, n, ot, c, bn, torch.bfloat16, mean=True)
    assert torch.equal(h16, h.to(torch.bfloat16))
    # backward of the mean: dh / ot on every frame, masked
    dh = _u(303, (n, c)).to(dtype).to(cuda)
    bn.mean.copy_(_u(304, (c,)))
    bn.invstd.copy_(_u(305, (c,), 0.5, 2.0))
    gm, dg, db = K.lt_pool_bwd_gather(dh, win, n, ot, c, bn, mean=True)
    gm2, dg2, db2 = K.lt_pool_bwd_gather(dh, win, n, ot, c, bn, mean=True)
    assert torch.equal(gm, gm2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    gm_r, dg_r, db_r, v = M.bwd_gather(_d(dh), _d(win), _d(bn.scale), _d(bn.shift), _d(bn.mean), _d(bn.invstd), True)
    bad = _check_mask(v, gm.cpu() != 0, _d(bn.scale), _d(win), _d(bn.shift)) & (gm_r != 0)
    assert rel_err(torch.where(bad, gm_r.float(), gm.cpu()), gm_r) <= 1e-6  # dh / ot: one f32 rounding
    assert rel_err(dg.cpu(), dg_r) <= 1e-4 and rel_err(db.cpu(), db_r) <= 1e-4


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_backward_pair(cuda, shape, dtype):
    """gather at pooled size, then the dense apply with dbias, chained on the forward's own outputs; two runs of
    each give equal bits."""
    from src.miaudio import kernels as K
    n, t, c, k = shape
    ot = t // k
    s = _chain(cuda, shape, dtype, 500 + c + t)
    bn = s["bn"]
    dout = _u(600 + c, (n, ot, c)).to(dtype).to(cuda)
    gm, dg, db = K.lt_pool_bwd_gather(dout, s["win"], n, ot, c, bn)
    gm2, dg2, db2 = K.lt_pool_bwd_gather(dout, s["win"], n, ot, c, bn)
    assert torch.equal(gm, gm2) and torch.equal(dg, dg2) and torch.equal(db, db2)
    z, win = _d(s["z"]), _d(s["win"])
    sc, sh, mu, istd = _d(bn.scale), _d(bn.shift), _d(bn.mean), _d(bn.invstd)
    gm_r, _, _, v = M.bwd_gather(_d(dout), win, sc, sh, mu, istd)
    bad = _check_mask(v, gm.cpu() != 0, sc, win, sh) & (_d(dout) != 0)
    gm_k = torch.where(bad, _d(gm), gm_r)  # the kernel's decision at the excluded entries
    assert torch.equal(_d(gm), gm_k)       # exact elsewhere: gm is dout or 0
    xhat = (win - mu) * istd
    assert rel_err(dg.cpu(), (gm_k * xhat).sum((0, 1))) <= 1e-4
    assert rel_err(db.cpu(), gm_k.sum((0, 1))) <= 1e-4
    dz, dbias = K.lt_pool_bwd_apply(gm, s["am"], s["z"], n, t, c, k, s["gamma"], bn, dg, db)
    dz2, dbias2 = K.lt_pool_bwd_apply(gm, s["am"], s["z"], n, t, c, k, s["gamma"], bn, dg, db)
    assert torch.equal(dz, dz2) and torch.equal(dbias, dbias2)
    dz_r, _ = M.bwd_apply(_d(gm), s["am"].cpu().long(), z, _d(s["gamma"]), mu, istd, _d(dg), _d(db), k)
    if dtype == torch.float32:
        assert rel_err(dz.cpu(), dz_r) <= 1e-4
        tol = 1e-5
    else:
        # stored bf16: the bound on the f32 value plus one bf16 ulp of each stored element
        err = (_d(dz) - dz_r).abs()
        assert bool((err <= 2.0 ** -8 * dz_r.abs() + 1e-4 * dz_r.abs().max()).all())
        tol = 2.0 ** -8
    # dbias = sum over rows of dz: its true value is 0, bounded absolutely per channel
    lim = tol * _d(dz).abs().sum((0, 1))
    print(f"dbias: max |dbias| / (tol sum|dz|) = {float((_d(dbias).abs() / lim.clamp_min(1e-30)).max()):.3f}")
    assert bool((_d(dbias).abs() <= lim).all())
    # without dbias the same dz
    dz3, none = K.lt_pool_bwd_apply(gm, s["am"], s["z"], n, t, c, k, s["gamma"], bn, dg, db, dbias=False)
    assert none is None and torch.equal(dz3, dz)


@pytest.mark.parametrize("halo", [0, 2])
@pytest.mark.parametrize("shape", PCEN_SHAPES, ids=str)
def test_pcen_channels_last(cuda, shape, halo):
    from src.miaudio import kernels as K
    B, F, Tp = shape
    Fp = (F + 7) // 8 * 8
    P = (_u(700 + F, (B, F, Tp), 0.05, 2.0) ** 2).to(cuda)
    r, delta = _u(701, (F,), 0.3, 0.7).to(cuda), _u(702, (F,), 1.0, 3.0).to(cuda)
    y_ref = K.pcen_fwd(P, r, delta, R.EPS)
    y32 = K.lt_pcen_fwd(P, r, delta, R.EPS, torch.float32, halo=halo)
    assert y32.shape == (B, Tp + 2 * halo, Fp)
    assert torch.equal(y32[:, halo:halo + Tp, :F], y_ref.transpose(1, 2))  # bit for bit
    assert rel_err(y_ref.cpu(), R.pcen(_d(P), _d(r), _d(delta))) <= 1e-5
    y16 = K.lt_pcen_fwd(P, r, delta, R.EPS, torch.bfloat16, halo=halo)
    assert torch.equal(y16, y32.to(torch.bfloat16))
    for y in (y32, y16):
        assert not bool(y[:, :, F:].any())                                   # pad channels exactly zero
        assert not bool(y[:, :halo].any()) and not bool(y[:, halo + Tp:].any())  # halo rows exactly zero
    # backward: gy in the forward's layout; pad channels and halo rows hold junk the kernel must not read into gP
    gy = _u(703 + halo, (B, Tp + 2 * halo, Fp)).to(cuda)
    gy_t = gy[:, halo:halo + Tp, :F].transpose(1, 2).contiguous()
    gP_ref, dr_ref, dd_ref = K.pcen_bwd(P, r, delta, R.EPS, gy_t)
    gP, dr, dd = K.lt_pcen_bwd(P, r, delta, R.EPS, gy, halo=halo)
    assert torch.equal(gP, gP_ref) and torch.equal(dr, dr_ref) and torch.equal(dd, dd_ref)  # bit for bit
    gP2, dr2, dd2 = K.lt_pcen_bwd(P, r, delta, R.EPS, gy, halo=halo)
    assert torch.equal(gP, gP2) and torch.equal(dr, dr2) and torch.equal(dd, dd2)
    g64 = R.pcen_bwd(_d(P), _d(r), _d(delta), _d(gy_t))
    assert rel_err(gP.cpu(), g64[0]) <= 1e-4 and rel_err(dr.cpu(), g64[1]) <= 1e-4 and rel_err(dd.cpu(), g64[2]) <= 1e-4
    # bf16 gy: the same arithmetic on the widened values
    gy16 = gy.to(torch.bfloat16)
    a = K.lt_pcen_bwd(P, r, delta, R.EPS, gy16, halo=halo)
    b = K.lt_pcen_bwd(P, r, delta, R.EPS, gy16.float(), halo=halo)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_limits_return_error_code(cuda):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    lib = L.load()
    z = torch.zeros(2, 9, 16, device=cuda)
    g = torch.ones(16, device=cuda)
    win = torch.empty(2, 2, 16, device=cuda)
    am = torch.empty(2, 2, 16, dtype=torch.uint8, device=cuda)
    args = (z.data_ptr(), L.F32, 2, 9)
    tail = (g.data_ptr(), None, win.data_ptr(), am.data_ptr(), None, 1, L.stream_ptr())
    for c, k in ((12, 4), (1032, 4), (16, 0), (16, 10), (16, 256)):
        assert lib.mia_lt_pool_stats(*args, c, k, *tail) != 0
        assert lib.mia_last_error_string()
    assert lib.mia_lt_pool_stats(z.data_ptr(), L.F32, 2, 9, 16, 4, g.data_ptr(), None, win.data_ptr(), am.data_ptr(),
                                 None, 2000, L.stream_ptr()) != 0
    assert b"nblocks" in lib.mia_last_error_string()
    assert lib.mia_lt_pcen_fwd(z.data_ptr(), g.data_ptr(), g.data_ptr(), 1e-6, win.data_ptr(), L.F32, 1, 2000, 4, 0,
                               L.stream_ptr()) != 0
    with pytest.raises(ValueError):
        K.lt_pool_stats(torch.zeros(2, 9, 12, device=cuda), 2, 9, 12, 4, g, None)
    with pytest.raises(RuntimeError):
        K.lt_pool_stats(z, 2, 9, 16, 10, g, None)
    torch.cuda.synchronize()
