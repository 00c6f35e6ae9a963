"""GPU: the two forms of mia_pool_fwd and mia_pool_bwd_gather compute the same bits.

The default forms (compile-time (1, 2) / (5, 3) windows, channel-major outputs written through an LDS transpose,
the channel-major pooled gradient staged through LDS) and the MIA_POOL_V1=1 forms run on the same inputs; every
output must be `torch.equal` -- the arithmetic is the same, only where and when values are loaded or stored
differs.  So that both cannot be wrong together, the default form is also compared with a plain torch statement:
max_pool2d (with indices) of relu(scale * x + shift) after the same rounding for the forward, the masked pooled
gradient and its float64 channel sums for the backward.

Geometries: every (layout, window, C) combination EnvNet uses plus the run-time-window fallback, at the smallest
sizes that still leave a partly filled 64-cell tile and leftover pixels."""
import pytest
import torch
import torch.nn.functional as F

from src.miaudio import kernels as K
from src.miaudio import lib as L

pytestmark = pytest.mark.gpu

#        n  H   W            C    kh kw  layout
FWD = [(3, 2, 67, 256, 1, 2, 2),           # last trunk pool: OW = 33, one column left over
       (2, 10, 11, 32, 5, 3, 0),           # first trunk pool
       (2, 1, 64 * 5 + 62, 64, 1, 64, 1),  # frontend pool: OW = 5, the tile partly filled
       (1, 3, 7, 8, 2, 3, 0)]              # run-time window
# the same geometries under every layout they allow (layout 1 needs OH == 1)
BWD = [(3, 2, 67, 256, 1, 2, 2), (3, 2, 67, 256, 1, 2, 0),
       (2, 10, 11, 32, 5, 3, 0), (2, 10, 11, 32, 5, 3, 2),
       (2, 1, 64 * 5 + 62, 64, 1, 64, 1), (2, 1, 64 * 5 + 62, 64, 1, 64, 0), (2, 1, 64 * 5 + 62, 64, 1, 64, 2),
       (1, 3, 7, 8, 2, 3, 0), (1, 3, 7, 8, 2, 3, 2),
       (5, 2, 67, 256, 1, 2, 2),           # 165 cells: a ragged last block iteration (8 cells per iteration)
       (3, 1, 262, 64, 1, 2, 1)]           # 131 cells a row: 4-cell pieces that straddle two images


def _out_shape(n, oh, ow, c, layout):
    return {0: (n, oh, ow, c), 1: (n, c, ow), 2: (n, c, oh, ow)}[layout]


def _bn(c, g, dev):
    """(mean, invstd, scale, shift) with mixed-sign scales."""
    return K.BNState((torch.randn(c, generator=g) * 0.1).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev),
                     ((torch.rand(c, generator=g) - 0.3) * 1.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev))


def _fwd(x, geom, st, with_win):
    n, h, w, c, kh, kw, layout = geom
    oh, ow = h // kh, w // kw
    out = torch.full(_out_shape(n, oh, ow, c, layout), float("nan"), dtype=x.dtype, device=x.device)
    am = torch.full((n, oh, ow, c), 255, dtype=torch.uint8, device=x.device)
    win = torch.full((n, oh, ow, c), float("nan"), dtype=x.dtype, device=x.device) if with_win else None
    K.pool_fwd(x, n, h, w, c, kh, kw, st, out, layout, am, win=win)
    torch.cuda.synchronize()
    return out, am, win


def _inputs(kind, geom, dtype, g):
    n, h, w, c, kh, kw, _ = geom
    if kind == "random":
        return torch.randn(n, h, w, c, generator=g).to(dtype)
    if kind == "ties":      # every window constant: the first position must win
        return torch.full((n, h, w, c), 0.75).to(dtype)
    assert kind == "clamped"  # relu clamps every value (the shift below is -100): value 0, first position
    return torch.rand(n, h, w, c, generator=g).to(dtype)


@pytest.mark.parametrize("with_win", [True, False], ids=["win", "nowin"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("geom", FWD, ids=lambda g: "x".join(map(str, g)))
def test_pool_fwd_forms_bit_identical(cuda, monkeypatch, geom, dtype, with_win):
    n, h, w, c, kh, kw, layout = geom
    oh, ow = h // kh, w // kw
    g = torch.Generator().manual_seed(h * w + c)
    for kind in ("random", "ties", "clamped"):
        x = _inputs(kind, geom, dtype, g)
        st = _bn(c, g, cuda)
        if kind == "clamped":
            st.scale.abs_()
            st.shift.fill_(-100.0)
        monkeypatch.delenv("MIA_POOL_V1", raising=False)
        new = _fwd(x.to(cuda), geom, st, with_win)
        monkeypatch.setenv("MIA_POOL_V1", "1")
        old = _fwd(x.to(cuda), geom, st, with_win)
        monkeypatch.delenv("MIA_POOL_V1")
        for a, b, what in zip(new, old, ("out", "argmax", "win")):
            if a is not None:
                assert torch.equal(a, b), f"{kind}: {what} differs between the forms"
        # torch on the CPU: relu(scale * x + shift) in float64 rounded once to f32 (what fmaf gives), pooled with
        # indices (first maximum in row-major window order), the pooled value rounded to the output dtype
        z = torch.relu(x.double() * st.scale.cpu().double() + st.shift.cpu().double()).float()
        ref, idx = F.max_pool2d(z.permute(0, 3, 1, 2), (kh, kw), (kh, kw), return_indices=True)  # (n, c, oh, ow)
        iy, ix = idx // w, idx % w
        pos = (iy - torch.arange(oh)[None, None, :, None] * kh) * kw + (ix - torch.arange(ow)[None, None, None, :] * kw)
        ref_l = {0: ref.permute(0, 2, 3, 1), 1: ref[:, :, 0, :], 2: ref}[layout].to(dtype)
        out, am, win = new
        assert torch.equal(out.cpu(), ref_l), f"{kind}: pooled values differ from max_pool2d"
        assert torch.equal(am.cpu().long(), pos.permute(0, 2, 3, 1)), f"{kind}: argmax differs from max_pool2d"
        if win is not None:
            xw = x.permute(0, 3, 1, 2).reshape(n, c, h * w).gather(2, idx.reshape(n, c, -1)).reshape(n, c, oh, ow)
            assert torch.equal(win.cpu(), xw.permute(0, 2, 3, 1)), f"{kind}: win is not x at the argmax"


def _gather(dout, geom, am, x, st, win):
    n, h, w, c, kh, kw, layout = geom
    gm, dg, db = K.pool_bwd_gather(dout, layout, am, x, n, h, w, c, kh, kw, st, win=win)
    torch.cuda.synchronize()
    cells = n * (h // kh) * (w // kw)
    nb = max(1, min(-(-cells // (256 // (c // 8) * 2)), 1024))  # the launch grid: one (C, 2) row of partial per block
    ws = K.workspace(L.load().mia_bn_partial_bytes(n * h * w, c), x.device, "bn")
    partial = ws[: nb * c * 2 * 4].clone().view(torch.float32)
    return gm.clone(), dg.clone(), db.clone(), partial


@pytest.mark.parametrize("with_win", [True, False], ids=["win", "nowin"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("geom", BWD, ids=lambda g: "x".join(map(str, g)))
def test_pool_bwd_gather_forms_bit_identical(cuda, monkeypatch, geom, dtype, with_win):
    n, h, w, c, kh, kw, layout = geom
    oh, ow = h // kh, w // kw
    g = torch.Generator().manual_seed(h * w + c + layout)
    x = torch.randn(n, h, w, c, generator=g).to(dtype).to(cuda)
    st = _bn(c, g, cuda)
    monkeypatch.delenv("MIA_POOL_V1", raising=False)
    _, am, win = _fwd(x, geom, st, True)
    dout0 = torch.randn(_out_shape(n, oh, ow, c, layout), generator=g).to(dtype).to(cuda)
    for lead in (0, 2) if layout != 0 else (0,):
        # lead 2: the channel-major gradient starts 2 elements past an aligned address, which moves every channel
        # run's aligned 4-cell pieces (the kernel must pick them by address, not by index)
        dout = torch.cat([dout0.new_zeros(lead), dout0.flatten()])[lead:].view(dout0.shape)
        new = _gather(dout, geom, am, x, st, win if with_win else None)
        monkeypatch.setenv("MIA_POOL_V1", "1")
        old = _gather(dout, geom, am, x, st, win if with_win else None)
        monkeypatch.delenv("MIA_POOL_V1")
        for a, b, what in zip(new, old, ("gm", "dgamma", "dbeta", "partial")):
            assert torch.equal(a, b), f"lead {lead}: {what} differs between the forms"
    # plain torch: the pooled gradient per NHWC cell, masked by relu'(scale * x_win + shift); float64 channel sums
    d = dout0 if layout == 0 else dout0.view(n, c, oh, ow).permute(0, 2, 3, 1)
    d = d.reshape(n * oh * ow, c).float().cpu()
    xw = win.reshape(n * oh * ow, c).float().cpu()
    mask = xw.double() * st.scale.cpu().double() + st.shift.cpu().double() > 0
    gm_ref = torch.where(mask, d, torch.zeros_like(d))
    gm, dg, db, _ = new
    assert torch.equal(gm.cpu(), gm_ref)
    xhat = (xw - st.mean.cpu()) * st.invstd.cpu()
    dg_ref, db_ref = (gm_ref.double() * xhat.double()).sum(0), gm_ref.double().sum(0)
    scale_g = float((gm_ref.double() * xhat.double()).abs().sum(0).max().clamp_min(1e-30))
    scale_b = float(gm_ref.double().abs().sum(0).max().clamp_min(1e-30))
    # f32 chains of at most ~10 adds per thread and 64 per block combine here (the blocks are then summed in f64):
    # worst case 74 * 2^-24 = 4.4e-6 of the channel's sum of absolute terms, so 1e-5 of it bounds the error
    assert float((dg.cpu().double() - dg_ref).abs().max()) < 1e-5 * scale_g
    assert float((db.cpu().double() - db_ref).abs().max()) < 1e-5 * scale_b
