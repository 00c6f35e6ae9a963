"""GPU: the read-ahead form of mia_pool_bwd_gather and the gm dtype of the pooled backward (include/miaudio_pool.h).

1. Forms.  With the winners saved (win) the default form of the gather is pool_bwd_sparse_ra_kernel (NHWC dout), the
   staged pool_bwd_sparse_tr_kernel (channel-major dout from 16 cells a block iteration) or pool_bwd_sparse_kernel
   (channel-major, C = 256); MIA_POOL_V1=1 selects pool_bwd_sparse_kernel throughout, the oracle.  Both run on the
   same inputs and gm, the rows of the partial
   workspace, dgamma and dbeta must be `torch.equal`, with gm in f32 and in bf16.  MIA_POOL_GRID caps the grid, so
   that at these small shapes a thread walks more iterations than the kernel reads ahead and ends on a ragged tail.
2. gm dtype.  gm_bf16.float() is gm_f32 exactly; the apply pass fed either one writes the same dx and dbias bits in
   each of its kernels (row octets, kw-pixel runs of 2 and 3, per pixel).
3. So that both forms cannot be wrong together, the default form (bf16 gm) is compared with a float64 torch
   statement at the tolerances tests/test_gpu_pool_forms.py and tests/test_gpu_norm.py use for the same quantities.
"""
import pytest
import torch
import torch.nn.functional as F

from src.miaudio import kernels as K
from src.miaudio import lib as L

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32

#         n  H   W           kh kw
WINDOWS = [(3, 10, 3 * 7 + 1, 5, 3),    # 42 cells: fewer than rslots at C <= 64 (rslots = 2048 / C)
           (3, 2, 2 * 37 + 1, 1, 2),    # 222 cells
           (3, 10, 2 * 37 + 1, 1, 2)]   # 1110 cells: one block walks 5 (C = 32) to 139 (C = 256) iterations
GEOMS = [(n, h, w, c, kh, kw, layout) for (n, h, w, kh, kw) in WINDOWS for c in (32, 64, 128, 256)
         for layout in (0, 2)]
GEOMS.append((1, 5, 22, 256, 5, 3, 0))  # 7 cells, rslots = 8: fewer cells than row slots at every C


def _out_shape(n, oh, ow, c, layout):
    return {0: (n, oh, ow, c), 2: (n, c, oh, ow)}[layout]


def _bn(c, g, dev):
    """(mean, invstd, scale, shift) with mixed-sign scales."""
    return K.BNState((torch.randn(c, generator=g) * 0.1).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev),
                     ((torch.rand(c, generator=g) - 0.3) * 1.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev))


def _fwd(x, geom, st):
    n, h, w, c, kh, kw, _ = geom
    oh, ow = h // kh, w // kw
    out = torch.empty(n, oh, ow, c, dtype=x.dtype, device=x.device)
    am = torch.full((n, oh, ow, c), 255, dtype=torch.uint8, device=x.device)
    win = torch.full((n, oh, ow, c), float("nan"), dtype=x.dtype, device=x.device)
    K.pool_fwd(x, n, h, w, c, kh, kw, st, out, 0, am, win=win)
    return am, win


def _gather(dout, geom, am, x, st, win, gm_dtype, grid):
    n, h, w, c, kh, kw, layout = geom
    gm, dg, db = K.pool_bwd_gather(dout, layout, am, x, n, h, w, c, kh, kw, st, win=win, gm_dtype=gm_dtype)
    torch.cuda.synchronize()
    assert gm.dtype == gm_dtype
    cells = n * (h // kh) * (w // kw)
    nb = max(1, min(-(-cells // (256 // (c // 8) * 2)), 1024))  # the launch grid: one (C, 2) row of partial per block
    if grid:
        nb = min(nb, grid)
    ws = K.workspace(L.load().mia_bn_partial_bytes(n * h * w, c), x.device, "bn")
    partial = ws[: nb * c * 2 * 4].clone().view(torch.float32)
    return gm.clone(), dg.clone(), db.clone(), partial


@pytest.mark.parametrize("grid", [None, 1, 3], ids=lambda v: f"grid{v}")
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_gather_forms_bit_identical(cuda, monkeypatch, geom, dtype, grid):
    n, h, w, c, kh, kw, layout = geom
    oh, ow = h // kh, w // kw
    g = torch.Generator().manual_seed(h * w + c + layout)
    x = torch.randn(n, h, w, c, generator=g).to(dtype).to(cuda)
    st = _bn(c, g, cuda)
    for v in ("MIA_POOL_V1", "MIA_POOL_GRID", "MIA_POOL_GM32"):
        monkeypatch.delenv(v, raising=False)
    am, win = _fwd(x, geom, st)
    dout = torch.randn(_out_shape(n, oh, ow, c, layout), generator=g).to(dtype).to(cuda)
    if grid:
        monkeypatch.setenv("MIA_POOL_GRID", str(grid))
    res = {}
    for gdt in (F32, BF16) if dtype == BF16 else (F32,):
        new = _gather(dout, geom, am, x, st, win, gdt, grid)
        monkeypatch.setenv("MIA_POOL_V1", "1")
        old = _gather(dout, geom, am, x, st, win, gdt, grid)
        monkeypatch.delenv("MIA_POOL_V1")
        for a, b, what in zip(new, old, ("gm", "dgamma", "dbeta", "partial")):
            assert a.dtype == b.dtype and torch.equal(a, b), f"gm {gdt}: {what} differs between the forms"
        res[gdt] = new
    if dtype == BF16:
        assert torch.equal(res[BF16][0].float(), res[F32][0]), "bf16 gm is not the f32 gm"
        for a, b, what in zip(res[BF16][1:], res[F32][1:], ("dgamma", "dbeta", "partial")):
            assert torch.equal(a, b), f"{what} depends on gm's dtype"
    if grid:
        return
    # plain torch: the pooled gradient per NHWC cell, masked by relu'(scale * x_win + shift); float64 channel sums
    d = dout if layout == 0 else dout.permute(0, 2, 3, 1)
    d = d.reshape(n * oh * ow, c).float().cpu()
    xw = win.reshape(n * oh * ow, c).float().cpu()
    mask = xw.double() * st.scale.cpu().double() + st.shift.cpu().double() > 0
    gm_ref = torch.where(mask, d, torch.zeros_like(d))
    gm, dg, db, _ = res[dtype]  # the default: gm in x's dtype
    assert torch.equal(gm.float().cpu(), gm_ref)
    xhat = (xw - st.mean.cpu()) * st.invstd.cpu()
    dg_ref, db_ref = (gm_ref.double() * xhat.double()).sum(0), gm_ref.double().sum(0)
    scale_g = float((gm_ref.double() * xhat.double()).abs().sum(0).max().clamp_min(1e-30))
    scale_b = float(gm_ref.double().abs().sum(0).max().clamp_min(1e-30))
    # natural grid: f32 chains of 2 adds per thread and at most 64 per block (the blocks are then summed in f64):
    # 66 * 2^-24 = 3.9e-6 of the channel's sum of absolute terms, so 1e-5 of it bounds the error
    assert float((dg.cpu().double() - dg_ref).abs().max()) < 1e-5 * scale_g
    assert float((db.cpu().double() - db_ref).abs().max()) < 1e-5 * scale_b


def test_gather_default_gm_dtype(cuda, monkeypatch):
    """gm comes in x's dtype unless MIA_POOL_GM32=1 (read at call time) or the caller says otherwise."""
    geom = (1, 5, 22, 32, 5, 3, 0)
    n, h, w, c, kh, kw, layout = geom
    g = torch.Generator().manual_seed(5)
    st = _bn(c, g, cuda)
    monkeypatch.delenv("MIA_POOL_GM32", raising=False)
    for dtype in (BF16, F32):
        x = torch.randn(n, h, w, c, generator=g).to(dtype).to(cuda)
        am, win = _fwd(x, geom, st)
        dout = torch.randn(n, h // kh, w // kw, c, generator=g).to(dtype).to(cuda)
        assert K.pool_bwd_gather(dout, 0, am, x, n, h, w, c, kh, kw, st, win=win)[0].dtype == dtype
        monkeypatch.setenv("MIA_POOL_GM32", "1")
        assert K.pool_bwd_gather(dout, 0, am, x, n, h, w, c, kh, kw, st, win=win)[0].dtype == F32
        monkeypatch.delenv("MIA_POOL_GM32")
    with pytest.raises(RuntimeError):  # a bf16 gm would round an f32 gradient: refused by the library
        K.pool_bwd_gather(dout, 0, am, x, n, h, w, c, kh, kw, st, win=win, gm_dtype=BF16)
    torch.cuda.synchronize()


#          n  H   W              C    kh kw     the apply kernel the geometry takes (bf16 x)
APPLY = [(2, 1, 64 * 5 + 62, 64, 1, 64),      # row octets (kw % 8 == 0)
         (3, 2, 2 * 37 + 1, 128, 1, 2),       # runs of 2
         (3, 11, 3 * 7 + 1, 32, 5, 3),        # runs of 3, a row and a column past the last whole cell
         (2, 5, 23, 64, 2, 5)]                # per pixel (kw = 5)


@pytest.mark.parametrize("geom", APPLY, ids=lambda g: "x".join(map(str, g)))
def test_apply_reads_either_gm_dtype(cuda, monkeypatch, geom):
    n, h, w, c, kh, kw = geom
    oh, ow = h // kh, w // kw
    for v in ("MIA_POOL_V1", "MIA_POOL_GRID", "MIA_POOL_GM32"):
        monkeypatch.delenv(v, raising=False)
    g = torch.Generator().manual_seed(h * w + c)
    y = torch.randn(n, h, w, c, generator=g).to(BF16)
    scale, shift = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    mean, invstd = torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) + 0.5
    st = K.BNState(mean.to(cuda), invstd.to(cuda), scale.to(cuda), shift.to(cuda))
    x = y.to(cuda)
    am, win = _fwd(x, geom + (0,), st)
    dout = torch.randn(n, oh, ow, c, generator=g).to(BF16)
    gamma = torch.rand(c, generator=g) + 0.5
    res = {}
    for gdt in (F32, BF16):
        gm, dg, db = K.pool_bwd_gather(dout.to(cuda), 0, am, x, n, h, w, c, kh, kw, st, win=win, gm_dtype=gdt)
        dx = torch.full_like(x, float("nan"))
        dbias = torch.full((c,), float("nan"), device=cuda)
        K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, gamma.to(cuda), st, dg, db, dx, dbias)
        torch.cuda.synchronize()
        res[gdt] = (gm, dg, db, dx, dbias)
    assert torch.equal(res[BF16][0].float(), res[F32][0])
    for a, b, what in zip(res[BF16][1:], res[F32][1:], ("dgamma", "dbeta", "dx", "dbias")):
        assert torch.equal(a, b), f"{what} depends on gm's dtype"
    # float64 restatement (tests/test_gpu_norm.py): route dout to the argmax of relu(z) per cell, mask, BN backward
    _, dg, db, dx, _ = res[BF16]
    yd = y.double()
    a = torch.relu(yd * scale.double() + shift.double()).permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(a, (kh, kw), (kh, kw)).backward(dout.double().permute(0, 3, 1, 2))
    dz = a.grad.permute(0, 2, 3, 1) * (yd * scale.double() + shift.double() > 0)
    P = n * h * w
    xhat = (yd - mean.double()) * invstd.double()
    ref = gamma.double() * invstd.double() * (dz - dz.sum((0, 1, 2)) / P - xhat * (dz * xhat).sum((0, 1, 2)) / P)

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))

    assert rel(dx, ref) < 1e-2
    assert rel(dg, (dz * xhat).sum((0, 1, 2))) < 1e-4 and rel(db, dz.sum((0, 1, 2))) < 1e-4
