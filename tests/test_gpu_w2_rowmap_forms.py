"""GPU: the two producers of a (1, 2)-conv backward's gradient storing through a row map (include/miaudio_rowmap.h)
against the dense producers followed by the copy pass mia_pad_w2.

For each producer G from the row-mapped call must be `torch.equal` to mia_pad_w2 of the dense call's dx, and dbias and
the rows of `partial` must be the same bits.  G and the pad pixel of `a` sit between one-pixel guard bands of sentinel
bytes, which must be intact; the pad pixel must be zero; lead = 0, row_pixels = w gives the dense bytes.

Pooled producer (a (1, 2) pool, 3 rows of 6): C = 8 / 64 / 256 give 9 / 72 / 288 runs, so C = 256 takes two blocks at the
natural grid and one thread walks two runs under MIA_POOL_GRID=1.  BN producer: 3 rows of 5, C = 8 and 128."""
import pytest
import torch

from src.miaudio import kernels as K
from src.miaudio import lib as L

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 0x5A


def _bn(c, g, dev):
    return K.BNState((torch.randn(c, generator=g) * 0.1).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev),
                     ((torch.rand(c, generator=g) - 0.3) * 1.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev))


class Guarded:
    """`pixels` pixels of c bf16 between two one-pixel guard bands of sentinel bytes."""

    def __init__(self, pixels, c, dev):
        self.raw = torch.full(((pixels + 2) * c * 2,), SENTINEL, dtype=torch.uint8, device=dev)
        self.t = self.raw[c * 2: (pixels + 1) * c * 2].view(BF16)
        self.c = c

    def intact(self):
        n = self.c * 2
        return bool((self.raw[:n] == SENTINEL).all()) and bool((self.raw[-n:] == SENTINEL).all())


def _poisoned_ws(P, c, dev):
    ws = K.workspace(L.load().mia_bn_partial_bytes(P, c), dev, "bn")
    ws.fill_(0xFF)
    return ws


def _snap_ws(P, c, dev):
    torch.cuda.synchronize()
    n = L.load().mia_bn_partial_bytes(P, c)
    return K.workspace(n, dev, "bn")[:n].clone()


def _pad_w2(dx, rows, w, c, zc):
    """mia_pad_w2 of the dense gradient: (G, pad pixel), both guarded."""
    G, zp = Guarded(1 + rows * w, c, dx.device), Guarded(1, zc, dx.device)
    L.check(L.load().mia_pad_w2(dx.data_ptr(), rows, w, c, G.t.data_ptr(), zp.t.data_ptr(), zc, L.stream_ptr()),
            "mia_pad_w2")
    torch.cuda.synchronize()
    assert G.intact() and zp.intact()
    return G.t, zp.t


def _check(Gm, zm, Gref, dbias_m, dbias_d, ws_m, ws_d):
    assert Gm.intact(), "row-mapped dx: a guard band was written"
    assert zm.intact(), "pad pixel: a guard band was written"
    assert bool((zm.t.view(torch.int16) == 0).all()), "a's pad pixel is not zero"
    assert torch.equal(Gm.t.view(torch.int16), Gref.view(torch.int16)), "G differs from mia_pad_w2 of the dense dx"
    assert torch.equal(dbias_m.view(torch.int32), dbias_d.view(torch.int32)), "dbias differs"
    assert torch.equal(ws_m, ws_d), "the rows of partial differ"


@pytest.mark.parametrize("grid", [None, 1], ids=lambda v: f"grid{v}")
@pytest.mark.parametrize("gdt", [BF16, F32], ids=["gm-bf16", "gm-f32"])
@pytest.mark.parametrize("c", [8, 64, 256])
def test_pooled_producer_row_map(cuda, monkeypatch, c, gdt, grid):
    for v in ("MIA_POOL_V1", "MIA_POOL_GRID", "MIA_POOL_GM32", "MIA_POOL_BWD_PIXEL"):
        monkeypatch.delenv(v, raising=False)
    n, h, w, kh, kw = 3, 1, 6, 1, 2  # 3 rows of 6
    oh, ow, P = h // kh, w // kw, n * h * w
    g = torch.Generator().manual_seed(c + 1)
    x = torch.randn(n, h, w, c, generator=g).to(BF16).to(cuda)
    st = _bn(c, g, cuda)
    gamma = ((torch.rand(c, generator=g) - 0.3) * 1.5).to(cuda)
    pooled = torch.empty(n, oh, ow, c, dtype=BF16, device=cuda)
    am = torch.full((n, oh, ow, c), 255, dtype=torch.uint8, device=cuda)
    win = torch.full((n, oh, ow, c), float("nan"), dtype=BF16, device=cuda)
    K.pool_fwd(x, n, h, w, c, kh, kw, st, pooled, 0, am, win=win)
    dout = torch.randn(n, oh, ow, c, generator=g).to(BF16).to(cuda)
    gm, dg, db = K.pool_bwd_gather(dout, 0, am, x, n, h, w, c, kh, kw, st, win=win, gm_dtype=gdt)
    if grid:
        monkeypatch.setenv("MIA_POOL_GRID", str(grid))
    # dense, then the copy pass
    dx = torch.full((P, c), float("nan"), dtype=BF16, device=cuda)
    dbias_d = torch.full((c,), float("nan"), device=cuda)
    _poisoned_ws(P, c, cuda)
    K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, gamma, st, dg, db, dx, dbias_d)
    ws_d = _snap_ws(P, c, cuda)
    zc = 64
    Gref, _ = _pad_w2(dx, n * h, w + 1, c, zc)
    # row-mapped: lead 1, rows of w + 1
    Gm, zm = Guarded(1 + n * h * (w + 1), c, cuda), Guarded(1, zc, cuda)
    dbias_m = torch.full((c,), float("nan"), device=cuda)
    _poisoned_ws(P, c, cuda)
    K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, gamma, st, dg, db, Gm.t, dbias_m, rowmap=(1, w + 1, zm.t))
    ws_m = _snap_ws(P, c, cuda)
    _check(Gm, zm, Gref, dbias_m, dbias_d, ws_m, ws_d)
    # the identity map is the dense form
    Di = Guarded(P, c, cuda)
    K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, gamma, st, dg, db, Di.t, None, rowmap=(0, w, None))
    torch.cuda.synchronize()
    assert Di.intact() and torch.equal(Di.t.view(torch.int16), dx.view(torch.int16).reshape(-1))


@pytest.mark.parametrize("c", [8, 128])
def test_bn_producer_row_map(cuda, c):
    rows, w = 3, 5
    P = rows * w
    g = torch.Generator().manual_seed(c + 2)
    x = torch.randn(P, c, generator=g).to(BF16).to(cuda)
    dact = torch.randn(P, c, generator=g).to(BF16).to(cuda)
    st = _bn(c, g, cuda)
    gamma = ((torch.rand(c, generator=g) - 0.3) * 1.5).to(cuda)
    dg, db = K.bn_relu_bwd_reduce(dact, None, x, P, c, st)
    dx = torch.full((P, c), float("nan"), dtype=BF16, device=cuda)
    dbias_d = torch.full((c,), float("nan"), device=cuda)
    _poisoned_ws(P, c, cuda)
    K.bn_relu_bwd_apply(dact, x, dx, P, c, gamma, st, dg, db, dbias_d)
    ws_d = _snap_ws(P, c, cuda)
    zc = 32
    Gref, _ = _pad_w2(dx, rows, w + 1, c, zc)
    Gm, zm = Guarded(1 + rows * (w + 1), c, cuda), Guarded(1, zc, cuda)
    dbias_m = torch.full((c,), float("nan"), device=cuda)
    _poisoned_ws(P, c, cuda)
    K.bn_relu_bwd_apply(dact, x, Gm.t, P, c, gamma, st, dg, db, dbias_m, rowmap=(w, 1, w + 1, zm.t))
    ws_m = _snap_ws(P, c, cuda)
    _check(Gm, zm, Gref, dbias_m, dbias_d, ws_m, ws_d)
    Di = Guarded(P, c, cuda)
    K.bn_relu_bwd_apply(dact, x, Di.t, P, c, gamma, st, dg, db, None, rowmap=(w, 0, w, None))
    torch.cuda.synchronize()
    assert Di.intact() and torch.equal(Di.t.view(torch.int16), dx.view(torch.int16).reshape(-1))


def test_row_map_is_refused_where_no_kernel_serves_it(cuda):
    """A map other than the dense one needs the run form of the pooled producer: kw = 5 has none."""
    n, h, w, c, kh, kw = 1, 2, 10, 8, 2, 5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, h, w, c, generator=g).to(BF16).to(cuda)
    st = _bn(c, g, cuda)
    am = torch.zeros(n, h // kh, w // kw, c, dtype=torch.uint8, device=cuda)
    gm = torch.zeros(n, h // kh, w // kw, c, dtype=BF16, device=cuda)
    z = torch.zeros(c, device=cuda)
    G = torch.zeros((1 + n * h * (w + 1)) * c, dtype=BF16, device=cuda)
    with pytest.raises(RuntimeError):
        K.pool_bn_relu_bwd_apply(gm, am, x, n, h, w, c, kh, kw, None, st, z, z, G, None, rowmap=(1, w + 1, None))
    torch.cuda.synchronize()
