"""GPU: the two forms of mia_conv1ch_dgrad and of mia_fe_conv1_wgrad_bn compute the same bits.

mia_conv1ch_dgrad (trunk conv3 backward-data).  The default form (wave-persistent: a wave owns a (clip, 32-column)
item, its dY rows stream through a register ring across items, the output strip of one item is stored under the
loads of the next) and the MIA_C1CH_V1=1 form (one block per (clip, 128 columns), a barrier per dY row) run on the
same inputs inside one process; `dx` must be `torch.equal` -- the arithmetic is the same, only the schedule differs.  So that both cannot be wrong together, the
default form is also compared with float64 conv_transpose2d of the same bf16 operands on the CPU, at the tolerance of
test_gpu_gemm.py::test_conv1ch_dgrad_bf16.

On a full-size device every shape here has fewer items than the grid has waves, so each wave would take one item
only.  MIA_C1CH_GRID (read at call time) caps the grid: every shape also runs with 1 and 2 blocks, where a wave
walks several items (up to 54 of them) and the epilogue of one runs under the loads of the next.

mia_fe_conv1_wgrad_bn (conv1 weight gradient + BN1/ReLU backward).  The default form (each wave stages and consumes
its own k-steps, two chunks wait in registers, x goes from the load registers to four shifted copies per parity) and
the MIA_CONV1W_V1=1 form (three block barriers a chunk, eight copies built through LDS) must agree in every output
and in the whole workspace prefix the main kernel writes (the per-block slabs and channel sums).  The default form
is also compared with the float64 statement of test_gpu_norm.py::test_fe_conv1_wgrad_bn_fused, at its tolerances.
Called through ctypes so that `split` (the grid) can vary."""
import pytest
import torch
import torch.nn.functional as F

from src.miaudio import kernels as K
from src.miaudio import lib as L

pytestmark = pytest.mark.gpu

#          n  oh  ow
DGRAD = [(1, 1, 1),       # the smallest shape: one item of 8 columns, one dY row
         (2, 3, 121),     # 128 output columns per clip (4 full items); odd oh
         (2, 4, 125),     # 132 columns: a fifth item 4 columns wide; even oh, one whole turn of the 4-row ring
         (3, 57, 125),    # full height (64 output rows): 14 ring turns + 1 row, 15 items
         (2, 2, 853)]     # the bench width: 27 items per clip, the last 28 columns wide


def _dgrad(dy, w, n, oh, ow):
    out = torch.full((n, oh + 7, ow + 7), float("nan"), dtype=torch.bfloat16, device=dy.device)
    K.conv1ch_dgrad(dy.reshape(-1, 32), w, n, oh, ow, out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("n,oh,ow", DGRAD, ids=lambda v: str(v))
def test_conv1ch_dgrad_forms_bit_identical(cuda, monkeypatch, n, oh, ow):
    g = torch.Generator().manual_seed(oh * 1000 + ow)
    dy = torch.randn(n, oh, ow, 32, generator=g).to(torch.bfloat16)
    w = torch.randn(32, 1, 8, 8, generator=g) * 0.1
    dyc, wc = dy.to(cuda), w.to(cuda)
    monkeypatch.delenv("MIA_C1CH_GRID", raising=False)
    monkeypatch.setenv("MIA_C1CH_V1", "1")
    old = _dgrad(dyc, wc, n, oh, ow)
    monkeypatch.delenv("MIA_C1CH_V1")
    new = {"default": _dgrad(dyc, wc, n, oh, ow)}
    for cap in ("1", "2"):
        monkeypatch.setenv("MIA_C1CH_GRID", cap)
        new[f"grid {cap}"] = _dgrad(dyc, wc, n, oh, ow)
    monkeypatch.delenv("MIA_C1CH_GRID")
    assert not bool(torch.isnan(old.float()).any()), "MIA_C1CH_V1 form left part of dx unwritten"
    for what, out in new.items():
        assert not bool(torch.isnan(out.float()).any()), f"{what}: part of dx was never written"
        assert torch.equal(out, old), f"{what}: dx differs from the MIA_C1CH_V1 form"
    wb = w.to(torch.bfloat16).double()
    ref = F.conv_transpose2d(dy.double().permute(0, 3, 1, 2), wb)[:, 0]
    err = float((new["default"].double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
    assert err < 1e-2, f"dx differs from float64 conv_transpose2d: rel {err}"


#          n  t     split     w1 = (t - 64) / 2 + 1
WGRAD = [(1, 64, 2),        # 1: a single pixel; one block idle
         (2, 574, 2),       # 256: exactly one full chunk per clip
         (3, 2718, 2),      # 1328 = 5 * 256 + 48: 18 chunks, 9 a block (4 pairs + 1), a ragged chunk in mid-stream
         (3, 2718, 7),      # uneven chunks per block (3 or 2)
         (3, 2718, 512)]    # most blocks idle


def _wgrad(x, da, y1, n, t, split, scale, shift, gamma, mean, invstd):
    dev = x.device
    out = {k: torch.full(s, float("nan"), device=dev) for k, s in
           (("dgamma", (32,)), ("dbeta", (32,)), ("dw", (32, 64)), ("dbias", (32,)))}
    ws = torch.full((split * (2 * 2048 + 96) + 2 * 2048 + n * 80 + 2 * 160 + 4,), float("nan"), device=dev)
    L.check(L.load().mia_fe_conv1_wgrad_bn(x.data_ptr(), da.data_ptr(), y1.data_ptr(), n, t, scale.data_ptr(),
                                           shift.data_ptr(), gamma.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                           out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), out["dw"].data_ptr(),
                                           out["dbias"].data_ptr(), ws.data_ptr(), split, K._s()),
            "mia_fe_conv1_wgrad_bn")
    torch.cuda.synchronize()
    out["slabs + channel sums"] = ws[: split * (2 * 2048 + 96)].clone()
    return out


def _check_wgrad_forms(cuda, monkeypatch, n, t, split, masked_off):
    w1 = (t - 64) // 2 + 1
    P = n * w1
    g = torch.Generator().manual_seed(t + 7 * n + split)
    x = torch.randn(n, t, generator=g) * 0.1
    y1 = (torch.randn(P, 32, generator=g) * 0.7 + 0.2).to(torch.bfloat16)
    da = (torch.randn(P, 32, generator=g) * 1e-3).to(torch.bfloat16)
    # a BN1 state with mixed-sign gamma: scale = gamma * invstd changes sign from channel to channel and the
    # ReLU mask is about half on
    gamma = (torch.rand(32, generator=g) + 0.5) * torch.where(torch.rand(32, generator=g) < 0.5, -1.0, 1.0)
    beta = torch.randn(32, generator=g) * 0.1
    mean = y1.float().mean(0) if P > 1 else torch.full((32,), 0.2)
    invstd = 1.0 / (y1.float().var(0, unbiased=False) + 1e-5).sqrt() if P > 1 else torch.full((32,), 1.0 / 0.7)
    scale = gamma * invstd
    shift = beta - mean * scale
    if masked_off:  # relu clamps every value
        scale, shift = scale.abs(), torch.full((32,), -100.0)
    args = [v.to(cuda) for v in (x, da, y1)] + [n, t, split] + [v.to(cuda) for v in (scale, shift, gamma, mean, invstd)]
    monkeypatch.setenv("MIA_CONV1W_V1", "1")
    old = _wgrad(*args)
    monkeypatch.delenv("MIA_CONV1W_V1")
    new = _wgrad(*args)
    for what in new:
        assert torch.equal(new[what], old[what]), f"{what} differs between the forms"
    # float64 restatement (test_gpu_norm.py::test_fe_conv1_wgrad_bn_fused)
    y = y1.double()
    z = y * scale.double() + shift.double()
    dz = torch.where(z > 0, da.double(), torch.zeros_like(z))
    xhat = (y - mean.double()) * invstd.double()
    mdz, mdzx = dz.mean(0), (dz * xhat).mean(0)
    d64 = gamma.double() * invstd.double() * (dz - mdz - xhat * mdzx)
    cols = x.double().unfold(1, 64, 2)  # (n, w1, 64)
    ref = torch.einsum("npc,npk->ck", d64.view(n, w1, 32), cols)

    def rel(a, b):
        return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))

    assert rel(new["dw"], ref) < 1e-2
    assert rel(new["dgamma"], (dz * xhat).sum(0)) < 1e-4 and rel(new["dbeta"], dz.sum(0)) < 1e-4
    assert float((new["dbias"].double().cpu() - d64.sum(0)).abs().max()) <= 1e-3 * float(d64.abs().sum(0).max())


@pytest.mark.parametrize("n,t,split", WGRAD, ids=lambda v: str(v))
def test_fe_conv1_wgrad_bn_forms_bit_identical(cuda, monkeypatch, n, t, split):
    _check_wgrad_forms(cuda, monkeypatch, n, t, split, masked_off=False)


def test_fe_conv1_wgrad_bn_forms_all_masked_off(cuda, monkeypatch):
    """Every y1 masked off by the ReLU: dz = 0, so every gradient is exactly zero in both forms."""
    _check_wgrad_forms(cuda, monkeypatch, 3, 2718, 7, masked_off=True)
