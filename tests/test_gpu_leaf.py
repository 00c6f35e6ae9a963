"""GPU: the LEAF frontend kernels (mia_leaf_energy_*, mia_pcen_*) and LeafFrontend against the reference's
float64 fixture (tests/golden/golden_leaf.npz) and the float64 restatement tests/_leaf_ref.py (with bf16
operand rounding for the BF16 compute mode).

Cases (golden_leaf.npz): A = the reference default F = 186 (2F = 372 is no tile multiple, ragged tail),
B = tiny F and a short filter, C = the shipped config at full length (sampled).  Each with the reference's
initial parameters and with spread ones (wide envelopes: taps far from the centre and the zero padding
carry weight).  Case C's restatement runs on a subset of the filters (FSEL) to stay quick: every output
row and every bank-gradient row depends on its own filter only.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.synth import synth_waveform
from tests import _leaf_ref as R
from tests._util import rel_err

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
PSETS = {"init": R.init_params, "spread": R.spread_params}
FSEL = [0, 1, 31, 32, 33, 63, 64, 77, 95, 96, 126, 127]
_CACHE: dict = {}


@pytest.fixture(scope="module")
def gl():
    return dict(np.load(REPO / "tests" / "golden" / "golden_leaf.npz", allow_pickle=False))


def case_inputs(gl, name):
    if name not in _CACHE:
        F, Kt, T, B, pool = (int(v) for v in gl[f"{name}__dims"])
        sx, sg = (int(v) for v in gl[f"{name}__seeds"])
        x = torch.from_numpy(synth_waveform(sx, B, T))
        gy = torch.from_numpy(synth_waveform(sg, B, F * (T // pool)).reshape(B, F, T // pool))
        _CACHE[name] = (F, Kt, T, B, pool, x, gy)
    return _CACHE[name]


def frontend(F, Kt, pool, pset, compute, dev):
    from src.models.leaf import LeafFrontend
    m = LeafFrontend(n_filters=F, kernel_size=Kt, pool=pool, compute_dtype=compute)
    p = PSETS[pset](F)
    with torch.no_grad():
        m.gabor.center_freqs.copy_(p["center_freqs"])
        m.gabor.bandwidths.copy_(p["bandwidths"])
        m.pcen.r.copy_(p["r"])
        m.pcen.delta.copy_(p["delta"])
    return m.to(dev)


def run_parts(m, x, code):
    """(w, P, y) of the module's own two autograd Functions, with w and P retaining their gradients."""
    from src.models.leaf import _LeafEnergy, _PCEN
    w = m.gabor.filters()
    P = _LeafEnergy.apply(x, w, m.pool, code)
    if w.requires_grad:
        w.retain_grad()
        P.retain_grad()
    y = _PCEN.apply(P, m.pcen.r, m.pcen.delta, m.pcen.eps)
    return w, P, y


def check_vs_golden(gl, pre, name, got, key, bound):
    got = got.detach().cpu().double()
    if name == "C":
        e1 = rel_err(got.numpy().ravel()[gl[pre + "idx"]], gl[pre + key + "_s"])
        e2 = rel_err(got.mean(-1), gl[pre + key + "_rowmean"])
        print(f"{pre}{key}: sampled {e1:.3e}, row means {e2:.3e}")
        assert e1 <= bound and e2 <= bound
    else:
        e = rel_err(got, gl[pre + key])
        print(f"{pre}{key}: {e:.3e}")
        assert e <= bound


# ----------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("pset", ["init", "spread"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_f32(cuda, gl, name, pset):
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, _ = case_inputs(gl, name)
    m = frontend(F, Kt, pool, pset, "f32", cuda)
    with torch.no_grad():
        _, P, y = run_parts(m, x.to(cuda), L.F32)
        y2 = m(x.to(cuda)[:, None, :])
    assert torch.equal(y, y2)
    pre = f"{name}_{pset}__"
    check_vs_golden(gl, pre, name, P, "P", 1e-5)
    check_vs_golden(gl, pre, name, y, "y", 1e-5)


@pytest.mark.parametrize("pset", ["init", "spread"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_bf16(cuda, gl, name, pset):
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, _ = case_inputs(gl, name)
    m = frontend(F, Kt, pool, pset, "bf16", cuda)
    with torch.no_grad():
        w, P, y = run_parts(m, x.to(cuda), L.BF16)
    assert bool(torch.isfinite(y).all())
    sel = FSEL if name == "C" else list(range(F))
    emu = R.energy_pool(x, w.cpu()[:, sel], pool, bf16=True)
    e = rel_err(P.cpu()[:, sel], emu)
    print(f"{name} {pset}: P vs the bf16-operand emulation {e:.3e}")
    assert e <= 1e-5
    check_vs_golden(gl, f"{name}_{pset}__", name, P, "P", 1e-2)


# ----------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name,pset", [("A", "spread"), ("B", "spread"), ("A", "init")])
def test_backward_f32(cuda, gl, name, pset):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, gy = case_inputs(gl, name)
    m = frontend(F, Kt, pool, pset, "f32", cuda)
    xd = x.to(cuda)
    w, P, y = run_parts(m, xd, L.F32)
    y.backward(gy.to(cuda))
    pre = f"{name}_{pset}__"
    got = {"gP": P.grad, "g_center_freqs": m.gabor.center_freqs.grad, "g_bandwidths": m.gabor.bandwidths.grad,
           "g_r": m.pcen.r.grad, "g_delta": m.pcen.delta.grad}
    for k, v in got.items():
        check_vs_golden(gl, pre, name, v, k, 1e-4)
    assert m.pcen.alpha.grad is None
    gP = torch.from_numpy(gl[pre + "gP"]).float()
    dw = K.leaf_energy_bwd(xd, w.detach(), gP.to(cuda), pool, L.F32)
    want = R.energy_bwd(x, w.detach().cpu(), gP, pool)
    e = rel_err(dw.cpu(), want)
    print(f"{pre}dw: {e:.3e}")
    assert e <= 1e-4


@pytest.mark.parametrize("name", ["A", "B"])
def test_backward_bf16(cuda, gl, name):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, _ = case_inputs(gl, name)
    m = frontend(F, Kt, pool, "spread", "bf16", cuda)
    w = m.gabor.filters().detach()
    gP = torch.from_numpy(gl[f"{name}_spread__gP"]).float()
    dw = K.leaf_energy_bwd(x.to(cuda), w, gP.to(cuda), pool, L.BF16)
    want = R.energy_bwd(x, w.cpu(), gP, pool, bf16=True)
    e = rel_err(dw.cpu(), want)
    print(f"{name} spread bf16 dw: {e:.3e}")
    assert e <= 1e-4


def test_backward_bf16_full_length(cuda, gl):
    """Case C through the module in bf16: the bank gradient rows of FSEL and every parameter gradient
    against the emulation (which takes the P and gP the GPU produced, so each stage is checked on its own)."""
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, gy = case_inputs(gl, "C")
    m = frontend(F, Kt, pool, "spread", "bf16", cuda)
    w, P, y = run_parts(m, x.to(cuda), L.BF16)
    y.backward(gy.to(cuda))
    assert m.pcen.alpha.grad is None
    p = R.spread_params(F)
    gP_e, dr_e, dd_e = R.pcen_bwd(P.detach().cpu(), p["r"], p["delta"], gy)
    errs = {"gP": rel_err(P.grad.cpu(), gP_e), "g_r": rel_err(m.pcen.r.grad.cpu(), dr_e),
            "g_delta": rel_err(m.pcen.delta.grad.cpu(), dd_e)}
    gP = P.grad.cpu()
    dw_e = R.energy_bwd(x, w.detach().cpu()[:, FSEL], gP[:, FSEL], pool, bf16=True)
    errs["dw"] = rel_err(w.grad.cpu()[:, FSEL], dw_e)
    cf = p["center_freqs"][FSEL].double().requires_grad_(True)
    bw = p["bandwidths"][FSEL].double().requires_grad_(True)
    R.filters(cf, bw, Kt).backward(dw_e)
    errs["g_center_freqs"] = rel_err(m.gabor.center_freqs.grad.cpu()[FSEL], cf.grad)
    errs["g_bandwidths"] = rel_err(m.gabor.bandwidths.grad.cpu()[FSEL], bw.grad)
    print({k: f"{v:.3e}" for k, v in errs.items()})
    assert all(v <= 1e-4 for v in errs.values()), errs


# ----------------------------------------------------------------------------------------------- tile edges
EDGES = {  # name: (B, F, Kt, pool, T)
    "one_frame": (2, 5, 65, 160, 160),
    "short_of_a_frame": (2, 5, 65, 160, 160 * 3 - 1),
    "wg_tile_plus_one_frame": (1, 5, 65, 160, 160 * 17),  # the MFMA kernel's workgroup walks 16 frames of 160
    "one_filter": (2, 1, 65, 160, 160 * 2 + 7),
    "three_taps": (2, 5, 3, 160, 160 * 2 + 7),
    "pool_32": (2, 5, 65, 32, 32 * 81 + 5),  # 80 frames of 32 per MFMA workgroup, plus one
    "pool_1024": (1, 5, 65, 1024, 1024 * 3 + 9),  # two frames per MFMA workgroup, plus one
    "longest_filter": (1, 3, 1023, 1024, 1024 * 3 + 5),  # the bank block streamed from memory, four tap blocks
    "filters_33": (1, 33, 33, 160, 160 * 2),  # a second filter block with one filter in it
    "filters_65": (1, 65, 33, 160, 160 * 2),  # the MFMA backward's second block of 64 filters, three idle waves
    "taps_447": (1, 3, 447, 160, 160 * 9 + 3),  # the longest filter of the MFMA backward; two units of 8 + 1 frames
    "taps_449": (1, 3, 449, 160, 160 * 2),  # the shortest filter that takes the FMA backward in bf16 mode
}


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("edge", list(EDGES))
def test_tile_edges(cuda, edge, mode):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    B, F, Kt, pool, T = EDGES[edge]
    bf = mode == "bf16"
    code = L.BF16 if bf else L.F32
    x = torch.from_numpy(synth_waveform(8100 + len(edge), B, T))
    p = R.spread_params(F)
    w = R.filters(p["center_freqs"].double(), p["bandwidths"].double(), Kt).float()
    gP = torch.from_numpy(synth_waveform(8200 + len(edge), B, F * (T // pool)).reshape(B, F, T // pool))
    P = K.leaf_energy_fwd(x.to(cuda), w.to(cuda), pool, code)
    dw = K.leaf_energy_bwd(x.to(cuda), w.to(cuda), gP.to(cuda), pool, code)
    eP = rel_err(P.cpu(), R.energy_pool(x, w, pool, bf16=bf))
    edw = rel_err(dw.cpu(), R.energy_bwd(x, w, gP, pool, bf16=bf))
    print(f"{edge} {mode}: P {eP:.3e}, dw {edw:.3e}")
    assert eP <= 1e-5
    assert edw <= 1e-4


# ----------------------------------------------------------------------------------------------- properties
def test_backward_is_deterministic(cuda, gl):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, gy = case_inputs(gl, "A")
    m = frontend(F, Kt, pool, "spread", "bf16", cuda)
    w = m.gabor.filters().detach()
    xd, gyd = x.to(cuda), gy.to(cuda)
    r, d = m.pcen.r.detach(), m.pcen.delta.detach()
    outs = []
    for _ in range(2):
        for code in (L.F32, L.BF16):
            P = K.leaf_energy_fwd(xd, w, pool, code)
            gP, dr, dd = K.pcen_bwd(P, r, d, 1e-6, gyd)
            outs.append((K.leaf_energy_bwd(xd, w, gP, pool, code), dr, dd))
    for a, b in zip(outs[:2], outs[2:]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_silence_and_quiet_clip(cuda, mode):
    m = frontend(7, 65, 160, "spread", mode, cuda)
    from src.miaudio import kernels as K
    z = torch.zeros(2, 160 * 4 + 3, device=cuda)
    with torch.no_grad():
        P = K.leaf_energy_fwd(z, m.gabor.filters(), 160, m._compute_code())
        y = m(z)
    assert torch.equal(P, torch.zeros_like(P))
    # P / (eps + M)^r is exactly 0, so y is log(delta) alone: the same bits in every frame and clip of a filter
    # (edge frames included), and the float32 logarithm of delta -- within 1 ulp of the float64 value, the
    # accuracy of the device's logf (two float32 log implementations need not agree in the last bit)
    assert torch.equal(y, y[:1, :, :1].expand_as(y))
    d64 = m.pcen.delta.detach().cpu().double()
    want = torch.log(d64)
    ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64)).float().double()
    ulp = 2.0 ** (torch.floor(torch.log2(ulp)) - 23)
    assert bool(((y[0, :, 0].cpu().double() - want).abs() <= ulp).all())
    q = torch.from_numpy(synth_waveform(8301, 2, 160 * 4 + 3)).to(cuda) * 1e-4
    y = m(q)
    y.sum().backward()
    assert bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(t.grad).all()) for t in (m.gabor.center_freqs, m.gabor.bandwidths, m.pcen.r,
                                                             m.pcen.delta))


def test_side_stream_and_workspace_slots(cuda, gl):
    """The op on a non-default stream gives the default stream's result, and the GEMM workspace slot is its
    own: a split-K GEMM gives the same bits before and after a frontend step."""
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    F, Kt, T, B, pool, x, gy = case_inputs(gl, "A")
    m = frontend(F, Kt, pool, "spread", "bf16", cuda)
    xd, gyd = x.to(cuda), gy.to(cuda)
    g = torch.Generator().manual_seed(5)
    a = torch.randn(64, 4096, generator=g).to(cuda)
    b = torch.randn(96, 4096, generator=g).to(cuda)

    def gemm():
        out = torch.empty(64, 96, dtype=torch.float32, device=cuda)
        K.gemm(K.dense(a, L.KC, 64, 4096), K.dense(b, L.KC, 96, 4096), K.epilogue(out, 96), 64, 96, 4096, L.F32,
               split_k=4)
        return out

    def step():
        for q in m.parameters():
            q.grad = None
        y = m(xd)
        y.backward(gyd)
        return y.detach(), m.gabor.center_freqs.grad.clone(), m.pcen.r.grad.clone()

    g0 = gemm()
    ref = step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = step()
        g1 = gemm()
    side.synchronize()
    assert all(torch.equal(u, v) for u, v in zip(ref, got))
    assert torch.equal(g0, g1)
