"""CPU: the LEAF restatement (tests/_leaf_ref.py) is pinned to the reference's float64 fixture, LeafFrontend
carries the reference's state_dict, its CPU path computes the golden output, and bad geometry is rejected
before anything is launched."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle.synth import synth_waveform
from tests import _leaf_ref as R
from tests._util import rel_err

REPO = Path(__file__).resolve().parents[1]
PSETS = {"init": R.init_params, "spread": R.spread_params}


@pytest.fixture(scope="module")
def gl():
    return dict(np.load(REPO / "tests" / "golden" / "golden_leaf.npz", allow_pickle=False))


def case_inputs(gl, name):
    F, Kt, T, B, pool = (int(v) for v in gl[f"{name}__dims"])
    sx, sg = (int(v) for v in gl[f"{name}__seeds"])
    x = torch.from_numpy(synth_waveform(sx, B, T))
    gy = torch.from_numpy(synth_waveform(sg, B, F * (T // pool)).reshape(B, F, T // pool))
    return F, Kt, T, B, pool, x, gy


@pytest.mark.parametrize("pset", ["init", "spread"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_ref_matches_golden_small(gl, name, pset):
    F, Kt, T, B, pool, x, gy = case_inputs(gl, name)
    p = {k: v.double().requires_grad_(True) for k, v in PSETS[pset](F).items()}
    w = R.filters(p["center_freqs"], p["bandwidths"], Kt)
    P = R.energy_pool(x, w.detach(), pool)
    y = R.pcen(P, p["r"].detach(), p["delta"].detach())
    pre = f"{name}_{pset}__"
    assert rel_err(P, gl[pre + "P"]) <= 1e-10
    assert rel_err(y, gl[pre + "y"]) <= 1e-10
    gP, dr, dd = R.pcen_bwd(P, p["r"].detach(), p["delta"].detach(), gy)
    assert rel_err(gP, gl[pre + "gP"]) <= 1e-10
    assert rel_err(dr, gl[pre + "g_r"]) <= 1e-10
    assert rel_err(dd, gl[pre + "g_delta"]) <= 1e-10
    dw = R.energy_bwd(x, w.detach(), gP, pool)
    w.backward(dw)
    assert rel_err(p["center_freqs"].grad, gl[pre + "g_center_freqs"]) <= 1e-10
    assert rel_err(p["bandwidths"].grad, gl[pre + "g_bandwidths"]) <= 1e-10


def test_ref_matches_golden_full_length(gl):
    """Case C (the shipped config, FFT path of the restatement) at the sampled indices and the row means."""
    F, Kt, T, B, pool, x, gy = case_inputs(gl, "C")
    p = R.spread_params(F)
    P, y = R.frontend(x, p, Kt, pool)
    pre = "C_spread__"
    idx = gl[pre + "idx"]
    assert rel_err(P.numpy().ravel()[idx], gl[pre + "P_s"]) <= 1e-10
    assert rel_err(y.numpy().ravel()[idx], gl[pre + "y_s"]) <= 1e-10
    assert rel_err(P.mean(-1), gl[pre + "P_rowmean"]) <= 1e-10
    assert rel_err(y.mean(-1), gl[pre + "y_rowmean"]) <= 1e-10


def test_state_dict_matches_reference(gl):
    from src.models.leaf import LeafFrontend
    sd = LeafFrontend().state_dict()
    want = {k[len("state186__"):]: v for k, v in gl.items() if k.startswith("state186__")}
    assert set(sd) == set(want) == {"gabor.center_freqs", "gabor.bandwidths", "gabor.window", "pcen.alpha",
                                    "pcen.delta", "pcen.r"}
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert sd[k].dtype == torch.float32
        assert np.array_equal(sd[k].numpy(), v), k


@pytest.mark.parametrize("pset", ["init", "spread"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_cpu_forward_matches_golden(gl, name, pset):
    from src.models.leaf import LeafFrontend
    F, Kt, T, B, pool, x, _ = case_inputs(gl, name)
    m = LeafFrontend(n_filters=F, kernel_size=Kt, pool=pool)
    p = PSETS[pset](F)
    with torch.no_grad():
        m.gabor.center_freqs.copy_(p["center_freqs"])
        m.gabor.bandwidths.copy_(p["bandwidths"])
        m.pcen.r.copy_(p["r"])
        m.pcen.delta.copy_(p["delta"])
    want = gl[f"{name}_{pset}__y"]
    with torch.no_grad():
        y32 = m(x[:, None, :])
        y64 = m.double()(x.double())
    assert y32.shape == want.shape and y32.dtype == torch.float32
    assert rel_err(y64, want) <= 1e-10
    # float32 evaluation of the same formulas: a few float32 roundings against the float64 values
    assert rel_err(y32, want) <= 1e-5


def test_input_requiring_grad_raises():
    from src.models.leaf import LeafFrontend
    m = LeafFrontend(n_filters=4, kernel_size=9)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 320, requires_grad=True))


def test_compute_dtype_spellings():
    from src.miaudio import lib as L
    from src.models.leaf import LeafFrontend
    for s, code in (("bf16", L.BF16), ("bfloat16", L.BF16), ("f32", L.F32), ("fp32", L.F32), ("32", L.F32)):
        assert LeafFrontend(4, 9, compute_dtype=s)._compute_code() == code


@pytest.mark.parametrize("Kt,pool,T", [(400, 160, 1600), (401, 100, 1600), (401, 160, 159), (1025, 160, 1600),
                                       (401, 2048, 4096)])
def test_bad_geometry_rejected(Kt, pool, T):
    from src.miaudio import kernels as K
    from src.miaudio import lib as L
    x = torch.zeros(2, T)
    w = torch.zeros(2, 4, Kt)
    # ValueError comes before the device check (these are CPU tensors): nothing was launched
    with pytest.raises(ValueError):
        K.leaf_energy_fwd(x, w, pool, L.F32)
    with pytest.raises(ValueError):
        K.leaf_energy_bwd(x, w, torch.zeros(2, 4, max(T // pool, 1)), pool, L.F32)
    # the library's own host-side validation agrees
    lib = L.load()
    assert lib.mia_leaf_workspace_bytes(2, T, 4, Kt, pool, 0) < 0
    assert lib.mia_leaf_workspace_bytes(2, T, 4, Kt, pool, 1) < 0
    assert lib.mia_leaf_energy_fwd(None, None, None, 2, T, 4, Kt, pool, L.F32, None, None) != 0


def test_workspace_sizes_for_valid_geometry():
    from src.miaudio import lib as L
    lib = L.load()
    assert lib.mia_leaf_workspace_bytes(2, 220_500, 128, 401, 160, 0) == 4 * 2 * 26 * 64 * 16
    assert lib.mia_leaf_workspace_bytes(2, 220_500, 128, 401, 160, 1) > 0
    assert lib.mia_pcen_workspace_bytes(2, 128) == 2 * 128 * 16
