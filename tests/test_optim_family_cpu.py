"""CPU: the host side of the fused optimizer family -- the header / signature / contract-case table of
include/miaudio_optim.h, constructor validation of FusedSGD and FusedAdamW, their state_dict exchange with
torch.optim.SGD / AdamW, the engine's routing of CPU parameters, and the update formulas (tests/_optim_ref.py)
against the installed torch on CPU."""
import copy
import re
from pathlib import Path

import pytest
import torch

from src.miaudio import lib as L
from tests import _optim_ref as R

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio_optim.h"
ENTRY_POINTS = {"mia_clip_sgd", "mia_clip_adamw", "mia_gemm_sgd", "mia_gemm_adamw"}


# ------------------------------------------------------------------------------------------------ header table
def _writes_caller_memory(params: str) -> bool:  # the rule of tests/test_memory_contract_table_cpu.py
    for prm in params.split(","):
        prm = " ".join(prm.split())
        if "*" not in prm:
            continue
        if prm.startswith(("const MiaEpilogue*", "const MiaPackJob*")):
            return True
        if not prm.startswith("const "):
            return True
    return False


def _header_text():
    return re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)


def test_every_entry_point_of_the_optim_header_is_exported_with_a_signature():
    every = set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", _header_text()))
    assert every == ENTRY_POINTS
    assert every <= set(L.SIGNATURES), sorted(every - set(L.SIGNATURES))
    assert every <= L.exported_symbols(), sorted(every - L.exported_symbols())
    decls = dict(re.findall(r"\bint\s+(mia_\w+)\s*\(([^;{]*?)\)\s*;", _header_text(), flags=re.S))
    for name, params in decls.items():  # one ctypes argument per declared parameter
        assert len(L.SIGNATURES[name][1]) == len(params.split(",")), name


def test_every_entry_point_of_the_optim_header_has_a_contract_case():
    from tests import test_gpu_optim_family_contract as T
    decls = re.findall(r"\bint\s+(mia_\w+)\s*\(([^;{]*?)\)\s*;", _header_text(), flags=re.S)
    names = {name for name, params in decls if _writes_caller_memory(params)}
    assert names == ENTRY_POINTS, names
    covered = {n for covers in T.COVERS.values() for n in covers}
    assert names == covered, (sorted(names - covered), sorted(covered - names))


def test_miaudio_h_does_not_declare_the_optimizer_family():
    text = (HEADER.parent / "miaudio.h").read_text()
    assert not any(n in text for n in ENTRY_POINTS)


# ------------------------------------------------------------------------------------------------ constructors
def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((5, 3), (7,))]


def test_fused_sgd_constructor_validation():
    from src.training.optim import FusedSGD
    p = _params()
    opt = FusedSGD(p, lr=0.1, momentum=0.9, nesterov=True, weight_decay=5e-4, clip=1.0, foreach=None, fused=None,
                   maximize=False, differentiable=False)
    assert opt.clip == 1.0 and opt.defaults["nesterov"] is True and opt.defaults["momentum"] == 0.9
    assert all(q._mia_fused_adam() is opt for q in p)  # the deferral protocol's attribute keeps its name
    assert FusedSGD(p, lr=0.1).defaults["momentum"] == 0
    for kw in ({"maximize": True}, {"differentiable": True}):
        with pytest.raises(ValueError, match="torch.optim.SGD"):
            FusedSGD(p, lr=0.1, **kw)
    with pytest.raises(TypeError, match="bogus"):
        FusedSGD(p, lr=0.1, bogus=1)
    with pytest.raises(TypeError):
        FusedSGD(p, lr=0.1, amsgrad=False)  # not an option of torch.optim.SGD
    for kw in ({"nesterov": True}, {"nesterov": True, "momentum": 0.9, "dampening": 0.1}):
        with pytest.raises(ValueError, match="[Nn]esterov"):
            FusedSGD(p, lr=0.1, **kw)
        with pytest.raises(ValueError, match="[Nn]esterov"):
            torch.optim.SGD(p, lr=0.1, **kw)


def test_fused_adamw_constructor_validation():
    from src.training.optim import FusedAdam, FusedAdamW
    p = _params()
    opt = FusedAdamW(p, lr=1e-3, clip=0.5, amsgrad=False, foreach=None, fused=None)
    assert isinstance(opt, FusedAdam) and opt.defaults["weight_decay"] == 1e-2 == torch.optim.AdamW(p).defaults[
        "weight_decay"]
    assert opt.clip == 0.5 and all(q._mia_fused_adam() is opt for q in p)
    for kw in ({"amsgrad": True}, {"maximize": True}, {"capturable": True}, {"differentiable": True}):
        with pytest.raises(ValueError, match="torch.optim.AdamW"):
            FusedAdamW(p, **kw)
    with pytest.raises(TypeError, match="bogus"):
        FusedAdamW(p, bogus=1)
    # FusedAdam itself keeps rejecting the decoupled form
    with pytest.raises(ValueError):
        FusedAdam(p, decoupled_weight_decay=True)
    assert FusedAdam(p).defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)


def test_moment_tensors_follow_the_optimizer():
    from src.training.optim import FusedAdam, FusedAdamW, FusedSGD
    p = _params()
    for cls, kw, names in ((FusedAdam, {}, ("exp_avg", "exp_avg_sq")), (FusedAdamW, {}, ("exp_avg", "exp_avg_sq")),
                           (FusedSGD, {"momentum": 0.9}, ("momentum_buffer",)), (FusedSGD, {}, ())):
        opt = cls(p, lr=1e-3, **kw)
        assert opt.moment_tensors(p[0]) == []  # no state before the first step
        for k in ("exp_avg", "exp_avg_sq", "momentum_buffer"):
            opt.state[p[0]][k] = torch.zeros_like(p[0])
        got = opt.moment_tensors(p[0])
        assert [t.data_ptr() for t in got] == [opt.state[p[0]][k].data_ptr() for k in names]


# ------------------------------------------------------------------------------------------------ state_dict
def _stepped(cls, p, seed, **kw):
    opt = cls(p, **kw)
    g = torch.Generator().manual_seed(seed)
    for _ in range(2):
        for q in p:
            q.grad = torch.randn(q.shape, generator=g)
        opt.step()
    return opt


@pytest.mark.parametrize("kw", [dict(lr=0.1, momentum=0.9, nesterov=True, weight_decay=5e-4), dict(lr=0.1)])
def test_fused_sgd_state_dict_round_trips_through_torch_sgd(kw):
    from src.training.optim import FusedSGD
    p = _params()
    src = _stepped(torch.optim.SGD, p, 1, **kw)
    fused = FusedSGD([torch.nn.Parameter(q.detach().clone()) for q in p], lr=0.5)
    fused.load_state_dict(copy.deepcopy(src.state_dict()))  # load_state_dict keeps f32 tensors by reference
    sd = fused.state_dict()
    assert sd["param_groups"][0]["lr"] == 0.1 and sd["param_groups"][0]["momentum"] == kw.get("momentum", 0)
    for st in sd["state"].values():
        assert set(st) == {"momentum_buffer"}  # torch's key, and no step count
    assert len(sd["state"]) == (2 if "momentum" in kw else 0)
    # back into torch.optim.SGD: it continues exactly as the optimizer the state came from
    q = [torch.nn.Parameter(t.detach().clone()) for t in p]
    back = torch.optim.SGD(q, lr=0.5)
    back.load_state_dict(sd)
    g = torch.Generator().manual_seed(2)
    for a, b in zip(p, q):
        a.grad = torch.randn(a.shape, generator=g)
        b.grad = a.grad.clone()
    src.step(), back.step()
    for a, b in zip(p, q):
        assert torch.equal(a, b)


def test_fused_adamw_state_dict_round_trips_through_torch_adamw():
    from src.training.optim import FusedAdamW
    p = _params()
    src = _stepped(torch.optim.AdamW, p, 3, lr=1e-2, weight_decay=0.05)
    fused = FusedAdamW([torch.nn.Parameter(q.detach().clone()) for q in p])
    fused.load_state_dict(copy.deepcopy(src.state_dict()))  # load_state_dict keeps f32 tensors by reference
    sd = fused.state_dict()
    assert sd["param_groups"][0]["weight_decay"] == 0.05
    for st in sd["state"].values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 2
    q = [torch.nn.Parameter(t.detach().clone()) for t in p]
    back = torch.optim.AdamW(q)
    back.load_state_dict(sd)
    g = torch.Generator().manual_seed(4)
    for a, b in zip(p, q):
        a.grad = torch.randn(a.shape, generator=g)
        b.grad = a.grad.clone()
    src.step(), back.step()
    for a, b in zip(p, q):
        assert torch.equal(a, b)
    # a fresh FusedAdamW's own group loads into torch.optim.AdamW too (every key torch's step reads is there)
    fresh = torch.optim.AdamW(q)
    fresh.load_state_dict(FusedAdamW(q, lr=3e-3).state_dict())
    for b in q:
        b.grad = torch.ones_like(b)
    fresh.step()
    assert fresh.param_groups[0]["lr"] == 3e-3


# ------------------------------------------------------------------------------------------------ engine
@pytest.mark.parametrize("target,kw,cls", [
    ("torch.optim.SGD", {"lr": 0.1, "momentum": 0.9, "nesterov": True}, torch.optim.SGD),
    ("torch.optim.AdamW", {"lr": 1e-3}, torch.optim.AdamW),
    ("torch.optim.Adam", {"lr": 1e-3}, torch.optim.Adam),
    ("torch.optim.Adam", {"lr": 1e-3, "decoupled_weight_decay": True}, torch.optim.Adam),
    ("torch.optim.RMSprop", {"lr": 1e-3}, torch.optim.RMSprop),
])
def test_configure_optimizers_keeps_torch_classes_for_cpu_parameters(target, kw, cls):
    from src.training.engine import LitClassifier
    lit = LitClassifier({"_target_": "tests._toy.EmitNet", "num_classes": 5, "in_samples": 16},
                        {"_target_": target, **kw})
    opt = lit.configure_optimizers()
    assert type(opt) is cls and not getattr(opt, "handles_clipping", False)
    for k, v in kw.items():
        assert opt.param_groups[0][k] == v


def test_engine_routes_every_fused_target():
    from src.training import engine, optim
    assert engine._FUSED_OPTIMIZERS == {
        "torch.optim.Adam": "FusedAdam", "src.training.optim.FusedAdam": "FusedAdam",
        "torch.optim.AdamW": "FusedAdamW", "src.training.optim.FusedAdamW": "FusedAdamW",
        "torch.optim.SGD": "FusedSGD", "src.training.optim.FusedSGD": "FusedSGD"}
    assert all(issubclass(getattr(optim, c), optim._FusedOptimizer) for c in engine._FUSED_OPTIMIZERS.values())


# ------------------------------------------------------------------------------------------------ formulas
SGD_CASES = [dict(momentum=m, nesterov=n, weight_decay=wd, dampening=d)
             for m, n, d in ((0.0, False, 0.0), (0.9, False, 0.0), (0.9, True, 0.0), (0.9, False, 0.1))
             for wd in (0.0, 1e-4)]


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(s, generator=g) for s in (1003, 64, 7)]
    grads = [[torch.randn(p.shape, generator=g) for p in ps] for _ in range(3)]
    return ps, grads


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("kw", SGD_CASES, ids=lambda kw: "-".join(f"{k[0]}{v}" for k, v in kw.items()))
def test_sgd_formula_matches_torch_sgd(kw, clip):
    """The restated sgd_kernel formula against torch.optim.SGD over 3 steps; tensor 1 misses the gradient of step 1,
    so its buffer initialises at step 2."""
    ps, grads = _tensors(11)
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    ropt = torch.optim.SGD(ref, lr=0.05, **kw)
    bufs = [None] * len(ps)
    for it in range(3):
        live = [i for i in range(len(ps)) if not (it == 0 and i == 1)]
        for i, r in enumerate(ref):
            r.grad = grads[it][i].clone() if i in live else None
        total, coef = R.clip_coef([grads[it][i] for i in live], clip)
        for i in live:
            bufs[i] = R.sgd_step(ps[i], grads[it][i], bufs[i], coef=coef, lr=0.05, **kw)
        if clip:
            want = torch.nn.utils.clip_grad_norm_(ref, clip)
            assert abs(total - float(want)) <= 1e-5 * float(want)
        ropt.step()
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p, r.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_adamw_formula_matches_torch_adamw(clip):
    """The restated AdamW kernel formula against torch.optim.AdamW over 3 steps; tensor 1 misses step 1, so its step
    count lags."""
    ps, grads = _tensors(12)
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    ropt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    ms, vs, steps = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps], [0] * len(ps)
    for it in range(3):
        live = [i for i in range(len(ps)) if not (it == 0 and i == 1)]
        for i, r in enumerate(ref):
            r.grad = grads[it][i].clone() if i in live else None
        _, coef = R.clip_coef([grads[it][i] for i in live], clip)
        for i in live:
            steps[i] += 1
            R.adamw_step(ps[i], grads[it][i], ms[i], vs[i], steps[i], coef=coef, lr=1e-2, weight_decay=1e-2)
        if clip:
            torch.nn.utils.clip_grad_norm_(ref, clip)
        ropt.step()
        for p, r in zip(ps, ref):
            torch.testing.assert_close(p, r.detach(), rtol=1e-5, atol=1e-6)
    assert steps == [3, 2, 3] == [int(ropt.state[r]["step"]) for r in ref]
