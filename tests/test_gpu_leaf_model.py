"""GPU: the whole LeafModel (energy kernel -> channels-last PCEN -> three conv blocks -> time mean -> classifier,
forward and backward) against the reference's float64 fixture tests/golden/golden_leaf_model.npz.

test_against_fixture.  Per quantity (logits, loss, every stored gradient, the running buffers, the eval-mode
logits), errors are tests._util.rel_err (max |a - b| / max |b|) against the fixture and the floor is the error of the
restatement tests/_leaf_model_ref.py evaluated on the CPU, which involves none of the code under test:
  f32 mode  floor = its float32 evaluation (maximum over two pinned thread counts, float32_floor); every floor must
            be <= 1e-3 (else the case is ill-conditioned) and the model may be 10x its floor;
  bf16 mode floor = its float64 evaluation with the kernels' bf16 roundings; the model may be 3x its floor, and for
            the forward quantities (logits, loss, eval logits, running buffers) 3x the floor must stay below 0.5, so
            the check cannot pass on garbage.
The gradients of the bf16 mode cannot be pinned that way: a ReLU or max-pool decision that a 2^-9 rounding tips
moves whole gradient entries, the restatement with the same roundings is 0.2-0.7 away from float64 in most gradients
(0.35 in relative L2) on any input we tried, and two correct bf16 evaluations that differ in one rounding differ by
as much.  test_stagewise pins them instead: every stage of the forward and of the backward, in both modes, is
recomputed in float64 from the tensors the model itself stored on the GPU (its own input bits, so no decision can
tip), and must agree to the kernel tests' bounds -- 1e-5 forward, 1e-4 gradients and reductions of the largest
entry, plus one bf16 step (2^-8 relative) per element where the output is stored in bf16.
The gradients of the six biases in front of a BatchNorm are exactly zero in exact arithmetic: they are bounded
absolutely, |dbias[c]| <= tol * sum_rows |dz[r][c]| with tol = 1e-5 (f32) or 2^-8 (bf16, the rounding of each
stored dz).
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _leaf_model_ref as M

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
BN_FED_SRC = {"conv_block.0.bias": ("dz", 0), "conv_block.4.bias": ("dz", 1), "conv_block.8.bias": ("dz", 2),
              "classifier.0.bias": ("du", 0), "classifier.4.bias": ("du", 1), "classifier.8.bias": ("du", 2)}


@pytest.fixture(scope="module")
def gm():
    return dict(np.load(REPO / "tests" / "golden" / "golden_leaf_model.npz", allow_pickle=False))


def build(gm, name, compute, dev, p_drop=0.0):
    from src.models.leaf import LeafModel
    d, x, y, state = M.case(gm, name)
    m = LeafModel(n_filters=d["F"], kernel_size=d["Kt"], num_classes=d["C"], compute_dtype=compute)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = p_drop
    return m.to(dev).train(), x.to(dev), y.to(dev)


def step(m, x, y):
    """One train-mode forward + soft-label CE + backward: (logits, loss, {param: grad})."""
    from src.miaudio import kernels as K
    for p in m.parameters():
        p.grad = None
    logits = m(x)
    loss, dlogits, _ = K.soft_ce(logits.detach(), y, input_sigmoid=False)
    logits.backward(dlogits)
    return logits.detach(), loss.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


class capture:
    """Collects what _LeafTrunk hands its test hook ("forward": saved tensors, "backward": dv / du / dz / dinp)."""

    def __enter__(self):
        from src.models import leaf
        self.got = {}
        leaf._LeafTrunk.capture = lambda kind, d: self.got.__setitem__(kind, dict(d))
        return self.got

    def __exit__(self, *exc):
        from src.models import leaf
        leaf._LeafTrunk.capture = None
        return False


def run_gpu(gm, name, compute, dev):
    m, x, y = build(gm, name, compute, dev)
    with capture() as cap:
        logits, loss, grads = step(m, x[:, None, :], y)
    running = {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k}
    tracked = [int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")]
    m.eval()
    with torch.no_grad():
        ev = m(x[:, None, :])
    return m, dict(logits=logits, loss=loss, eval_logits=ev, grads=grads, running=running), cap, tracked


FORWARD_Q = ("logits", "loss", "eval_logits")


@pytest.mark.parametrize("compute,margin", [("f32", 10.0), ("bf16", 3.0)])
@pytest.mark.parametrize("name", ["M1", "M2"])
def test_against_fixture(cuda, gm, name, compute, margin):
    m, got, cap, tracked = run_gpu(gm, name, compute, cuda)
    dbg = cap["backward"]
    order = [k for k, _ in m.named_parameters()]
    assert got["logits"].dtype == torch.float32 and bool(torch.isfinite(got["logits"]).all())
    assert all(g.dtype == torch.float32 and bool(torch.isfinite(g).all()) for g in got["grads"].values())
    assert "pcen.alpha" not in got["grads"] and tracked == [1] * 6
    errs = M.compare(gm, name, got, order)
    if compute == "f32":
        floor = M.float32_floor(gm, name, order)
        bad = {q: v for q, v in floor.items() if v > 1e-3}
        assert not bad, f"ill-conditioned case: float32 floors over 1e-3: {bad}"
    else:
        floor = M.compare(gm, name, M.run_case(gm, name, torch.float64, bf16=True), order)
        bad = {q: v for q, v in floor.items() if (q in FORWARD_Q or q.startswith("run:")) and margin * v >= 0.5}
        assert not bad, f"ill-conditioned case: {margin} x the bf16 floor of a forward quantity reaches 0.5: {bad}"
    over = {}
    for q in sorted(errs):
        flag = "" if errs[q] <= margin * floor[q] else "  <-- over"
        print(f"{name} {compute} {q:34s} err {errs[q]:.3e}  floor {floor[q]:.3e}  bound {margin * floor[q]:.3e}{flag}")
        if flag:
            over[q] = (errs[q], margin * floor[q])
    # the biases in front of a BatchNorm: absolute bound against the column sums of |dz| of the same backward
    tol = 1e-5 if compute == "f32" else 2.0 ** -8
    for k, (kind, i) in BN_FED_SRC.items():
        dz = dbg[kind][i].float()
        lim = tol * dz.abs().reshape(-1, dz.shape[-1]).sum(0)
        g = got["grads"][k].abs()
        print(f"{name} {compute} {k}: max |dbias| / (tol sum |dz|) = {float((g / lim.clamp_min(1e-30)).max()):.3f}")
        if not bool((g <= lim).all()):
            over[k] = "absolute bound"
    assert not over, over


def test_dropout_mask(cuda, gm):
    """p = 0.3: among the entries the ReLU passes, the dropped fraction of each layer is within 5 sigma of 0.3, the
    kept ones are scaled by 1 / 0.7, and the backward is zero exactly where the forward was."""
    m, x, y = build(gm, "M1", "f32", cuda, p_drop=0.3)
    with capture() as cap:
        step(m, x, y)
    for j, ml in enumerate(cap["forward"]["mlp"]):
        v = ml["u"] * ml["bn"].scale + ml["bn"].shift
        passed = v > 1e-6  # clear of the ReLU threshold
        n = int(passed.sum())
        dropped = int((passed & (ml["a"] == 0)).sum())
        sigma = (0.3 * 0.7 / n) ** 0.5
        print(f"layer {j}: dropped {dropped} of {n} ({dropped / n:.4f}), 5 sigma = {5 * sigma:.4f}")
        assert abs(dropped / n - 0.3) <= 5 * sigma
        kept = passed & (ml["a"] != 0)
        size = (ml["u"] * ml["bn"].scale).abs() + ml["bn"].shift.abs()  # v is a difference of terms this large
        assert bool(((ml["a"] - v / 0.7).abs()[kept] <= 1e-5 * size[kept]).all())
        dv = cap["backward"]["dv"][j]
        assert not bool(dv[ml["a"] == 0].any())
        assert bool((dv[kept] != 0).float().mean() > 0.99)


def test_eval_single_clip_and_input_ranks(cuda, gm):
    m, x, _ = build(gm, "M1", "bf16", cuda)
    with pytest.raises(ValueError):
        m(x[:1])
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        one = m(x[:1])
        a, b = m(x), m(x[:, None, :])
    assert one.shape == (1, 10) and bool(torch.isfinite(one).all())
    assert torch.equal(a, b)
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())  # no statistics updated
    m.train()
    assert torch.equal(m(x), m(x[:, None, :]))  # batch statistics: the buffers take no part


@pytest.mark.parametrize("compute", ["f32", "bf16"])
def test_repeatable_and_stream_independent(cuda, gm, compute):
    m, x, y = build(gm, "M1", compute, cuda)
    l1, loss1, g1 = step(m, x, y)
    l2, loss2, g2 = step(m, x, y)
    assert torch.equal(l1, l2) and torch.equal(loss1, loss2) and set(g1) == set(g2)
    assert all(torch.equal(g1[k], g2[k]) for k in g1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l3, loss3, g3 = step(m, x, y)
    side.synchronize()
    assert torch.equal(l1, l3) and all(torch.equal(g1[k], g3[k]) for k in g1)


def test_autocast_selects_bf16(cuda, gm):
    from src.miaudio import lib as L
    m, x, _ = build(gm, "M1", None, cuda)
    assert m._compute_code() == L.F32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert m._compute_code() == L.BF16
        z = m(x)
    assert z.dtype == torch.float32
    m.compute_dtype = "fp8"
    assert m._compute_code() == L.BF16


# ------------------------------------------------------------------------------------------------ stage by stage
def _d(t):
    return t.detach().float().cpu().double()


def _check(what, got, ref, bound, stored_bf16):
    """|got - ref| <= bound * max |ref| (+ one bf16 step of each element where the value is stored in bf16)."""
    got, ref = _d(got).reshape(-1), ref.reshape(-1).double()
    lim = bound * ref.abs().max() + (2.0 ** -8 * ref.abs() if stored_bf16 else 0.0)
    worst = float(((got - ref).abs() / torch.as_tensor(lim).clamp_min(1e-300)).max())
    print(f"  {what:24s} worst error / allowed {worst:.3f}")
    assert worst <= 1.0, f"{what}: {worst:.3f} of the allowed error"


@pytest.mark.parametrize("compute", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["M1", "M2"])
def test_stagewise(cuda, gm, name, compute):
    """Every stage of one train step recomputed in float64 from the model's own stored tensors."""
    from tests import _leaf_ref as R
    m, x, y = build(gm, name, compute, cuda)
    with capture() as cap:
        logits, _, grads = step(m, x, y)
    s, b = cap["forward"], cap["backward"]
    bf = compute == "bf16"
    op = (lambda w: M._bf(_d(w))) if bf else _d  # a GEMM weight operand
    B, F = s["B"], s["F"]
    sd = {k: v for k, v in m.named_parameters()}
    # PCEN, channels-last, pad channels zero
    y_cl = s["blocks"][0]["inp"]
    ref = R.pcen(_d(s["P"]), _d(sd["pcen.r"]), _d(sd["pcen.delta"])).transpose(1, 2)
    _check("pcen", y_cl[:, :, :F], ref, 1e-5, bf)
    assert not bool(y_cl[:, :, F:].any())
    # conv blocks, forward
    for l, (ci, bi, k, pk) in enumerate(M.TRUNK):
        blk = s["blocks"][l]
        cin = sd[f"conv_block.{ci}.weight"].shape[1]
        z_ref = M.conv1d(_d(blk["inp"])[:, :, :cin].transpose(1, 2), op(sd[f"conv_block.{ci}.weight"]),
                         _d(sd[f"conv_block.{ci}.bias"])).transpose(1, 2)
        _check(f"block {l} conv", blk["z"], z_ref, 1e-5, bf)
        z = _d(blk["z"])
        mean, var = M.bn_batch_stats(z)
        sc, sh, istd = M.scale_shift(_d(sd[f"conv_block.{bi}.weight"]), _d(sd[f"conv_block.{bi}.bias"]), mean, var)
        _check(f"block {l} bn scale", blk["bn"].scale, sc, 1e-4, False)
        _check(f"block {l} bn shift", blk["bn"].shift, sh, 1e-4, False)
        win, arg = M.winners(z, _d(sd[f"conv_block.{bi}.weight"]), pk)
        assert torch.equal(_d(blk["win"]), win) and torch.equal(blk["am"].cpu().long(), arg)
        nxt = s["blocks"][l + 1]["inp"] if l < 2 else s["mlp"][0]["hin"]
        ksc, ksh = _d(blk["bn"].scale), _d(blk["bn"].shift)
        _check(f"block {l} pooled", nxt, M.time_mean(win, ksc, ksh) if l == 2 else M.apply(win, ksc, ksh), 1e-5, bf)
    # classifier, forward
    for j, (li, bi) in enumerate(M.MLP):
        ml = s["mlp"][j]
        u_ref = _d(ml["hin"]) @ op(sd[f"classifier.{li}.weight"]).T + _d(sd[f"classifier.{li}.bias"])
        _check(f"mlp {j} linear", ml["u"], u_ref, 1e-5, bf)
        _check(f"mlp {j} bn relu", ml["a"], M.apply(_d(ml["u"]), _d(ml["bn"].scale), _d(ml["bn"].shift)), 1e-5, bf)
    a3 = _d(s["mlp"][2]["a"])
    _check("logits", logits, a3 @ op(sd["classifier.12.weight"]).T + _d(sd["classifier.12.bias"]), 1e-5, False)
    # classifier, backward (dropout p = 0: the DACT_NZ mask is the ReLU mask)
    p = torch.softmax(_d(logits), 1)
    yy = _d(y)
    # d/dz of -mean_b sum_c y log(softmax(z) + 1e-8)
    w = yy * p / (p + 1e-8)
    dl = (p * w.sum(1, keepdim=True) - w) / B
    dl_op = M._bf(dl) if bf else dl  # the f32 loss gradient enters both GEMMs as a bf16 operand in bf16 mode
    _check("last linear dW", grads["classifier.12.weight"], dl_op.T @ a3, 1e-4, False)
    _check("last linear db", grads["classifier.12.bias"], dl.sum(0), 1e-4, False)
    dnext, wnext = dl_op, op(sd["classifier.12.weight"])
    for j in (2, 1, 0):
        ml = s["mlp"][j]
        li, bi = M.MLP[j]
        dv_ref = (dnext @ wnext) * (_d(ml["a"]) != 0)
        _check(f"mlp {j} dv", b["dv"][j], dv_ref, 1e-4, bf)
        dv, u = _d(b["dv"][j]), _d(ml["u"])
        mean, istd = _d(ml["bn"].mean), _d(ml["bn"].invstd)
        g = dv * ((u * _d(ml["bn"].scale) + _d(ml["bn"].shift)) > 0)
        xhat = (u - mean) * istd
        dg, db = (g * xhat).sum(0), g.sum(0)
        _check(f"mlp {j} dgamma", grads[f"classifier.{bi}.weight"], dg, 1e-4, False)
        _check(f"mlp {j} dbeta", grads[f"classifier.{bi}.bias"], db, 1e-4, False)
        kdg, kdb = _d(grads[f"classifier.{bi}.weight"]), _d(grads[f"classifier.{bi}.bias"])
        du_ref = _d(sd[f"classifier.{bi}.weight"]) * istd * (g - kdb / B - xhat * kdg / B)
        _check(f"mlp {j} du", b["du"][j], du_ref, 1e-4, bf)
        du = _d(b["du"][j])
        _check(f"mlp {j} dW", grads[f"classifier.{li}.weight"], du.T @ _d(ml["hin"]), 1e-4, False)
        dnext, wnext = du, op(sd[f"classifier.{li}.weight"])
    # conv blocks, backward
    _check("dh", b["dh"], dnext @ wnext, 1e-4, bf)  # the gradient of the time mean
    dout = _d(b["dh"])
    for l in (2, 1, 0):
        ci, bi, k, pk = M.TRUNK[l]
        blk = s["blocks"][l]
        z, win = _d(blk["z"]), _d(blk["win"])
        sc, sh, mean, istd = (_d(getattr(blk["bn"], a)) for a in ("scale", "shift", "mean", "invstd"))
        gm_, dg, db, _ = M.bwd_gather(dout, win, sc, sh, mean, istd, mean_mode=(l == 2))
        _check(f"block {l} dgamma", grads[f"conv_block.{bi}.weight"], dg, 1e-4, False)
        _check(f"block {l} dbeta", grads[f"conv_block.{bi}.bias"], db, 1e-4, False)
        kdg, kdb = _d(grads[f"conv_block.{bi}.weight"]), _d(grads[f"conv_block.{bi}.bias"])
        dz_ref, _ = M.bwd_apply(gm_, blk["am"].cpu().long(), z, _d(sd[f"conv_block.{bi}.weight"]), mean, istd, kdg, kdb, pk)
        _check(f"block {l} dz", b["dz"][l], dz_ref, 1e-4, bf)
        dz = _d(b["dz"][l]).transpose(1, 2).clone().requires_grad_(False)  # (B, C, T)
        cin = sd[f"conv_block.{ci}.weight"].shape[1]
        xin = _d(blk["inp"])[:, :, :cin].transpose(1, 2).clone().requires_grad_(True)
        wop = op(sd[f"conv_block.{ci}.weight"]).clone().requires_grad_(True)
        (M.conv1d(xin, wop, torch.zeros(wop.shape[0], dtype=torch.float64)) * dz).sum().backward()
        _check(f"block {l} wgrad", grads[f"conv_block.{ci}.weight"], wop.grad, 1e-4, False)
        _check(f"block {l} dgrad", b["dinp"][l][:, :, :cin], xin.grad.transpose(1, 2), 1e-4, bf)
        dout = _d(b["dinp"][l])
    gP, dr, dd = R.pcen_bwd(_d(s["P"]), _d(sd["pcen.r"]), _d(sd["pcen.delta"]), dout[:, :, :F].transpose(1, 2))
    _check("pcen dr", grads["pcen.r"], dr, 1e-4, False)
    _check("pcen ddelta", grads["pcen.delta"], dd, 1e-4, False)
