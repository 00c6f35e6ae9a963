"""Restatement of LeafModel's trunk and classifier behind the frontend of tests/_leaf_ref.py: the checker of
tests/test_leaf_model_cpu.py, tests/test_gpu_leaftrunk.py and tests/test_gpu_leaf_model.py.  Written from the
formulas (unfold + einsum convolutions, explicit BatchNorm sums, reshape + max pooling), in the dtype of the
parameters it is handed: float64 to check, float32 to measure the arithmetic floor of the graph.

Two layers:
  * per-kernel functions on channels-last maps (n, t, c), explicit forward and backward formulas, fed a kernel's
    own input bits: ``winners``, ``bn_batch_stats``, ``apply``, ``time_mean``, ``bwd_gather``, ``bwd_apply``;
  * per-stage functions in the reference's channels-first layout (``conv1d``, ``bn_relu_pool``, ``mlp_layer``)
    and ``model_step`` = frontend + three blocks + time mean + classifier + soft-label CE, backward by autograd.

``bf16=True`` rounds what the kernels round in BF16 mode: the waveform, the Gabor bank and the backward's scaled
energy tile (as tests/_leaf_ref.py), every GEMM weight operand, and every stored activation and activation
gradient (y, z_l, the pooled maps, the time mean, u_j, a_j and their gradients).  Statistics, scale / shift, the
logits and the parameter gradients stay unrounded.
"""
from __future__ import annotations

import torch

from tests import _leaf_ref as R

BN_EPS = 1e-5
MOMENTUM = 0.1
TRUNK = ((0, 1, 5, 4), (4, 5, 3, 4), (8, 9, 3, 2))  # (conv index, BN index, kernel, pool) in conv_block
MLP = ((0, 1), (4, 5), (8, 9))                       # (Linear, BatchNorm1d) in classifier


def _bf(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _RoundFwd(torch.autograd.Function):  # operand rounding: the gradient is the f32 master's
    @staticmethod
    def forward(ctx, t):
        return _bf(t)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBoth(torch.autograd.Function):  # a stored activation: its gradient is stored in bf16 too
    @staticmethod
    def forward(ctx, t):
        return _bf(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


class _RoundBwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return _bf(g)


def _op(t, bf16):
    return _RoundFwd.apply(t) if bf16 else t


def _act(t, bf16):
    return _RoundBoth.apply(t) if bf16 else t


# ------------------------------------------------------------------------------------------- per-kernel (n, t, c)
def winners(z: torch.Tensor, gamma: torch.Tensor, k: int):
    """(win (n, t // k, c), argmax int64): raw max for gamma > 0, raw min for gamma < 0, first position for
    gamma == 0; first occurrence on ties."""
    n, t, c = z.shape
    ot = t // k
    w = z[:, :ot * k].reshape(n, ot, k, c)
    key = w * torch.sign(gamma).to(z.dtype)
    best = key.max(dim=2, keepdim=True).values
    first = (key == best).to(torch.int64) * torch.arange(k, 0, -1).view(1, 1, k, 1)  # largest at the first hit
    arg = first.argmax(dim=2)
    return torch.gather(w, 2, arg.unsqueeze(2)).squeeze(2), arg


def bn_batch_stats(z: torch.Tensor):
    """(mean, biased var) over every frame of every clip."""
    f = z.reshape(-1, z.shape[-1])
    mean = f.mean(0)
    return mean, ((f - mean) ** 2).mean(0)


def scale_shift(gamma, beta, mean, var, eps: float = BN_EPS):
    invstd = 1.0 / torch.sqrt(var + eps)
    return gamma * invstd, beta - mean * gamma * invstd, invstd


def apply(win, scale, shift):
    return torch.relu(win * scale + shift)


def time_mean(win, scale, shift):
    return apply(win, scale, shift).mean(1)


def bwd_gather(dout, win, scale, shift, mean, invstd, mean_mode: bool = False):
    """(gm, dgamma, dbeta, v): v = scale * win + shift, the ReLU argument (its sign decides the mask)."""
    if mean_mode:
        dout = (dout / win.shape[1]).unsqueeze(1).expand_as(win)
    v = win * scale + shift
    gm = dout * (v > 0)
    xhat = (win - mean) * invstd
    return gm, (gm * xhat).sum((0, 1)), gm.sum((0, 1)), v


def bwd_apply(gm, arg, z, gamma, mean, invstd, dgamma, dbeta, k: int):
    """(dz, dbias): dz = gamma invstd (g - dbeta / P - xhat dgamma / P), g = gm scattered to the argmax frames."""
    n, t, c = z.shape
    ot = t // k
    g = torch.zeros_like(z)
    gw = torch.zeros(n, ot, k, c, dtype=z.dtype)
    gw.scatter_(2, arg.unsqueeze(2), gm.unsqueeze(2))
    g[:, :ot * k] = gw.reshape(n, ot * k, c)
    P = n * t
    xhat = (z - mean) * invstd
    dz = gamma * invstd * (g - dbeta / P - xhat * dgamma / P)
    return dz, dz.sum((0, 1))


# ------------------------------------------------------------------------------------------- per-stage (B, C, T)
def conv1d(x, w, b):
    """x (B, Cin, T), w (Cout, Cin, k), zero padding k // 2."""
    k = w.shape[-1]
    win = torch.nn.functional.pad(x, (k // 2, k // 2)).unfold(2, k, 1)  # (B, Cin, T, k)
    return torch.einsum("bctk,ock->bot", win, w) + b.view(1, -1, 1)


def bn_train(z, gamma, beta, dims):
    """Training-mode BatchNorm: (zhat * gamma + beta, mean, unbiased var)."""
    mean = z.mean(dims, keepdim=True)
    var = ((z - mean) ** 2).mean(dims, keepdim=True)
    n = z.numel() // z.shape[1]
    shape = [1, -1] + [1] * (z.ndim - 2)
    out = (z - mean) / torch.sqrt(var + BN_EPS) * gamma.view(shape) + beta.view(shape)
    return out, mean.flatten(), var.flatten() * n / max(n - 1, 1)


def bn_eval(z, gamma, beta, rm, rv):
    shape = [1, -1] + [1] * (z.ndim - 2)
    return (z - rm.view(shape)) / torch.sqrt(rv.view(shape) + BN_EPS) * gamma.view(shape) + beta.view(shape)


def max_pool(a, k):
    B, C, T = a.shape
    return a[:, :, :T // k * k].reshape(B, C, T // k, k).max(-1).values


def energy(x, w, pool: int, bf16: bool):
    """P (B, F, Tp) in w's dtype, differentiable in w (the frontend of tests/_leaf_ref.py on conv1d)."""
    F, Kt = w.shape[1], w.shape[2]
    x = x.to(w.dtype)
    if bf16:
        x = _bf(x)
    z = torch.nn.functional.conv1d(x[:, None, :], _op(w, bf16).reshape(2 * F, 1, Kt), padding=Kt // 2)
    if bf16:
        z = _RoundBwd.apply(z)  # the backward's scaled tile (2 / pool) gP z is rounded
    e = z[:, :F] ** 2 + z[:, F:] ** 2
    Tp = x.shape[1] // pool
    return e[:, :, :Tp * pool].reshape(x.shape[0], F, Tp, pool).mean(-1)


def model_step(sd: dict, x, labels, Kt: int, pool: int = 160, sr: int = 44100, bf16: bool = False,
               training: bool = True):
    """One forward (+ loss) of LeafModel from a state dict of leaf tensors (float64 or float32; requires_grad where
    a gradient is wanted).  Returns (logits, loss, new_running) with new_running = {key: tensor} of the BatchNorm
    running_mean / running_var after the step (training) -- call loss.backward() for the gradients."""
    dt = sd["pcen.r"].dtype
    w = R.filters(sd["gabor.center_freqs"], sd["gabor.bandwidths"], Kt, sr)
    P = energy(torch.as_tensor(x), w, pool, bf16)
    h = _act(R.pcen(P, sd["pcen.r"], sd["pcen.delta"]), bf16)
    running = {}

    def bn(prefix, z, dims):
        g, b = sd[prefix + ".weight"], sd[prefix + ".bias"]
        if not training:
            return bn_eval(z, g, b, sd[prefix + ".running_mean"], sd[prefix + ".running_var"])
        out, mean, unb = bn_train(z, g, b, dims)
        running[prefix + ".running_mean"] = ((1 - MOMENTUM) * sd[prefix + ".running_mean"] + MOMENTUM * mean).detach()
        running[prefix + ".running_var"] = ((1 - MOMENTUM) * sd[prefix + ".running_var"] + MOMENTUM * unb).detach()
        return out

    for l, (ci, bi, k, pk) in enumerate(TRUNK):
        z = _act(conv1d(h, _op(sd[f"conv_block.{ci}.weight"], bf16), sd[f"conv_block.{ci}.bias"]), bf16)
        a = max_pool(torch.relu(bn(f"conv_block.{bi}", z, (0, 2))), pk)
        h = _act(a.mean(-1), bf16) if l == 2 else _act(a, bf16)
    for li, bi in MLP:
        u = _act(h @ _op(sd[f"classifier.{li}.weight"], bf16).T + sd[f"classifier.{li}.bias"], bf16)
        h = _act(torch.relu(bn(f"classifier.{bi}", u, (0,))), bf16)
    logits = h @ _op(sd["classifier.12.weight"], bf16).T + sd["classifier.12.bias"]
    loss = None
    if labels is not None:
        y = torch.as_tensor(labels).to(dt)
        loss = -torch.sum(y * torch.log(torch.softmax(logits, dim=1) + 1e-8), dim=1).mean()
    return logits, loss, running


def case_waveform(seed: int, B: int, T: int, pool: int = 160, amp: float = 100.0):
    """(B, T) float32 clips with strong dynamics at the scale the model sees: uniform noise times a gain that
    changes every pooled frame (two decades, per clip and frame), times a per-clip level (one decade over the
    batch), times ``amp``; all from oracle.synth.hash_uniform.

    Why not oracle.synth.synth_waveform: peak-normalised white noise has the same energy in every pooled frame, so
    PCEN's output log(P / (eps + M)^r + delta) is the constant log(delta + ~0.7) plus a ripple of about 0.01 --
    three bf16 steps at that magnitude -- and the BatchNorm behind conv1 divides by that ripple: the bf16 mode's
    error against float64 was 0.3 of the logits.  Here P / M^r spans 0.1 .. 100 around delta = 2, PCEN's output
    spans ~0.7 .. 4.5, and a bf16 step is 1e-3 of that range."""
    import numpy as np

    from oracle.synth import hash_uniform
    nseg = -(-T // pool)
    noise = hash_uniform(seed, (B, T)).astype(np.float64)
    env = 10.0 ** hash_uniform(seed + 7, (B, nseg), -2.0, 0.0).astype(np.float64)
    level = 10.0 ** np.linspace(-1.0, 0.0, B)[:, None]
    return (amp * noise * np.repeat(env, pool, axis=1)[:, :T] * level).astype(np.float32)


def hash_init(keys_shapes, seed: int) -> dict:
    """Deterministic stand-in for the default ``nn`` initialisation, regenerated bit-identically wherever it is
    needed (the trunk's 1.6 M weights do not fit a fixture): Conv1d / Linear weights and biases uniform in
    +-1 / sqrt(fan_in) (the bound of torch's default), BatchNorm weights in [0.5, 1.5] and biases in [-0.2, 0.2]
    so no gradient is trivially zero; float32 numpy arrays from oracle.synth.hash_uniform(seed + position)."""
    import math

    import numpy as np

    from oracle.synth import hash_uniform
    out, fan = {}, {}
    for i, (k, shape) in enumerate(keys_shapes):
        if not (k.startswith("conv_block.") or k.startswith("classifier.")) or "running_" in k or "num_batches" in k:
            continue
        stem = k.rsplit(".", 1)[0]
        if k.endswith(".weight") and len(shape) >= 2:
            fan[stem] = int(np.prod(shape[1:]))
        if stem in fan:
            b = 1.0 / math.sqrt(fan[stem])
            out[k] = hash_uniform(seed + i, tuple(shape), -b, b).astype(np.float32)
        elif k.endswith(".weight"):
            out[k] = hash_uniform(seed + i, tuple(shape), 0.5, 1.5).astype(np.float32)
        else:
            out[k] = hash_uniform(seed + i, tuple(shape), -0.2, 0.2).astype(np.float32)
    return out


N_SAMPLED, SAMPLE_SEED = 96, 8555  # tests/golden/make_golden_leaf_model.py
LARGE = ("conv_block.0.weight", "conv_block.4.weight", "conv_block.8.weight", "classifier.0.weight",
         "classifier.4.weight", "classifier.8.weight")
BN_FED = ("conv_block.0.bias", "conv_block.4.bias", "conv_block.8.bias", "classifier.0.bias", "classifier.4.bias",
          "classifier.8.bias")


def sample_indices(j: int, n: int):
    import numpy as np

    from oracle.synth import hash_uniform
    idx = (hash_uniform(SAMPLE_SEED + j, (N_SAMPLED,), 0.0, 1.0).astype(np.float64) * n).astype(np.int64)
    return idx.clip(0, n - 1)


_CASES: dict = {}


def case(gm: dict, name: str):
    """(dims dict, x [B][T] f32, y one-hot [B][C] f32, state {key: f32 numpy}) of fixture case ``name``; the state
    is the model's full initial state_dict (gabor / pcen from the fixture, the rest from hash_init, default
    BatchNorm buffers)."""
    if name in _CASES:
        return _CASES[name]
    import numpy as np

    from src.models.leaf import LeafModel
    F, Kt, T, B, C, pool = (int(v) for v in gm[f"{name}__dims"])
    sx, sl, si = (int(v) for v in gm[f"{name}__seeds"])
    x = torch.from_numpy(case_waveform(sx, B, T))
    y = torch.zeros(B, C)
    y[torch.arange(B), torch.from_numpy(gm[f"{name}__labels"])] = 1.0
    base = LeafModel(n_filters=F, kernel_size=Kt, num_classes=C).state_dict()
    state = {k: v.numpy().copy() for k, v in base.items()}
    for k in base:
        if k.startswith(("gabor.", "pcen.")):
            state[k] = gm[f"{name}__state__{k}"].copy()
        elif "running_mean" in k:
            state[k] = np.zeros_like(state[k])
        elif "running_var" in k:
            state[k] = np.ones_like(state[k])
    state.update(hash_init([(k, tuple(v.shape)) for k, v in base.items()], si))
    _CASES[name] = (dict(F=F, Kt=Kt, T=T, B=B, C=C, pool=pool), x, y, state)
    return _CASES[name]


def tensors(state: dict, dtype=torch.float64, grad: bool = True) -> dict:
    """Leaf tensors of a numpy state dict in ``dtype`` (parameters with requires_grad)."""
    sd = {}
    for k, v in state.items():
        t = torch.from_numpy(v.copy())
        if t.is_floating_point():
            t = t.to(dtype)
            if grad and "running_" not in k and k not in ("gabor.window", "pcen.alpha"):
                t.requires_grad_(True)
        sd[k] = t
    return sd


_RUNS: dict = {}


FLOOR_THREADS = (16, 5)  # float32 floors: the per-quantity maximum over these intra-op thread counts


def run_case(gm: dict, name: str, dtype=torch.float64, bf16: bool = False, threads: int | None = None):
    """The restatement's train step + eval forward of a fixture case, computed once per (case, dtype, bf16, threads):
    dict(logits, loss, eval_logits, grads {param: tensor}, running {buffer: tensor}).  ``threads`` pins torch's
    intra-op thread count for the run (it decides how the float32 sums are split)."""
    key = (name, dtype, bf16, threads)
    if key in _RUNS:
        return _RUNS[key]
    if threads is not None:
        before = torch.get_num_threads()
        torch.set_num_threads(threads)
        try:
            _RUNS[key] = run_case(gm, name, dtype, bf16)
            del _RUNS[(name, dtype, bf16, None)]
        finally:
            torch.set_num_threads(before)
        return _RUNS[key]
    d, x, y, state = case(gm, name)
    sd = tensors(state, dtype)
    logits, loss, running = model_step(sd, x, y, d["Kt"], d["pool"], bf16=bf16)
    loss.backward()
    grads = {k: v.grad.detach() for k, v in sd.items() if torch.is_tensor(v) and v.grad is not None}
    sd2 = tensors(state, dtype, grad=False)
    sd2.update(running)
    with torch.no_grad():
        ev, _, _ = model_step(sd2, x, None, d["Kt"], d["pool"], bf16=bf16, training=False)
    _RUNS[key] = dict(logits=logits.detach(), loss=loss.detach(), eval_logits=ev, grads=grads, running=running)
    return _RUNS[key]


def run_quantities(run: dict, param_order) -> dict:
    """{quantity: float64 numpy array} of a run (run_case's layout) in the fixture's form: logits, loss,
    eval_logits, every gradient the fixture stores (sampled entries / channel sums for the large weights) and the
    running buffers.  ``param_order``: the model's named_parameters() keys (the sampling seeds follow it)."""
    out = {q: run[q].double().cpu().numpy() for q in ("logits", "loss", "eval_logits")}
    for j, k in enumerate(param_order):
        if k in BN_FED or k == "pcen.alpha":
            continue
        g = run["grads"][k].double().cpu().numpy()
        if k in LARGE:
            out["gs:" + k] = g.ravel()[sample_indices(j, g.size)]
            if g.ndim == 3:
                out["gsum:" + k] = g.reshape(g.shape[0], -1).sum(1)
        else:
            out["g:" + k] = g
    for k, v in run["running"].items():
        out["run:" + k] = v.double().cpu().numpy()
    return out


def fixture_quantities(gm: dict, name: str) -> dict:
    pre = f"{name}__"
    tag = {"g__": "g:", "gs__": "gs:", "gsum__": "gsum:", "run__": "run:"}
    out = {q: gm[pre + q] for q in ("logits", "loss", "eval_logits")}
    for k, v in gm.items():
        if k.startswith(pre):
            for a, b in tag.items():
                if k[len(pre):].startswith(a) and not k.endswith("num_batches_tracked"):
                    out[b + k[len(pre) + len(a):]] = v
    return out


def errors(a: dict, b: dict) -> dict:
    """{quantity: tests._util.rel_err(a, b)} over the quantities of ``b``."""
    from tests._util import rel_err
    return {q: rel_err(a[q], b[q]) for q in b}


def compare(gm: dict, name: str, got: dict, param_order) -> dict:
    """{quantity: relative error} of a run against the fixture."""
    return errors(run_quantities(got, param_order), fixture_quantities(gm, name))


def float32_floor(gm: dict, name: str, param_order, bf16: bool = False) -> dict:
    """{quantity: error} of the restatement evaluated in float32 on the CPU against its own float64 evaluation with
    the same roundings (for bf16 = False that is the fixture, to 1e-10): what float32 arithmetic costs on this graph.
    One float32 evaluation is one draw of the rounding -- for a single number such as the loss it can land on the
    exact value -- so the floor is the per-quantity maximum over FLOOR_THREADS pinned thread counts (different
    splits of every sum), which also makes it the same on every host with that many cores."""
    ref = run_quantities(run_case(gm, name, torch.float64, bf16), param_order)
    out = {}
    for t in FLOOR_THREADS:
        e = errors(run_quantities(run_case(gm, name, torch.float32, bf16, threads=t), param_order), ref)
        out = {q: max(v, out.get(q, 0.0)) for q, v in e.items()}
    # a result handed back in float32 carries up to half a unit in the last place whatever computed it
    return {q: max(v, 2.0 ** -24) for q, v in out.items()}
