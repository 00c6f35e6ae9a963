"""Fused gradient-clip + optimizer step on the MI355X (one norm pass + one update pass over all tensors):
FusedAdam, FusedAdamW and FusedSGD.

Replaces Lightning's ``gradient_clip_val`` (torch clip_grad_norm_, configs/base_training.yaml:51)
followed by ``torch.optim.Adam(lr, weight_decay)`` (base_training.yaml:56-59, instantiated at
src/training/engine.py:300).  Numerics follow torch's single-tensor Adam: L2 decay added to the
(clipped) gradient, ``exp_avg.lerp_(g, 1-beta1)``, ``exp_avg_sq = beta2*v + (1-beta2) g^2``,
``p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)``.  The clip coefficient is computed on the device,
so the step never synchronises with the host.  FusedAdamW is torch's AdamW (``p *= 1 - lr * wd``, then the Adam
update with no L2 term); FusedSGD is torch's single-tensor SGD with momentum, dampening, Nesterov and L2 decay
(include/miaudio_optim.h).
"""
from __future__ import annotations

import math
import weakref

import numpy as np
import torch
from torch.optim.optimizer import register_optimizer_step_pre_hook

from ..miaudio import kernels as K
from ..miaudio import lib as L


def _materialise_for_other_optimizers(opt, args, kwargs):
    """Global optimizer step pre-hook: an optimizer other than the fused ones about to step a parameter whose
    weight gradient was deferred gets the gradient materialised into ``p.grad`` first (the same GEMM), and
    the parameter stops deferring -- so torch.optim.Adam built after a FusedAdam updates FC1 from its
    first step instead of silently skipping it."""
    if isinstance(opt, _FusedOptimizer):
        return
    for grp in opt.param_groups:
        for p in grp["params"]:
            if getattr(p, "_mia_fused_adam", None) is not None:
                p._mia_fused_adam = None
            if getattr(p, "_mia_deferred", None) is not None:
                K.materialise_deferred_grad(p)


register_optimizer_step_pre_hook(_materialise_for_other_optimizers)


class _FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share: option checking, the deferral protocol and the step -- gather the tensors,
    keep the pinned pointer table, run the subclass's clip + update kernel and its GEMM form for deferred weight
    gradients, refresh the bf16 operand copies.  A subclass supplies its state and its two launches."""
    _TORCH = ""                      # the torch optimizer the subclass implements
    _DEFAULT_ONLY: dict = {}         # its options the fused kernel implements only at their defaults
    _IGNORED = ("foreach", "fused")  # implementation selectors of torch's optimizers: this is the fused one

    def _check_options(self, kw):
        name = type(self).__name__
        for k, v in kw.items():
            if k in self._IGNORED:
                continue
            if k not in self._DEFAULT_ONLY:
                raise TypeError(f"{name} got an unexpected keyword argument {k!r}")
            if bool(v) != self._DEFAULT_ONLY[k]:
                raise ValueError(f"{name} implements {self._TORCH} with {k}={self._DEFAULT_ONLY[k]} only "
                                 f"(got {k}={v}); use {self._TORCH} for this option")

    def _init_fused(self, clip):
        self.clip = float(clip or 0.0)
        self.last_total_norm = None
        self.last_precomputed = 0  # tensors whose norm came from their GEMM's per-tile sums (last step)
        self._table_key = None     # pointer table of the last step (host pinned + device copy)
        self._table = None
        self.table_builds = 0
        self.last_deferred = 0     # weight gradients applied by their fused update GEMM (last step)
        ref = weakref.ref(self)
        for p in self.param_groups[0]["params"]:
            # models may defer a wide Linear's weight gradient to this optimizer (K.defer_weight_grad) while
            # it is alive; another optimizer stepping the parameter first materialises the gradient
            # (_materialise_for_other_optimizers), and takes the parameter over
            p._mia_fused_adam = ref

    # ---- supplied by the subclass
    def _state_names(self, grp):
        """Names of the per-parameter state tensors shaped like the parameter, in kernel-table order."""
        raise NotImplementedError

    def _advance(self, p, grp):
        """Create the state of ``p`` at its first gradient and advance it by one step."""
        raise NotImplementedError

    def _tensor_values(self, ps):
        """One int per stepped tensor for the kernel, and whether the kernel needs them as a device table."""
        raise NotImplementedError

    def _launch(self, lib, grp, table, n, max_numel, max_norm_numel, first_value, tot, ws, pre, values):
        raise NotImplementedError

    def _launch_deferred(self, lib, grp, d, p, off, shadow, coef, value):
        raise NotImplementedError

    def moment_tensors(self, p):
        """The state tensors shaped like ``p`` (what GradAllReducer.sync_param gathers beside the parameter)."""
        st = self.state.get(p) or {}
        return [st[k] for k in self._state_names(self.param_groups[0]) if st.get(k) is not None]

    @torch.no_grad()
    def step(self, closure=None):
        name = type(self).__name__
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise RuntimeError(f"{name} drives one parameter group (the reference configures one)")
        grp = self.param_groups[0]
        ps = [p for p in grp["params"] if p.grad is not None or getattr(p, "_mia_deferred", None) is not None]
        if not ps:
            return loss
        dev = ps[0].device
        L.require_device(ps[0], name)
        deferred = [getattr(p, "_mia_deferred", None) for p in ps]
        for p, d in zip(ps, deferred):
            shard = getattr(p, "_mia_shard", None)
            if shard is not None and (d is None or "row0" not in d):
                # the last steps updated only this rank's row slice (GradAllReducer fc1_exchange="shard"):
                # bring every rank's rows of the parameter and moments back before a whole-tensor update
                shard[0].sync_param(p)
            if d is not None and p.grad is not None:
                raise RuntimeError("a parameter has both a gradient and a deferred weight gradient")
            if p.dtype != torch.float32 or (d is None and p.grad.dtype != torch.float32):
                raise TypeError(f"{name} keeps f32 master parameters and gradients")
            self._advance(p, grp)
        values, values_table = self._tensor_values(ps)
        gs = [None if d is not None else (p.grad if p.grad.is_contiguous() else p.grad.contiguous())
              for p, d in zip(ps, deferred)]
        # parameters with a live bf16 operand copy (K.bf16_shadow) get it rewritten in the update pass
        shadows = [getattr(p, "_mia_bf16", None) if getattr(p, "_mia_bf16_ver", None) == p._version else None
                   for p in ps]
        # gradients whose producing GEMM left per-tile sums of squares (K.sqsum_slots) skip the norm read;
        # a deferred one is in the table with a NULL gradient: norm from its sums, update by its GEMM
        pre = [d["sq"] if d is not None else K.valid_sqsum(p, g) for p, g, d in zip(ps, gs, deferred)]
        self.last_precomputed = sum(q is not None for q in pre)
        self.last_deferred = sum(d is not None for d in deferred)
        have_pre = self.last_precomputed > 0
        names = self._state_names(grp)
        rows = [[p.data_ptr() for p in ps], [0 if g is None else g.data_ptr() for g in gs]]
        rows += [[self.state[p][k].data_ptr() for p in ps] for k in names]
        rows += [[0 if sh is None else sh.data_ptr() for sh in shadows], [p.numel() for p in ps]]
        if have_pre:
            rows += [[0 if q is None else q.data_ptr() for q in pre], [0 if q is None else q.numel() for q in pre]]
        # the device pointer table is rebuilt only when a pointer changed: in steady state the caching
        # allocator hands every gradient the same storage step after step
        key = tuple(map(tuple, rows))
        if key != self._table_key:
            host = torch.tensor(rows, dtype=torch.int64).pin_memory()
            self._table = (host, host.to(dev, non_blocking=True))
            self._table_key = key
            self.table_builds += 1
        table = self._table[1]
        values_host = torch.tensor(values, dtype=torch.int32).pin_memory() if values_table else None
        values_dev = values_host.to(dev, non_blocking=True) if values_table else None
        n = len(ps)
        lib = L.load()
        ws = K.workspace(lib.mia_adam_workspace_bytes(n), dev, "adam")
        tot = torch.empty(1, dtype=torch.float32, device=dev)
        # algorithmic HBM bytes: grad read by the norm pass (4 B/param) + the update pass's reads and writes
        # (_pass_bytes: Adam's p, g, m, v read and p, m, v written are 28 B/param; SGD with a momentum buffer 20,
        # without 12) + the bf16 operand copies rewritten (2 B/param where shadowed)
        # (a sharded deferred gradient: only this rank's rows are updated and read)
        upd = [d["M"] * d["N"] if d is not None else p.numel() for p, d in zip(ps, deferred)]
        nbytes = (4 + self._pass_bytes(grp)) * sum(upd) + 2 * sum(u for u, sh in zip(upd, shadows) if sh is not None)
        nbytes -= 4 * sum(u for u, q in zip(upd, pre) if q is not None)  # no norm read of those
        for u, d in zip(upd, deferred):  # no gradient read either; the GEMM reads its two bf16 operands
            if d is not None:
                nbytes += -4 * u + 2 * d["K"] * (d["M"] + d["N"])
        with K.probe("optim.step", 0.0, nbytes):
            ns = len(names)
            self._launch(lib, grp, [table[i].data_ptr() for i in range(4 + ns)], n,
                         max((p.numel() for p, d in zip(ps, deferred) if d is None), default=1),
                         max((p.numel() for p, q in zip(ps, pre) if q is None), default=1), values[0],
                         tot.data_ptr(), ws.data_ptr(),
                         (table[4 + ns].data_ptr(), table[5 + ns].data_ptr()) if have_pre else (None, None),
                         values_dev.data_ptr() if values_table else None)
            coef = ws.data_ptr() + int(lib.mia_adam_coef_offset(n))
            for p, d, sh, v in zip(ps, deferred, shadows, values):
                if d is None:
                    continue
                off = d.get("row0", 0) * d["N"]  # a sharded gradient covers rows [row0, row0 + M) only
                self._launch_deferred(lib, grp, d, p, off, sh, coef, v)
                if "row0" in d:
                    d["shard"].after_shard_update(p, sh, d)
        self.last_total_norm = tot
        for p, sh in zip(ps, shadows):
            if sh is not None:
                p._mia_bf16_ver = p._version  # the copy now matches the updated parameter
        for p in ps:
            p._mia_sqsum = None  # consumed (or stale): the next step's gradient brings its own
            p._mia_deferred = None
        self._keep = (gs, pre, values_host, values_dev, deferred)  # alive until the next step (async use)
        return loss


class FusedAdam(_FusedOptimizer):
    _TORCH = "torch.optim.Adam"
    # torch.optim.Adam options the fused kernel implements only at their defaults
    _DEFAULT_ONLY = {"amsgrad": False, "maximize": False, "capturable": False, "differentiable": False,
                     "decoupled_weight_decay": False}
    _CLIP, _GEMM = "mia_clip_adam", "mia_gemm_adam"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, clip: float = 0.0, **kw):
        self._check_options(kw)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **self._extra_defaults())
        super().__init__(params, defaults)
        self._init_fused(clip)

    def _extra_defaults(self):
        return {}

    def _state_names(self, grp):
        return ("exp_avg", "exp_avg_sq")

    def _pass_bytes(self, grp):
        return 28

    def _advance(self, p, grp):
        st = self.state[p]
        if not st:
            st["step"] = torch.zeros((), dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["step"] += 1

    def _tensor_values(self, ps):
        # torch's Adam keeps one step count per parameter; they differ only after a parameter missed
        # gradients, and then the kernel takes the per-tensor counts
        steps = [int(self.state[p]["step"].item()) for p in ps]
        return steps, any(v != steps[0] for v in steps)

    def _launch(self, lib, grp, table, n, max_numel, max_norm_numel, step, tot, ws, pre, steps):
        b1, b2 = grp["betas"]
        L.check(getattr(lib, self._CLIP)(*table, n, max_numel, max_norm_numel, float(grp["lr"]), float(b1),
                                         float(b2), float(grp["eps"]), float(grp["weight_decay"]), step,
                                         self.clip, tot, ws, pre[0], pre[1], steps, L.stream_ptr()), self._CLIP)

    def _deferred_tail(self, grp):
        return (float(grp["weight_decay"]),)

    def _launch_deferred(self, lib, grp, d, p, off, sh, coef, st):
        b1, b2 = grp["betas"]
        # the bias corrections exactly as mia_clip_adam forms them: f32 lr / betas, double pow
        lr32, b1_32, b2_32 = (float(np.float32(v)) for v in (grp["lr"], b1, b2))
        lr_bc1 = lr32 / (1.0 - math.pow(b1_32, st))
        bc2_sqrt = math.sqrt(1.0 - math.pow(b2_32, st))
        L.check(getattr(lib, self._GEMM)(d["A"], d["B"], d["M"], d["N"], d["K"], p.data_ptr() + 4 * off,
                                         self.state[p]["exp_avg"].data_ptr() + 4 * off,
                                         self.state[p]["exp_avg_sq"].data_ptr() + 4 * off,
                                         0 if sh is None else sh.data_ptr() + 2 * off, d["N"], coef, lr_bc1,
                                         bc2_sqrt, float(b1), float(b2), float(grp["eps"]),
                                         *self._deferred_tail(grp), L.stream_ptr()), self._GEMM)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW (Adam with decoupled weight decay) on mia_clip_adamw / mia_gemm_adamw."""
    _TORCH = "torch.optim.AdamW"
    _DEFAULT_ONLY = {"amsgrad": False, "maximize": False, "capturable": False, "differentiable": False}
    _CLIP, _GEMM = "mia_clip_adamw", "mia_gemm_adamw"

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, clip: float = 0.0, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip=clip, **kw)

    def _extra_defaults(self):
        # the rest of torch.optim.AdamW's group, so that a state_dict() loads into it and steps
        return dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                    decoupled_weight_decay=True)

    def _deferred_tail(self, grp):
        return (float(grp["lr"]), float(grp["weight_decay"]))


class FusedSGD(_FusedOptimizer):
    """torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay) on mia_clip_sgd / mia_gemm_sgd.  The state
    is torch's: ``momentum_buffer`` per parameter, created at the parameter's first gradient, none at momentum 0."""
    _TORCH = "torch.optim.SGD"
    _DEFAULT_ONLY = {"maximize": False, "differentiable": False}

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, clip: float = 0.0, **kw):
        self._check_options(kw)
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        # torch.optim.SGD's whole group, so that a state_dict() loads into it and steps
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=False, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults)
        self._init_fused(clip)
        self._first = {}  # parameters whose buffer this step creates (_advance -> _tensor_values)

    def _state_names(self, grp):
        return ("momentum_buffer",) if grp["momentum"] != 0 else ()

    def _pass_bytes(self, grp):
        return 20 if grp["momentum"] != 0 else 12  # p, g (and the buffer) read; p (and the buffer) written

    def _advance(self, p, grp):
        st = self.state[p]
        first = grp["momentum"] != 0 and st.get("momentum_buffer") is None
        if first:  # torch clones the gradient here; the kernel writes it (first-use flag)
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        self._first[p] = first

    def _tensor_values(self, ps):
        first = [int(self._first.pop(p)) for p in ps]
        return first, any(first)

    def _rule(self, grp):
        return (float(grp["lr"]), float(grp["momentum"]), float(grp["dampening"]), float(grp["weight_decay"]),
                int(bool(grp["nesterov"])))

    def _launch(self, lib, grp, table, n, max_numel, max_norm_numel, first0, tot, ws, pre, first):
        if grp["momentum"] == 0:
            table = table[:2] + [None] + table[2:]  # no buffer table
        lr, mom, damp, wd, nesterov = self._rule(grp)
        L.check(lib.mia_clip_sgd(*table, n, max_numel, max_norm_numel, lr, mom, damp, wd, nesterov, self.clip, tot,
                                 ws, pre[0], pre[1], first, L.stream_ptr()), "mia_clip_sgd")

    def _launch_deferred(self, lib, grp, d, p, off, sh, coef, first):
        buf = self.state[p]["momentum_buffer"].data_ptr() + 4 * off if grp["momentum"] != 0 else None
        L.check(lib.mia_gemm_sgd(d["A"], d["B"], d["M"], d["N"], d["K"], p.data_ptr() + 4 * off, buf,
                                 0 if sh is None else sh.data_ptr() + 2 * off, d["N"], coef, *self._rule(grp), first,
                                 L.stream_ptr()), "mia_gemm_sgd")
