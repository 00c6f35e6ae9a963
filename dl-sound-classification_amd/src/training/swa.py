"""Stochastic weight averaging as Lightning 2.5's ``StochasticWeightAveraging`` callback schedules it (the
reference builds it from ``cfg.swa``, src/training/callbacks.py:71-79), on the lite Trainer's hooks.

With E = ``trainer.max_epochs`` and S = ``int(E * swa_epoch_start)`` (or the int itself): ``swa_start =
max(S - 1, 0)``, ``swa_end = E - 1``.  At the start of epoch ``swa_start`` the trainer's scheduler becomes torch's
``SWALR`` (annealing to ``swa_lrs``); at the start of every epoch in ``[swa_start, swa_end]`` the parameters
enter the running average (K.swa_update: one HIP pass over all tensors).  A model with BatchNorm runs one more,
forward-only epoch E: the average is transferred into the parameters (K.swa_transfer, which also rewrites their
bf16 operand copies), every BatchNorm is reset and switched to the cumulative moving average (``momentum=None``),
and one pass over the train loader re-estimates the statistics; then the momenta return.  A model without
BatchNorm takes the transfer when the loop ends after epoch E - 1.  A loop that stops early transfers nothing.

CPU parameters (``trainer.accelerator=cpu`` plumbing) take the same f32 expression on torch ops.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.optim.swa_utils import SWALR

_BatchNorm = nn.modules.batchnorm._BatchNorm


def swa_window(max_epochs: int, swa_epoch_start) -> tuple[int, int]:
    """(swa_start, swa_end), 0-based epochs."""
    s = int(max_epochs * swa_epoch_start) if isinstance(swa_epoch_start, float) else int(swa_epoch_start)
    return max(s - 1, 0), max_epochs - 1


def average_(avg: torch.Tensor, p: torch.Tensor, n_averaged: int) -> None:
    """What mia_swa_update computes, on torch ops: one f32 subtract, one true divide (a tensor divisor: a Python
    scalar may be folded into a multiply by its reciprocal), one add."""
    if n_averaged == 0:
        avg.copy_(p)
    else:
        avg.add_((p - avg) / torch.full((1,), float(n_averaged + 1), dtype=avg.dtype, device=avg.device))


class StochasticWeightAveraging:
    def __init__(self, swa_lrs, swa_epoch_start=0.8, annealing_epochs: int = 10, annealing_strategy: str = "cos"):
        lrs = list(swa_lrs) if isinstance(swa_lrs, (list, tuple)) else [swa_lrs]
        if len(lrs) != 1:
            raise ValueError("StochasticWeightAveraging drives one parameter group: swa_lrs is one positive float")
        if isinstance(lrs[0], bool) or not isinstance(lrs[0], (int, float)) or not lrs[0] > 0:
            raise ValueError(f"swa_lrs must be a positive float (got {swa_lrs!r})")
        if isinstance(swa_epoch_start, bool) or not isinstance(swa_epoch_start, (int, float)):
            raise ValueError(f"swa_epoch_start must be an int >= 1 or a float in [0, 1] (got {swa_epoch_start!r})")
        if isinstance(swa_epoch_start, float) and not 0.0 <= swa_epoch_start <= 1.0:
            raise ValueError(f"a float swa_epoch_start lies in [0, 1] (got {swa_epoch_start})")
        if isinstance(swa_epoch_start, int) and swa_epoch_start < 1:
            raise ValueError(f"an int swa_epoch_start is >= 1 (got {swa_epoch_start})")
        if annealing_strategy not in ("cos", "linear"):
            raise ValueError(f"annealing_strategy must be 'cos' or 'linear' (got {annealing_strategy!r})")
        if int(annealing_epochs) < 0:
            raise ValueError(f"annealing_epochs must be >= 0 (got {annealing_epochs})")
        self.swa_lr = float(lrs[0])
        self.swa_epoch_start = swa_epoch_start
        self.annealing_epochs = int(annealing_epochs)
        self.annealing_strategy = annealing_strategy
        self.n_averaged = 0
        self.swa_start = self.swa_end = None
        self._avg = None           # the averaged tensors, in list(module.parameters()) order
        self._swalr = False        # SWALR is the trainer's scheduler
        self._momenta = {}         # BatchNorm module name -> its momentum, while the re-estimate epoch runs
        self._has_bn = False
        self._transferred = False
        self._last_epoch = -1      # the last epoch that started

    # ------------------------------------------------------------------ state
    def state_dict(self):
        return {"n_averaged": self.n_averaged, "swalr": self._swalr, "transferred": self._transferred,
                "average": None if self._avg is None else [a.detach().clone() for a in self._avg],
                # a momentum of None (cumulative average) travels as -1.0
                "momenta": {k: -1.0 if v is None else float(v) for k, v in self._momenta.items()}}

    def load_state_dict(self, st):
        self.n_averaged = int(st.get("n_averaged", 0))
        self._swalr = bool(st.get("swalr", False))
        self._transferred = bool(st.get("transferred", False))
        self._avg = None if st.get("average") is None else [a.clone() for a in st["average"]]
        self._momenta = {k: None if v < 0 else v for k, v in st.get("momenta", {}).items()}

    # ------------------------------------------------------------------ hooks
    def on_fit_start(self, trainer, module):
        if trainer.optimizer is None or len(trainer.optimizer.param_groups) != 1:
            raise ValueError("StochasticWeightAveraging needs an optimizer with one parameter group")
        self.swa_start, self.swa_end = swa_window(trainer.max_epochs, self.swa_epoch_start)
        self._has_bn = any(isinstance(m, _BatchNorm) for m in module.modules())
        if self._has_bn:
            trainer.extra_epochs = 1  # the BatchNorm re-estimate epoch
        params = list(module.parameters())
        if self._avg is not None:  # resumed
            if len(self._avg) != len(params) or any(a.shape != p.shape for a, p in zip(self._avg, params)):
                raise RuntimeError("the checkpoint's averaged tensors do not match the module's parameters")
            self._avg = [a.to(device=p.device, dtype=p.dtype).contiguous() for a, p in zip(self._avg, params)]
        if self._swalr:  # resumed past swa_start: SWALR back in place before its state is loaded
            self._install_swalr(trainer)

    def _install_swalr(self, trainer):
        opt = trainer.optimizer
        opt.param_groups[0]["initial_lr"] = self.swa_lr
        trainer.scheduler = SWALR(opt, swa_lr=self.swa_lr, anneal_epochs=self.annealing_epochs,
                                  anneal_strategy=self.annealing_strategy)
        self._swalr = True

    def on_train_epoch_start(self, trainer, module):
        e = self._last_epoch = module.current_epoch
        if e == self.swa_start and not self._swalr:
            self._install_swalr(trainer)
        if self.swa_start <= e <= self.swa_end:
            self._update(trainer, module)
        if self._has_bn and e == self.swa_end + 1:
            self._transfer(trainer, module)
            for name, m in module.named_modules():
                if isinstance(m, _BatchNorm) and m.running_mean is not None:
                    m.running_mean.zero_()
                    m.running_var.fill_(1.0)
                    m.num_batches_tracked.zero_()
                    self._momenta[name] = m.momentum
                    m.momentum = None
            trainer.forward_only = True

    def on_epoch_end(self, trainer, module, metrics):
        if self._momenta and module.current_epoch == self.swa_end + 1:
            mods = dict(module.named_modules())
            for name, mom in self._momenta.items():
                mods[name].momentum = mom
            self._momenta = {}

    def on_train_end(self, trainer, module):
        if self.swa_start is None or self._transferred:
            return
        if not self._has_bn and self._last_epoch == self.swa_end and self.n_averaged > 0:
            self._transfer(trainer, module)
            return
        if trainer.is_global_zero:
            print(f"[swa] training ended after epoch {self._last_epoch}, before the averaging window closed "
                  f"(swa_end {self.swa_end}): the averaged weights were not transferred", flush=True)

    # ------------------------------------------------------------------ the two passes
    def _whole_rows(self, trainer):
        # data parallel: rows of a sharded FC1 that other ranks own come back first (a collective; the trainer's
        # epoch-end sync_sharded() has normally done it already)
        if trainer.ddp is not None:
            trainer.ddp.sync_sharded()

    @torch.no_grad()
    def _update(self, trainer, module):
        self._whole_rows(trainer)
        params = list(module.parameters())  # the parameters themselves: K.wait_param reads their pending events
        if self._avg is None:
            self._avg = [torch.empty(p.shape, dtype=p.dtype, device=p.device) for p in params]
        if params[0].is_cuda:
            from ..miaudio import kernels as K
            K.swa_update(self._avg, params, self.n_averaged)
        else:
            for a, p in zip(self._avg, params):
                average_(a, p, self.n_averaged)
        self.n_averaged += 1

    @torch.no_grad()
    def _transfer(self, trainer, module):
        self._whole_rows(trainer)
        params = list(module.parameters())
        if params[0].is_cuda:
            from ..miaudio import kernels as K
            K.swa_transfer(params, self._avg)  # reads p._mia_bf16 / _version off the parameters themselves
        else:
            for p, a in zip(params, self._avg):
                p.copy_(a)
        self._transferred = True
