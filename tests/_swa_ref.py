"""Helpers of the stochastic-weight-averaging tests: the averaging expression and the whole schedule restated on
plain torch (torch.optim.swa_utils.SWALR + a Python loop), a data module with a fixed batch order, and the small
recording callbacks the tests hang on the Trainer."""
import torch
import torch.nn as nn
from torch.optim.swa_utils import SWALR

_BN = nn.modules.batchnorm._BatchNorm


def average_expr(avg: torch.Tensor, p: torch.Tensor, n_averaged: int) -> torch.Tensor:
    """avg + (p - avg) / (n + 1) in f32 on the CPU: one subtract, one true divide (by a tensor, so that no scalar
    reciprocal can be folded in), one add.  n == 0: the parameter itself."""
    avg, p = avg.detach().cpu().float(), p.detach().cpu().float()
    if n_averaged == 0:
        return p.clone()
    return avg + (p - avg) / torch.full_like(avg, float(n_averaged + 1))


def sequential_average(snapshots):
    """The running average of a list of snapshots (each a list of tensors), formed one snapshot at a time."""
    avg = None
    for n, snap in enumerate(snapshots):
        avg = [average_expr(s if avg is None else avg[i], s, n) for i, s in enumerate(snap)]
    return avg


class FixedDM:
    """A data module whose loaders are lists of fixed batches: the same order in every epoch and every run."""

    def __init__(self, n_batches=4, batch=8, in_samples=16, num_classes=5, seed=0):
        g = torch.Generator().manual_seed(seed)
        self.train = [(torch.randn(batch, in_samples, generator=g), torch.randint(0, num_classes, (batch,), generator=g))
                      for _ in range(n_batches)]
        self.val = [(torch.randn(batch, in_samples, generator=g), torch.randint(0, num_classes, (batch,), generator=g))]

    def setup(self, stage=None):
        pass

    def train_dataloader(self):
        return self.train

    def val_dataloader(self):
        return self.val


class Recorder:
    """Epochs run, the LR the trainer reports after each, optimizer step counts and (optionally) the parameters at
    the start of each epoch and at the end of training."""

    def __init__(self, snapshots=False):
        self.epochs, self.lrs, self.steps, self.snaps, self.final = [], [], [], [], None
        self.snapshots = snapshots

    def on_train_epoch_start(self, trainer, module):
        if self.snapshots:
            self.snaps.append([p.detach().cpu().clone() for p in module.parameters()])

    def on_epoch_end(self, trainer, module, metrics):
        self.epochs.append(metrics["epoch"])
        self.lrs.append(metrics["lr"])
        self.steps.append(module.global_step)

    def on_train_end(self, trainer, module):
        self.final = [p.detach().cpu().clone() for p in module.parameters()]


class StopAfter:
    def __init__(self, epoch):
        self.epoch, self.params = epoch, None

    def on_epoch_end(self, trainer, module, metrics):
        if metrics["epoch"] == self.epoch:
            trainer.should_stop = True
            self.params = [p.detach().cpu().clone() for p in module.parameters()]


class SaveAt:
    def __init__(self, epoch, path):
        self.epoch, self.path = epoch, str(path)

    def on_epoch_end(self, trainer, module, metrics):
        if metrics["epoch"] == self.epoch and trainer.is_global_zero:
            trainer.save_checkpoint(self.path)


def restate_fit(lit, dm, max_epochs, swa_lr, swa_epoch_start, annealing_epochs, strategy="cos"):
    """The SWA schedule on plain torch: (final parameters, per-epoch LR list, number of epochs run).  ``lit`` is
    a LitClassifier on the CPU (its training_step is the loss); the optimizer and scheduler are its own."""
    cfg = lit.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    s = int(max_epochs * swa_epoch_start) if isinstance(swa_epoch_start, float) else swa_epoch_start
    swa_start, swa_end = max(s - 1, 0), max_epochs - 1
    bns = [m for m in lit.modules() if isinstance(m, _BN)]
    avg, n, lrs = None, 0, []
    params = list(lit.parameters())

    def transfer():
        with torch.no_grad():
            for p, a in zip(params, avg):
                p.copy_(a)

    total = max_epochs + (1 if bns else 0)
    for e in range(total):
        lit.train()
        if e == swa_start:
            opt.param_groups[0]["initial_lr"] = swa_lr
            sched = SWALR(opt, swa_lr=swa_lr, anneal_epochs=annealing_epochs, anneal_strategy=strategy)
        if swa_start <= e <= swa_end:
            avg = [average_expr(p if avg is None else avg[i], p, n) for i, p in enumerate(params)]
            n += 1
        if bns and e == max_epochs:
            transfer()
            momenta = [m.momentum for m in bns]
            for m in bns:
                m.reset_running_stats()
                m.momentum = None
            with torch.no_grad():
                for i, b in enumerate(dm.train):
                    lit.training_step(b, i)
            for m, mom in zip(bns, momenta):
                m.momentum = mom
        else:
            for i, b in enumerate(dm.train):
                lit.training_step(b, i).backward()
                opt.step()
                opt.zero_grad(set_to_none=True)
        lit._flush_logs()
        lit.train_acc.reset()
        sched.step()
        lrs.append(opt.param_groups[0]["lr"])
    if not bns:
        transfer()
    return [p.detach().clone() for p in params], lrs, total
