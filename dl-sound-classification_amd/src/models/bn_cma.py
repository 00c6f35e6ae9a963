"""The running-statistics update factor of a BatchNorm training forward, as torch's ``_BatchNorm.forward``
chooses it: the module's ``momentum``, or with ``momentum=None`` (cumulative moving average) ``1 / k`` for the
k-th training forward since the statistics were reset.  The factor goes to the kernels as their ``momentum``
float (mia_bn_fwd_stats / mia_bn_finalize_shifted: running = (1 - f) running + f batch), so f = 1/k makes the
running statistics the plain mean of the k batch statistics.

``num_batches_tracked`` is incremented on the device; k itself is a host-side count kept on the module, so a
step never reads the counter back.  The count is trusted while the buffer is the tensor, at the version, this
module last left it; anything else that wrote it (first use, ``load_state_dict``, ``reset_running_stats``,
``zero_()``, a move to another device) moves the version or the pointer and costs one read."""
from __future__ import annotations

import contextlib

import torch
import torch.nn as nn


def _stamp(nbt: torch.Tensor):
    return (nbt.data_ptr(), nbt._version)


def update_factor(bn: nn.modules.batchnorm._BatchNorm, training: bool, count_always: bool) -> float:
    """The factor for this forward; in a training forward also counts it in ``num_batches_tracked`` -- always with
    ``momentum=None``, and with a float momentum only where the model counts at all (``count_always``)."""
    nbt = bn.num_batches_tracked
    if bn.momentum is not None:
        if training and count_always and nbt is not None:
            nbt.add_(1)
        return float(bn.momentum)
    if not training:
        return 0.0  # evaluation reads the running statistics and updates nothing
    if nbt is None:
        raise RuntimeError("BatchNorm(momentum=None) needs track_running_stats=True (num_batches_tracked)")
    held = getattr(bn, "_mia_cma", None)
    k = held[1] if held is not None and held[0] == _stamp(nbt) else int(nbt.item())
    k += 1
    nbt.add_(1)
    bn._mia_cma = (_stamp(nbt), k)
    return 1.0 / k


@contextlib.contextmanager
def counts_kept(module: nn.Module):
    """Around a write to the counters that is known to leave their values alone (rank 0's buffers broadcast to
    ranks that counted the same forwards): the host-side counts that were trusted before it stay trusted, instead
    of one read per BatchNorm afterwards."""
    trusted = [m for m in module.modules()
               if getattr(m, "_mia_cma", None) is not None and m._mia_cma[0] == _stamp(m.num_batches_tracked)]
    yield
    for m in trusted:
        m._mia_cma = (_stamp(m.num_batches_tracked), m._mia_cma[1])
