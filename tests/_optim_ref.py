"""Torch-tensor restatements of the update formulas of include/miaudio_optim.h (sgd_kernel, the AdamW kernel and
their clip coefficient), for tests.  Shares no code with the package: plain f32 tensor arithmetic, one rounding per
operation where the kernels fuse a multiply-add (the difference is within the tests' 1e-5 tolerance)."""
import math

import numpy as np
import torch


def clip_coef(grads, clip):
    """(total norm, coefficient) as norm_final_kernel forms them: f64 sum of squares, f32 norm, clip / (norm + 1e-6)
    capped at 1; clip <= 0 disables clipping."""
    tot = math.sqrt(sum(float(g.double().square().sum()) for g in grads))
    totf = np.float32(tot)
    coef = np.float32(1.0)
    if clip > 0:
        coef = min(np.float32(clip) / (totf + np.float32(1e-6)), np.float32(1.0))
    return float(totf), float(coef)


def sgd_step(p, g, buf, *, coef, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False):
    """One tensor, in place on ``p``; returns the momentum buffer (``buf`` is None at the tensor's first use)."""
    g = weight_decay * p + g * coef
    if momentum != 0:
        buf = g.clone() if buf is None else momentum * buf + (1 - dampening) * g
        g = g + momentum * buf if nesterov else buf
    p.sub_(lr * g)
    return buf


def adamw_step(p, g, m, v, step, *, coef, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
    """One tensor, in place on ``p``, ``m`` and ``v``; ``step`` is the tensor's own 1-based count."""
    lr32, b1, b2 = (float(np.float32(x)) for x in (lr, betas[0], betas[1]))
    lr_over_bc1 = float(np.float32(lr32 / (1.0 - b1 ** step)))
    bc2_sqrt = float(np.float32(math.sqrt(1.0 - b2 ** step)))
    decay = float(np.float32(1.0 - lr32 * float(np.float32(weight_decay))))
    g = g * coef
    p.mul_(decay)
    m.add_((1 - betas[0]) * (g - m))
    v.mul_(betas[1]).add_((1 - betas[1]) * g * g)
    p.sub_(lr_over_bc1 * (m / (v.sqrt() / bc2_sqrt + eps)))
