"""LEAF frontend on the MI355X: learnable Gabor filterbank -> squared modulus -> average pool -> PCEN.

The frontend of the reference's ``LeafModel`` (its ``gabor``, ``downsample`` and ``pcen`` members, in the
order its forward applies them).  ``LeafFrontend`` keeps the reference's parameter names and shapes for
those modules, so their part of a reference checkpoint loads as is:

    gabor.center_freqs [F]   gabor.bandwidths [F]   gabor.window [1, Kt] (buffer)
    pcen.alpha [F] (unused, no gradient)   pcen.delta [F]   pcen.r [F]

The filter taps are synthesised by torch elementwise ops on [F, Kt] tensors (autograd carries the bank
gradient back to ``center_freqs`` / ``bandwidths``); energy + pooling and PCEN are two autograd Functions
over the HIP kernels (``mia_leaf_energy_*``, ``mia_pcen_*``): no [B, F, T] tensor is ever written.
A CPU tensor takes the same math on torch ops (plumbing runs without a GPU).  The trunk and classifier
of ``LeafModel`` are not part of this module.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F_

from ..miaudio import kernels as K
from ..miaudio import lib as L


class GaborFilters(nn.Module):
    """Parameters of the Gabor bank and its tap synthesis: ``filters()`` -> w [2][F][Kt] (re, im)."""

    def __init__(self, n_filters=186, kernel_size=401, sample_rate=44100, min_freq=60.0, max_freq=7800.0):
        super().__init__()
        self.n_filters, self.kernel_size, self.sample_rate = int(n_filters), int(kernel_size), int(sample_rate)
        self.center_freqs = nn.Parameter(torch.linspace(min_freq, max_freq, n_filters) / (sample_rate / 2))
        self.bandwidths = nn.Parameter(torch.full((n_filters,), 1.0))
        self.register_buffer("window", torch.hann_window(kernel_size).unsqueeze(0))

    def filters(self) -> torch.Tensor:
        h = self.kernel_size // 2
        dev = self.center_freqs.device
        t = (torch.arange(self.kernel_size, device=dev) - h).to(torch.float32) / self.sample_rate
        t = t.view(1, -1)
        cf = self.center_freqs.view(-1, 1)
        bw = self.bandwidths.view(-1, 1)
        env = torch.exp(-0.5 * (t * bw * self.sample_rate) ** 2) * self.window
        # cf is Hz / (sr / 2) and multiplies t in seconds with no further sample-rate factor, as the reference
        ph = 2 * math.pi * cf * t
        return torch.stack([torch.cos(ph) * env, torch.sin(ph) * env])


class PCENParams(nn.Module):
    def __init__(self, num_channels, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, s=0.04):
        super().__init__()
        self.eps = eps
        self.alpha = nn.Parameter(torch.full((num_channels,), alpha))  # present in the reference, takes no part
        self.delta = nn.Parameter(torch.full((num_channels,), delta))
        self.r = nn.Parameter(torch.full((num_channels,), r))
        self.s = s


class _LeafEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, pool, compute):
        ctx.save_for_backward(x, w)
        ctx.pool, ctx.compute = pool, compute
        return K.leaf_energy_fwd(x, w, pool, compute, tag="leaf.energy.fwd")

    @staticmethod
    def backward(ctx, gP):
        x, w = ctx.saved_tensors
        dw = None
        if ctx.needs_input_grad[1]:
            dw = K.leaf_energy_bwd(x, w, gP.contiguous().float(), ctx.pool, ctx.compute, tag="leaf.energy.bwd")
        return None, dw, None, None


class _PCEN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, r, delta, eps):
        ctx.save_for_backward(P, r, delta)
        ctx.eps = eps
        return K.pcen_fwd(P, r, delta, eps, tag="leaf.pcen.fwd")

    @staticmethod
    def backward(ctx, gy):
        P, r, delta = ctx.saved_tensors
        gP, dr, dd = K.pcen_bwd(P, r, delta, ctx.eps, gy.contiguous().float(), tag="leaf.pcen.bwd")
        return gP, dr, dd, None


class LeafFrontend(nn.Module):
    """(B, 1, T) or (B, T) f32 waveform -> (B, F, T // pool) PCEN-compressed Gabor energies."""

    def __init__(self, n_filters: int = 186, kernel_size: int = 401, sample_rate: int = 44100, pool: int = 160,
                 compute_dtype: str | None = "bf16"):
        super().__init__()
        K.leaf_check_args(1, pool, n_filters, kernel_size, pool)
        self.pool = int(pool)
        self.compute_dtype = compute_dtype
        self.gabor = GaborFilters(n_filters, kernel_size, sample_rate)
        self.pcen = PCENParams(n_filters)

    def _compute_code(self) -> int:
        cd = self.compute_dtype
        if cd is None:
            if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
                return L.BF16
            return L.F32
        return {"bf16": L.BF16, "bfloat16": L.BF16, "f32": L.F32, "fp32": L.F32, "32": L.F32, "fp8": L.BF16}[str(cd)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 3 and x.shape[1] == 1:
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ValueError(f"LeafFrontend expects (B,1,T) or (B,T), got {tuple(x.shape)}")
        if x.requires_grad:
            raise RuntimeError("LeafFrontend: the waveform must not require grad (the kernels produce no dx)")
        K.leaf_check_args(x.shape[0], x.shape[1], self.gabor.n_filters, self.gabor.kernel_size, self.pool)
        if not x.is_cuda:
            return self._cpu_forward(x)
        with torch.autocast("cuda", enabled=False):
            w = self.gabor.filters()
            P = _LeafEnergy.apply(x.float().contiguous(), w, self.pool, self._compute_code())
            return _PCEN.apply(P, self.pcen.r, self.pcen.delta, self.pcen.eps)

    def _cpu_forward(self, x: torch.Tensor) -> torch.Tensor:
        """accelerator=cpu plumbing: the same formulas on torch's CPU ops, in the input's dtype."""
        w = self.gabor.filters().to(x.dtype)
        h = self.gabor.kernel_size // 2
        z = F_.conv1d(x[:, None, :], w.reshape(-1, 1, w.shape[-1]), padding=h)
        nf = self.gabor.n_filters
        P = F_.avg_pool1d(z[:, :nf] ** 2 + z[:, nf:] ** 2, self.pool)
        M = F_.avg_pool1d(P, 5, stride=1, padding=2)  # count_include_pad: the divisor stays 5 at the edges
        r, d = self.pcen.r.to(x.dtype).view(1, -1, 1), self.pcen.delta.to(x.dtype).view(1, -1, 1)
        return torch.log(P / (self.pcen.eps + M) ** r + d)
