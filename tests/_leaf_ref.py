"""Float64 restatement of the LEAF frontend formulas (Gabor energy, average pool, PCEN), the checker of
tests/test_leaf_cpu.py and tests/test_gpu_leaf.py.  Written from the formulas, torch elementwise ops,
matmul and FFT only.

``bf16=True`` emulates the kernels' BF16 compute mode: x, w and the backward's scaled tile are rounded to
bf16 before the float64 sums.
"""
from __future__ import annotations

import math

import torch

EPS = 1e-6


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def init_params(F: int, sr: int = 44100):
    cf = torch.linspace(60.0, 7800.0, F) / (sr / 2)
    return {"center_freqs": cf, "bandwidths": torch.full((F,), 1.0), "alpha": torch.full((F,), 0.98),
            "delta": torch.full((F,), 2.0), "r": torch.full((F,), 0.5)}


def spread_params(F: int, sr: int = 44100):
    p = init_params(F, sr)
    p["bandwidths"] = torch.linspace(0.002, 1.0, F)
    p["center_freqs"] = p["center_freqs"] * 300
    p["r"] = torch.linspace(0.3, 0.7, F)
    p["delta"] = torch.linspace(1.0, 3.0, F)
    return p


def filters(cf: torch.Tensor, bw: torch.Tensor, Kt: int, sr: int = 44100) -> torch.Tensor:
    """w [2][F][Kt] (re, im) in the dtype of cf; differentiable in cf and bw."""
    h = Kt // 2
    dt = cf.dtype
    # the tap times are float32 values (integer / sample rate in torch's default dtype), whatever dt is
    t = ((torch.arange(Kt, device=cf.device) - h).to(torch.float32) / sr).to(dt)
    window = torch.hann_window(Kt, periodic=True, dtype=torch.float32).to(dt).to(cf.device)
    env = torch.exp(-0.5 * (t[None, :] * bw[:, None] * sr) ** 2)
    ph = 2 * math.pi * cf[:, None] * t[None, :]
    return torch.stack([torch.cos(ph) * env * window, torch.sin(ph) * env * window])


def _corr_fft(a: torch.Tensor, xs_f: torch.Tensor, n: int, out_len: int) -> torch.Tensor:
    """out[r][i] = sum_j a[r][j] * xs[i + j], i < out_len (xs_f = rfft(xs, n), no wrap for i + j < n)."""
    return torch.fft.irfft(torch.conj(torch.fft.rfft(a, n)) * xs_f[None, :], n)[:, :out_len]


def conv_pair(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """z [B][2F][T]: z[b][r][t] = sum_k w[r][k] x[b][t + k - h] with zero padding (float64)."""
    B, T = x.shape
    R, Kt = w.shape[0] * w.shape[1], w.shape[2]
    h = Kt // 2
    wm = w.reshape(R, Kt)
    xs = torch.nn.functional.pad(x, (h, h))
    if T * Kt <= 4_000_000:
        win = xs.unfold(1, Kt, 1)  # [B][T][Kt]
        return torch.einsum("btk,rk->brt", win, wm)
    n = 1 << (T + 2 * h).bit_length()
    out = torch.empty(B, R, T, dtype=torch.float64)
    for b in range(B):
        xf = torch.fft.rfft(xs[b], n)
        for r0 in range(0, R, 32):
            out[b, r0:r0 + 32] = _corr_fft(wm[r0:r0 + 32], xf, n, T)
    return out


def energy_pool(x, w, pool: int, bf16: bool = False) -> torch.Tensor:
    """P [B][F][Tp] float64."""
    x = torch.as_tensor(x).to(torch.float64)
    w = torch.as_tensor(w).to(torch.float64)
    if bf16:
        x, w = bf16_round(x), bf16_round(w)
    F = w.shape[1]
    B, T = x.shape
    Tp = T // pool
    z = conv_pair(x, w)
    e = z[:, :F] ** 2 + z[:, F:] ** 2
    return e[:, :, :Tp * pool].reshape(B, F, Tp, pool).mean(-1)


def energy_bwd(x, w, gP, pool: int, bf16: bool = False) -> torch.Tensor:
    """dw [2][F][Kt] float64 of sum(P * gP)."""
    x = torch.as_tensor(x).to(torch.float64)
    w = torch.as_tensor(w).to(torch.float64)
    gP = torch.as_tensor(gP).to(torch.float64)
    if bf16:
        x, w = bf16_round(x), bf16_round(w)
    _, F, Kt = w.shape
    h = Kt // 2
    B, T = x.shape
    Tp = T // pool
    z = conv_pair(x, w)
    g = torch.zeros(B, F, T, dtype=torch.float64)
    g[:, :, :Tp * pool] = gP.repeat_interleave(pool, dim=2) * (2.0 / pool)
    s = z * torch.cat([g, g], 1)
    if bf16:
        s = bf16_round(s)
    xs = torch.nn.functional.pad(x, (h, h))
    if T * Kt <= 4_000_000:
        win = xs.unfold(1, Kt, 1)
        return torch.einsum("brt,btk->rk", s, win).reshape(2, F, Kt)
    n = 1 << (T + 2 * h).bit_length()
    dw = torch.zeros(2 * F, Kt, dtype=torch.float64)
    for b in range(B):
        xf = torch.fft.rfft(xs[b], n)
        for r0 in range(0, 2 * F, 32):
            dw[r0:r0 + 32] += _corr_fft(s[b, r0:r0 + 32], xf, n, Kt)
    return dw.reshape(2, F, Kt)


def smooth5(P: torch.Tensor) -> torch.Tensor:
    Pp = torch.nn.functional.pad(P, (2, 2))
    Tp = P.shape[-1]
    return sum(Pp[..., i:i + Tp] for i in range(5)) / 5.0


def pcen(P, r, delta, eps: float = EPS) -> torch.Tensor:
    M = smooth5(P)
    return torch.log(P / (eps + M) ** r.view(1, -1, 1) + delta.view(1, -1, 1))


def pcen_bwd(P, r, delta, gy, eps: float = EPS):
    """(gP, dr, ddelta) float64 by autograd over the formula."""
    P = torch.as_tensor(P).to(torch.float64).clone().requires_grad_(True)
    r = torch.as_tensor(r).to(torch.float64).clone().requires_grad_(True)
    delta = torch.as_tensor(delta).to(torch.float64).clone().requires_grad_(True)
    y = pcen(P, r, delta, eps)
    y.backward(torch.as_tensor(gy).to(torch.float64))
    return P.grad, r.grad, delta.grad


def frontend(x, params, Kt: int, pool: int, sr: int = 44100, bf16: bool = False):
    """(P, y) float64 from the parameter dict (init_params / spread_params layout)."""
    w = filters(params["center_freqs"].double(), params["bandwidths"].double(), Kt, sr)
    P = energy_pool(x, w, pool, bf16)
    return P, pcen(P, params["r"].double(), params["delta"].double())
