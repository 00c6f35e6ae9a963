"""Float64 restatement of torchaudio 2.7.1 ``transforms.Resample`` (Hann-windowed sinc, lowpass_filter_width 6,
rolloff 0.99) for the resampling tests: its own tap construction and a direct-sum apply of the formula in
include/miaudio_resample.h.  numpy only; shares no code with the package.

torchaudio cannot be imported where this project runs, so parity at that boundary is restated from its documented
semantics (``_get_sinc_resample_kernel`` with ``dtype=None`` and ``_apply_sinc_resample_kernel``), not pinned.
"""
from __future__ import annotations

import math

import numpy as np

PAIRS = [(44100, 16000), (16000, 44100), (44100, 22050), (22050, 44100), (44100, 48000), (8000, 44100)]
U = 2.0 ** -24  # unit roundoff of f32


def geometry(orig: int, new: int, lpw: int = 6, rolloff: float = 0.99):
    """(o, n, width, K)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    return o, n, width, 2 * width + o


def taps64(orig: int, new: int, lpw: int = 6, rolloff: float = 0.99) -> np.ndarray:
    """[n][K] float64: the values torchaudio holds before it rounds the kernel to f32."""
    o, n, width, K = geometry(orig, new, lpw, rolloff)
    base = min(o, n) * rolloff
    idx = np.arange(-width, width + o, dtype=np.float64) / o
    # torch: an int64 tensor divided by a python int is float32; the float64 idx then promotes the sum
    phase = (np.arange(0, -n, -1).astype(np.float32) / np.float32(n)).astype(np.float64)
    t = phase[:, None] + idx[None, :]
    t = t * base
    t = np.clip(t, -lpw, lpw)
    window = np.cos(t * math.pi / lpw / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(t == 0, 1.0, np.sin(t) / t)
    k = k * (window * (base / o))
    assert k.shape == (n, K)
    return k


def taps32(orig: int, new: int) -> np.ndarray:
    return taps64(orig, new).astype(np.float32)


def out_len(T: int, o: int, n: int) -> int:
    return -(-n * T // o)


def apply(x: np.ndarray, taps: np.ndarray, o: int, n: int, width: int, lengths=None):
    """x (B, T), taps (n, K) -> (out float64 (B, Tout), mag float64 (B, Tout)) with
    out[b, f*n + j] = sum_k xz_b[f*o + k - width] * taps[j, k] for f*n + j < ceil(n * L_b / o), 0 behind it, and
    mag the same sum over |xz| * |taps| (the scale of the f32 dot-product error bound)."""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    B, T = x.shape
    K = taps.shape[1]
    assert taps.shape[0] == n and K == 2 * width + o
    Tout = out_len(T, o, n)
    frames = -(-Tout // n) if Tout else 0
    out = np.zeros((B, Tout))
    mag = np.zeros((B, Tout))
    for b in range(B):
        L = T if lengths is None else min(max(int(lengths[b]), 0), T)
        xz = np.zeros(width + frames * o + K)
        xz[width:width + L] = x[b, :L]
        win = np.lib.stride_tricks.sliding_window_view(xz, K)[::o][:frames]  # [f][k] = xz[f*o + k] (shifted by width)
        full = (win @ taps.T).reshape(-1)[:Tout]
        fmag = (np.abs(win) @ np.abs(taps).T).reshape(-1)[:Tout]
        ol = out_len(L, o, n)
        out[b, :ol], mag[b, :ol] = full[:ol], fmag[:ol]
    return out, mag


def apply_exact(x: np.ndarray, taps: np.ndarray, o: int, n: int, width: int, lengths=None) -> np.ndarray:
    """The same direct sum on integer operands in int64 (no rounding anywhere)."""
    x = np.asarray(x, dtype=np.int64)
    taps = np.asarray(taps, dtype=np.int64)
    B, T = x.shape
    K = taps.shape[1]
    Tout = out_len(T, o, n)
    frames = -(-Tout // n) if Tout else 0
    out = np.zeros((B, Tout), dtype=np.int64)
    for b in range(B):
        L = T if lengths is None else min(max(int(lengths[b]), 0), T)
        xz = np.zeros(width + frames * o + K, dtype=np.int64)
        xz[width:width + L] = x[b, :L]
        win = np.lib.stride_tricks.sliding_window_view(xz, K)[::o][:frames]
        ol = out_len(L, o, n)
        out[b, :ol] = (win @ taps.T).reshape(-1)[:Tout][:ol]
    return out


def bound(K: int, mag: np.ndarray) -> np.ndarray:
    """|fl(sum) - sum| <= gamma_K * sum |x||t| for an f32 dot product of K terms in any order, with or without FMA
    (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1), plus half the smallest subnormal."""
    gamma = K * U / (1.0 - K * U)
    return gamma * mag + 2.0 ** -149
