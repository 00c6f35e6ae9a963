"""Clip-length fitting restated in numpy from its description (the reference's
src/utils/audio.py::pad_or_trim plus the zero mode and the empty clip): the expected value of fit_clip and
mia_fit_gather.  Works on any 1-D array; pass a uint32 / int32 view to compare bits."""
import numpy as np

MODES = ("wrap", "zero")


def fit_ref(clip: np.ndarray, length: int, mode: str = "wrap") -> np.ndarray:
    assert mode in MODES and length >= 1 and clip.ndim == 1
    n = clip.shape[0]
    if n == length:
        return clip.copy()
    if n > length:
        start = (n - length) // 2
        return clip[start:start + length].copy()
    if n == 0:
        return np.zeros(length, dtype=clip.dtype)
    if mode == "wrap":
        return clip[np.arange(length) % n]
    out = np.zeros(length, dtype=clip.dtype)
    out[:n] = clip
    return out
