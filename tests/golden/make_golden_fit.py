#!/usr/bin/env python
"""Generate tests/golden/golden_fit.npz by running the REFERENCE's clip-length rule.

Run where the reference checkout is present (REFERENCE_DIR, as make_golden.py):
    python tests/golden/make_golden_fit.py

What runs from the reference (imported as-is, never copied): src/utils/audio.py::pad_or_trim ("make waveform
exactly `length_samples` long (pad wrap or trim)"), through tests/golden/_stubs/torchaudio (the module imports
torchaudio; pad_or_trim itself needs only torch).  Only numbers are stored.

Cases: every (n, L) in NS x LS.  Per case two (1, n) f32 inputs: np.arange(n), and a clip drawn from
np.random.default_rng(SEED + 1000 * n + L).standard_normal.
Keys: "n<n>_L<L>__arange_out" [L], "n<n>_L<L>__rand_in" [n], "n<n>_L<L>__rand_out" [L]; "ns", "ls".
"""
from __future__ import annotations

import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path(os.environ.get("REFERENCE_DIR", "/root/reference"))
sys.path.insert(0, str(HERE / "_stubs"))
sys.path.insert(1, str(REF))
sys.dont_write_bytecode = True

NS = (1, 2, 3, 4, 5, 7, 11, 64, 129)
LS = (1, 4, 5, 64)
SEED = 2020


def main():
    from src.utils.audio import pad_or_trim
    out = {"ns": np.array(NS, dtype=np.int64), "ls": np.array(LS, dtype=np.int64)}
    for n in NS:
        for L in LS:
            pre = f"n{n}_L{L}__"
            ramp = np.arange(n, dtype=np.float32)
            rand = np.random.default_rng(SEED + 1000 * n + L).standard_normal(n).astype(np.float32)
            out[pre + "arange_out"] = pad_or_trim(torch.from_numpy(ramp)[None], L)[0].numpy().copy()
            out[pre + "rand_in"] = rand
            out[pre + "rand_out"] = pad_or_trim(torch.from_numpy(rand)[None], L)[0].numpy().copy()
            assert out[pre + "arange_out"].shape == (L,) and out[pre + "rand_out"].shape == (L,)
    path = HERE / "golden_fit.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
