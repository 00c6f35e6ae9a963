#!/usr/bin/env python
"""Generate tests/golden/golden_leaf.npz by running the REFERENCE's LEAF modules in float64.

Run where the reference checkout is present (REFERENCE_DIR, as make_golden.py):
    python tests/golden/make_golden_leaf.py

What runs from the reference (imported as-is, never copied): src/models/leaf.py::GaborConv1d and PCEN,
with avg_pool1d(160) between them as LeafModel.forward orders them, all under .double().
Inputs and the upstream gradient come from oracle/synth.py::synth_waveform so the tests regenerate them
bit-identically; the seeds are recorded in the file.  Only numbers are stored.

Keys: "<case>_<set>__<name>", case A / B / C (tests/test_gpu_leaf.py CASES), set init / spread.
  A, B: P, y, gP [B][F][Tp] and g_center_freqs, g_bandwidths, g_r, g_delta [F]
  C:    idx (sampled flat indices), P_s, y_s, gP_s (values there), P_rowmean, y_rowmean, gP_rowmean [B][F],
        and the four parameter gradients
  "<case>__dims" = (F, Kt, T, B, pool), "<case>__seeds" = (seed_x, seed_gy)
  "state186__<key>": the initial state_dict of the reference's gabor / pcen modules at the default F = 186
"""
from __future__ import annotations

import importlib.util
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
REF = Path(os.environ.get("REFERENCE_DIR", "/root/reference"))
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

from oracle.synth import hash_uniform, synth_waveform  # noqa: E402

POOL = 160
CASES = {  # name: (F, Kt, T, B, seed_x, seed_gy)
    "A": (186, 401, 160 * 7 + 37, 3, 7101, 7102),
    "B": (5, 33, 160 * 3 + 1, 2, 7201, 7202),
    "C": (128, 401, 220_500, 2, 7301, 7302),
}
N_SAMPLED = 2048
SAMPLE_SEED = 7555


def ref_leaf():
    spec = importlib.util.spec_from_file_location("_ref_leaf", REF / "src" / "models" / "leaf.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def spread_(gabor, pcen, F):
    with torch.no_grad():
        gabor.bandwidths.copy_(torch.linspace(0.002, 1.0, F))
        gabor.center_freqs.mul_(300)
        pcen.r.copy_(torch.linspace(0.3, 0.7, F))
        pcen.delta.copy_(torch.linspace(1.0, 3.0, F))


def run_case(mod, name, pset, out):
    F, Kt, T, B, sx, sg = CASES[name]
    Tp = T // POOL
    gabor = mod.GaborConv1d(n_filters=F, kernel_size=Kt, sample_rate=44100)
    pcen = mod.PCEN(F)
    if pset == "spread":
        spread_(gabor, pcen, F)
    gabor, pcen = gabor.double(), pcen.double()
    x = torch.from_numpy(synth_waveform(sx, B, T)).double()[:, None, :]
    gy = torch.from_numpy(synth_waveform(sg, B, F * Tp).reshape(B, F, Tp)).double()
    e = gabor(x)
    P = torch.nn.functional.avg_pool1d(e, POOL)
    P.retain_grad()
    y = pcen(P)
    y.backward(gy)
    assert pcen.alpha.grad is None
    pre = f"{name}_{pset}__"
    grads = {"g_center_freqs": gabor.center_freqs.grad, "g_bandwidths": gabor.bandwidths.grad,
             "g_r": pcen.r.grad, "g_delta": pcen.delta.grad}
    for k, v in grads.items():
        out[pre + k] = v.numpy().copy()
    full = {"P": P.detach(), "y": y.detach(), "gP": P.grad}
    if name == "C":
        n = B * F * Tp
        idx = (hash_uniform(SAMPLE_SEED, (N_SAMPLED,), 0.0, 1.0).astype(np.float64) * n).astype(np.int64).clip(0, n - 1)
        out[pre + "idx"] = idx
        for k, v in full.items():
            out[pre + k + "_s"] = v.numpy().ravel()[idx].copy()
            out[pre + k + "_rowmean"] = v.mean(-1).numpy().copy()
    else:
        for k, v in full.items():
            out[pre + k] = v.numpy().copy()
    out[f"{name}__dims"] = np.array([F, Kt, T, B, POOL], dtype=np.int64)
    out[f"{name}__seeds"] = np.array([sx, sg], dtype=np.int64)


def main():
    torch.set_num_threads(os.cpu_count() or 8)
    mod = ref_leaf()
    out = {}
    m = mod.LeafModel()
    for k, v in m.state_dict().items():
        if k.startswith("gabor.") or k.startswith("pcen."):
            out["state186__" + k] = v.numpy().copy()
    for name in CASES:
        for pset in ("init", "spread"):
            t0 = time.time()
            run_case(mod, name, pset, out)
            print(f"case {name} {pset}: {time.time() - t0:.1f} s", flush=True)
    path = HERE / "golden_leaf.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
