#!/usr/bin/env python
"""Generate tests/golden/golden_leaf_model.npz by running the REFERENCE's LeafModel in float64.

Run where the reference checkout is present (REFERENCE_DIR, as make_golden_leaf.py):
    python tests/golden/make_golden_leaf_model.py

What runs from the reference (imported as-is, never copied): src/models/leaf.py::LeafModel, under .double(), in
train mode with p = 0 set on the instance's Dropout modules (BatchNorm on batch statistics, no mask), one forward
and backward of the engine's soft-label cross-entropy on one-hot labels; then the same input in eval mode (the
running statistics the train-mode forward just updated; no parameter update in between).

Parameters: gabor.* and pcen.* as the reference constructs them (stored); the conv / linear / BatchNorm parameters
are overwritten with tests/_leaf_model_ref.py::hash_init(seed) -- the 1.6 M default-initialised trunk weights would
not fit the fixture, the hash is regenerated bit-identically by the tests -- and the seed is recorded.  Inputs come
from case_waveform (below), labels from hash_uniform; seeds recorded.  Only numbers are stored.

Cases: T = 160 * 94 + 37 (Tp = 94 -> 23 -> 5 -> 2 frames: every pool drops a remainder, two frames reach the mean);
M1 = F 24, Kt 33, 10 classes; M2 = the default F 186 (Fp = 192) with Kt 401, 50 classes; both at B = 8.  The clips are
tests/_leaf_model_ref.py::case_waveform (noise under a gain that changes every pooled frame, per-clip levels,
amplitude up to 100), not oracle.synth.synth_waveform: on peak-normalised white noise PCEN's output is a constant
plus a ripple of three bf16 steps, and every later BatchNorm divides by that ripple (the docstring there has the
figures).  With these clips the float32 evaluation of the restatement is within 1.3e-5 of every stored value and its
bf16-rounding evaluation within 4e-2 of the logits.
The seeds were chosen among candidates by two properties of the float64 forward alone, because a max-pool window or
a ReLU argument that float32 rounding can tip decides where a gradient entry goes (one re-routed entry moved a conv
weight gradient by 1e-2 in an earlier fixture): no pool window of any block whose two largest values are closer than
1.5e-6 of the layer's largest |z| (M1 / M2: 2.6e-6 at the closest), and no pooled or classifier BatchNorm output
closer to the ReLU threshold than 5e-7 of the layer's largest.

Keys, per case M1 / M2 ("<case>__<name>"):
  dims = (F, Kt, T, B, classes, pool), seeds = (seed_x, seed_labels, seed_init), labels [B]
  state__gabor.* / state__pcen.*: the initial values of those modules
  logits, loss, eval_logits
  g__<param>: the full gradient of every small parameter (Gabor, PCEN, BatchNorm, classifier.12.weight and .bias)
  gs__<param> / gsum__<param>: for the six large weights, N_SAMPLED sampled entries (flat indices
      sample_indices(j, numel), j = the parameter's position in named_parameters()) and, for the three conv
      weights, the per-output-channel sums
  (the gradients of the six biases in front of a BatchNorm are exactly 0 up to float64 rounding noise, asserted
  here to be below 1e-12 and not stored, to keep the file within the size of golden.npz)
  run__<buffer>: the BatchNorm running_mean / running_var / num_batches_tracked after the step
"default__keys" / "default__shapes": state_dict keys and shapes (padded with -1) of the default LeafModel().
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

from oracle.synth import hash_uniform  # noqa: E402
from tests._leaf_model_ref import case_waveform, hash_init  # noqa: E402

POOL = 160
T_CLIP = 160 * 94 + 37  # Tp = 94 -> 23 -> 5 -> 2: every pool has a remainder, two frames reach the mean
CASES = {  # name: (F, Kt, T, B, classes, seed_x, seed_labels, seed_init)
    "M1": (24, 33, T_CLIP, 8, 10, 30001, 30002, 30003),
    "M2": (186, 401, T_CLIP, 8, 50, 20001, 20002, 20003),
}
LARGE = ("conv_block.0.weight", "conv_block.4.weight", "conv_block.8.weight", "classifier.0.weight",
         "classifier.4.weight", "classifier.8.weight")
BN_FED = ("conv_block.0.bias", "conv_block.4.bias", "conv_block.8.bias", "classifier.0.bias", "classifier.4.bias",
          "classifier.8.bias")  # biases in front of a BatchNorm
N_SAMPLED = 96
SAMPLE_SEED = 8555


def sample_indices(j: int, n: int) -> np.ndarray:
    idx = (hash_uniform(SAMPLE_SEED + j, (N_SAMPLED,), 0.0, 1.0).astype(np.float64) * n).astype(np.int64)
    return idx.clip(0, n - 1)


def ref_leaf():
    spec = importlib.util.spec_from_file_location("_ref_leaf", REF / "src" / "models" / "leaf.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_case(mod, name, out):
    F, Kt, T, B, C, sx, sl, si = CASES[name]
    m = mod.LeafModel(n_filters=F, kernel_size=Kt, sample_rate=44100, num_classes=C)
    pre = f"{name}__"
    for k, v in m.state_dict().items():
        if k.startswith("gabor.") or k.startswith("pcen."):
            out[pre + "state__" + k] = v.numpy().copy()
    init = hash_init([(k, tuple(v.shape)) for k, v in m.state_dict().items()], si)
    missing, unexpected = m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()}, strict=False)
    assert not unexpected and all(k.startswith(("gabor.", "pcen.")) or "running_" in k or "num_batches" in k
                                  for k in missing), missing
    for mm in m.modules():
        if isinstance(mm, torch.nn.Dropout):
            mm.p = 0.0
    m = m.double().train()
    x = torch.from_numpy(case_waveform(sx, B, T)).double()[:, None, :]
    labels = (hash_uniform(sl, (B,), 0.0, 1.0).astype(np.float64) * C).astype(np.int64).clip(0, C - 1)
    y = torch.zeros(B, C, dtype=torch.float64)
    y[torch.arange(B), torch.from_numpy(labels)] = 1.0
    logits = m(x)
    loss = -torch.sum(y * torch.log(torch.softmax(logits, dim=1) + 1e-8), dim=1).mean()  # engine.py soft-label CE
    loss.backward()
    out[pre + "dims"] = np.array([F, Kt, T, B, C, POOL], dtype=np.int64)
    out[pre + "seeds"] = np.array([sx, sl, si], dtype=np.int64)
    out[pre + "labels"] = labels
    out[pre + "logits"] = logits.detach().numpy().copy()
    out[pre + "loss"] = np.array(float(loss.detach()))
    for j, (k, p) in enumerate(m.named_parameters()):
        if p.grad is None:
            assert k == "pcen.alpha", k
            continue
        g = p.grad.numpy()
        if k in LARGE:
            n = g.size
            idx = sample_indices(j, n)
            out[pre + "gs__" + k] = g.ravel()[idx].copy()
            if g.ndim == 3:
                out[pre + "gsum__" + k] = g.reshape(g.shape[0], -1).sum(1)
        elif k in BN_FED:
            # true value exactly 0 (the BatchNorm removes the bias): what the reference holds is float64 rounding
            # noise; not stored, the tests bound these gradients absolutely
            assert np.abs(g).max() < 1e-12, (k, np.abs(g).max())
        else:
            out[pre + "g__" + k] = g.copy()
    for k, v in m.state_dict().items():
        if "running_" in k or "num_batches" in k:
            out[pre + "run__" + k] = v.numpy().copy()
    m.eval()
    with torch.no_grad():
        out[pre + "eval_logits"] = m(x).numpy().copy()


def main():
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    mod = ref_leaf()
    out = {}
    sd = mod.LeafModel().state_dict()
    out["default__keys"] = np.array(list(sd.keys()))
    out["default__shapes"] = np.array([list(v.shape) + [-1] * (3 - v.ndim) for v in sd.values()], dtype=np.int64)
    for name in CASES:
        t0 = time.time()
        run_case(mod, name, out)
        print(f"case {name}: {time.time() - t0:.1f} s", flush=True)
    path = HERE / "golden_leaf_model.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
