#!/usr/bin/env python
"""Generate tests/golden/golden_ast_small.npz by running the REFERENCE's ASTViTSmall / ASTMiniViT in float64.

Run where the reference checkout is present (REFERENCE_DIR, as make_golden_leaf_model.py):
    python tests/golden/make_golden_ast_small.py

What runs from the reference (imported as-is, never copied): src/models/ast_small.py::ASTViTSmall and
src/models/ast_mini.py::ASTMiniViT under .double(), one forward and backward of the engine's soft-label
cross-entropy on the returned probabilities, in two modes:
  eval   -- model.eval() (identical to train mode with p = 0);
  masked -- model.train() with torch.nn.functional.dropout replaced, for that call only, by a function that applies
            the project's masks (tests/_ast_small_ref.py: attn_keep on the (B*H, N, N) probabilities, index b*H + h;
            elem_keep on the (B, N, 4D) and (B, N, D) activations) for the stored seeds.  The replacement counts its
            calls and asserts the three shapes per block, in that order.
Parameters: tests/_ast_small_ref.py::hash_init(seed) over the state dict (no zero bias, no zero cls); inputs
hash_uniform in [-1, 1); one-hot labels from hash_uniform.  Only numbers are stored.

Cases (tests/_ast_small_ref.py::CASES): S = ASTViTSmall, 133 tokens = its whole position table (3 key tiles with
a 5-key tail, 2 query blocks); M = ASTMiniViT, 61 tokens of a table of 85 (one partial tile, the table slice).

Keys: "<case>__<mode>__probs", "__loss", "__g__<param>" (every gradient of at most LARGE_NUMEL entries in full),
"__gs__<param>" / "__gsum__<param>" (larger ones: N_SAMPLED sampled entries; for matrices the sums along the longer
side), "<case>__seeds" (depth, 3); "<class>__keys" / "__shapes" (state-dict keys and shapes, padded with -1) and
"<class>__init_sums" (per tensor sum and sum of squares, float64) of the default-constructed model under
torch.manual_seed(0).
"""
from __future__ import annotations

import importlib.util
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parents[1]
REF = Path(os.environ.get("REFERENCE_DIR", "/root/reference"))
sys.path.insert(0, str(REPO))
sys.dont_write_bytecode = True

from tests import _ast_small_ref as R  # noqa: E402


def ref_module(stem: str):
    spec = importlib.util.spec_from_file_location("_ref_" + stem, REF / "src" / "models" / f"{stem}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CLASSES = {"ASTViTSmall": "ast_small", "ASTMiniViT": "ast_mini"}


def masked_dropout(name: str):
    """The replacement of F.dropout for one masked forward of case ``name``."""
    B, N, D, H, _ = R.case_geometry(name)
    seeds = R.case_seeds(name)
    calls = [0]

    def drop(x, p=0.5, training=True, inplace=False):
        i, site = divmod(calls[0], 3)
        calls[0] += 1
        assert training and abs(p - R.P_DROP) < 1e-12
        want = [(B * H, N, N), (B, N, 4 * D), (B, N, D)][site]
        assert tuple(x.shape) == want, (tuple(x.shape), want)
        if site == 0:
            m = torch.from_numpy(R.attn_keep_mask(int(seeds[i, 0]), B, H, N, p)).reshape(B * H, N, N)
            return x * (m.to(x.dtype) * R.attn_scale(p))
        m = torch.from_numpy(R.elem_keep(int(seeds[i, site]), want, p))
        return x * (m.to(x.dtype) * R.elem_scale(p))

    return drop, calls


def run_case(name: str, out: dict):
    cls, kw, _, (_, _, si, _) = R.CASES[name]
    m = getattr(ref_module(CLASSES[cls]), cls)(**kw)
    keys_shapes = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    init = R.hash_init(keys_shapes, si)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()}, strict=True)
    m = m.double()
    spec, y = R.case_inputs(name)
    x, y = torch.from_numpy(spec).double(), torch.from_numpy(y).double()
    order = [k for k, _ in m.named_parameters()]
    assert order == [k for k, _ in keys_shapes]
    out[f"{name}__seeds"] = R.case_seeds(name)
    for mode in ("eval", "masked"):
        m.zero_grad(set_to_none=True)
        if mode == "eval":
            m.eval()
            probs = m(x)
        else:
            m.train()
            drop, calls = masked_dropout(name)
            keep = torch.nn.functional.dropout
            torch.nn.functional.dropout = drop
            try:
                probs = m(x)
            finally:
                torch.nn.functional.dropout = keep
            assert calls[0] == 3 * kw["depth"], calls
        loss = R.soft_ce(probs, y)
        loss.backward()
        run = dict(probs=probs.detach(), loss=loss.detach(), grads={k: p.grad.detach() for k, p in m.named_parameters()})
        for q, v in R.quantities(run, order).items():
            out[f"{name}__{mode}__" + q.replace(":", "__", 1)] = np.asarray(v, dtype=np.float64)
        print(f"case {name} {mode}: loss {float(loss.detach()):.6f}", flush=True)


def default_meta(cls: str, out: dict):
    torch.manual_seed(0)
    m = getattr(ref_module(CLASSES[cls]), cls)()
    sd = m.state_dict()
    out[f"{cls}__keys"] = np.array(list(sd.keys()))
    out[f"{cls}__shapes"] = np.array([list(v.shape) + [-1] * (4 - v.ndim) for v in sd.values()], dtype=np.int64)
    out[f"{cls}__init_sums"] = np.array([[float(v.double().sum()), float((v.double() ** 2).sum())] for v in sd.values()])


def main():
    torch.set_num_threads(min(os.cpu_count() or 8, 16))
    out = {}
    for cls in CLASSES:
        default_meta(cls, out)
    for name in R.CASES:
        run_case(name, out)
    path = HERE / "golden_ast_small.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
