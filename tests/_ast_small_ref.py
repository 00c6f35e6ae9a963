"""Restatement of the small-AST family (ASTViTSmall / ASTMiniViT) in torch ops with explicit dropout masks, and of
the project's two mask functions in plain numpy: the checker of tests/test_ast_small_cpu.py,
tests/test_gpu_attn_dropout.py and tests/test_gpu_ast_small.py.

Masks
  * ``attn_keep``: keep(seed, b, h, q, k) of the attention kernels (include/miaudio.h, mia_attn_fwd_dropout): one
    splitmix64 per 2 x 2 (query pair, key pair) cell, cut into four 16-bit fields, field >= round(p * 65536).
  * ``elem_keep``: mia_dropout / mia_dropout_apply: hash_u01(seed, flat index) >= p, i.e. oracle.synth.hash_uniform.

Model: ``forward`` follows the module tree (Conv2d patch embedding, cls + position table slice, pre-LN blocks on
nn.MultiheadAttention's packed in_proj with dropout on the probabilities, Linear-GELU-Dropout-Linear-Dropout, final
LayerNorm, sigmoid head on the CLS token; LayerNorm eps 1e-5), in the dtype of the tensors it is handed and under
CPU autocast when the caller enables it.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle.synth import hash_uniform

LN_EPS = 1e-5
_G = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = x + _G
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def attn_thr(p: float) -> int:
    """16-bit keep threshold of a rate (the kernels' quantisation: p_eff = thr / 65536)."""
    return min(int(np.rint(np.float32(p) * np.float32(65536.0))), 65535)


def attn_p_eff(p: float) -> float:
    return attn_thr(p) / 65536.0


def attn_scale(p: float) -> float:
    """c = 1 / (1 - p_eff) as the kernels hold it (float32)."""
    return float(np.float32(65536.0 / (65536.0 - attn_thr(p))))


def attn_keep(seed: int, b, h, q, k, p: float):
    """keep(seed, b, h, q, k): bool array of the broadcast shape of b, h, q, k."""
    b, h, q, k = (np.asarray(v, dtype=np.uint64) for v in (b, h, q, k))
    seed = np.uint64(int(seed) & (2 ** 64 - 1))
    s32, s16, one = np.uint64(32), np.uint64(16), np.uint64(1)
    key = splitmix64(seed ^ splitmix64((b << s32) | h))
    w = splitmix64(key ^ (((q >> one) << s32) | (k >> one)))
    field = (w >> (s32 * (q & one) + s16 * (k & one))) & np.uint64(0xFFFF)
    return field >= np.uint64(attn_thr(p))


def attn_keep_mask(seed: int, B: int, H: int, N: int, p: float) -> np.ndarray:
    """(B, H, N, N) bool, [b, h, q, k]."""
    b = np.arange(B).reshape(B, 1, 1, 1)
    h = np.arange(H).reshape(1, H, 1, 1)
    q = np.arange(N).reshape(1, 1, N, 1)
    k = np.arange(N).reshape(1, 1, 1, N)
    return attn_keep(seed, b, h, q, k, p)


def elem_keep(seed: int, shape, p: float) -> np.ndarray:
    """mia_dropout's keep mask over a contiguous tensor of ``shape``."""
    return hash_uniform(int(seed) & (2 ** 64 - 1), shape, 0.0, 1.0) >= np.float32(p)


def elem_scale(p: float) -> float:
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ model
def block_masks(seeds, B: int, H: int, N: int, D: int, p: float, dtype=torch.float64):
    """Scaled masks of one block for its three seeds (attention, after GELU, after fc2): tensors (B, H, N, N),
    (B, N, 4D), (B, N, D) holding 0 or 1 / (1 - p)."""
    sa, s1, s2 = (int(s) for s in seeds)
    return (torch.from_numpy(attn_keep_mask(sa, B, H, N, p)).to(dtype) * attn_scale(p),
            torch.from_numpy(elem_keep(s1, (B, N, 4 * D), p)).to(dtype) * elem_scale(p),
            torch.from_numpy(elem_keep(s2, (B, N, D), p)).to(dtype) * elem_scale(p))


def forward(sd: dict, spec: torch.Tensor, stride: int, heads: int, masks=None) -> torch.Tensor:
    """Sigmoid probabilities (B, classes) from a state dict of tensors; masks: per block (attn, mlp1, mlp2) scaled
    masks or None (eval mode = train mode with p = 0)."""
    depth = 1 + max(int(k.split(".")[1]) for k in sd if k.startswith("blocks."))
    x = F.conv2d(spec[:, None].to(sd["patch_embed.proj.weight"].dtype), sd["patch_embed.proj.weight"],
                 sd["patch_embed.proj.bias"], stride=stride)
    x = x.flatten(2).transpose(1, 2)
    B, _, D = x.shape
    x = torch.cat((sd["cls_token"].expand(B, -1, -1).to(x.dtype), x), dim=1)
    N = x.shape[1]
    x = x + sd["pos_embed"][:, :N]
    hd = D // heads
    for i in range(depth):
        pre = f"blocks.{i}."
        m = masks[i] if masks is not None else (None, None, None)
        h = F.layer_norm(x, (D,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], LN_EPS)
        qkv = F.linear(h, sd[pre + "attn.in_proj_weight"], sd[pre + "attn.in_proj_bias"])
        q, k, v = qkv.view(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4).unbind(0)
        a = torch.softmax((q * (1.0 / math.sqrt(hd))) @ k.transpose(-1, -2), dim=-1)
        if m[0] is not None:
            a = a * m[0].to(a.dtype)
        o = (a @ v).transpose(1, 2).reshape(B, N, D)
        x = x + F.linear(o, sd[pre + "attn.out_proj.weight"], sd[pre + "attn.out_proj.bias"])
        h = F.layer_norm(x, (D,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], LN_EPS)
        g = F.gelu(F.linear(h, sd[pre + "mlp.0.weight"], sd[pre + "mlp.0.bias"]))
        if m[1] is not None:
            g = g * m[1].to(g.dtype)
        y = F.linear(g, sd[pre + "mlp.3.weight"], sd[pre + "mlp.3.bias"])
        if m[2] is not None:
            y = y * m[2].to(y.dtype)
        x = x + y
    x = F.layer_norm(x, (D,), sd["norm.weight"], sd["norm.bias"], LN_EPS)
    return torch.sigmoid(F.linear(x[:, 0], sd["head.weight"], sd["head.bias"]))


def soft_ce(probs: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The engine's soft-label cross-entropy, on the model's returned probabilities as the engine applies it."""
    return -torch.sum(y * torch.log(torch.softmax(probs, dim=1) + 1e-8), dim=1).mean()


def hash_init(keys_shapes, seed: int) -> dict:
    """Deterministic float32 parameters regenerated wherever needed: weights (ndim >= 2) uniform in
    +-1 / sqrt(fan_in), LayerNorm weights in [0.5, 1.5], cls / position table in +-0.5, every bias in +-0.2
    (no zero bias, no zero cls); hash_uniform(seed + position)."""
    out = {}
    for i, (k, shape) in enumerate(keys_shapes):
        shape = tuple(shape)
        if k in ("cls_token", "pos_embed"):
            lo, hi = -0.5, 0.5
        elif len(shape) >= 2:
            b = 1.0 / math.sqrt(int(np.prod(shape[1:])))
            lo, hi = -b, b
        elif "norm" in k and k.endswith(".weight"):
            lo, hi = 0.5, 1.5
        else:
            lo, hi = -0.2, 0.2
        out[k] = hash_uniform(seed + i, shape, lo, hi).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ fixture cases
# name: (class name, constructor kwargs, input (B, F, T), seeds (x, labels, init, masks))
CASES = {
    "S": ("ASTViTSmall", dict(sample_rate=7200, patch_stride=10, overlap=6, num_classes=10, depth=2, f_dim=36),
          (2, 36, 446), (41001, 41002, 41003, 41004)),
    "M": ("ASTMiniViT", dict(sample_rate=7200, patch_stride=16, overlap=0, num_classes=50, depth=2, f_dim=48),
          (3, 48, 330), (42001, 42002, 42003, 42004)),
}
HEADS = {"ASTViTSmall": 6, "ASTMiniViT": 3}
P_DROP = 0.1
N_SAMPLED, SAMPLE_SEED = 96, 8777
LARGE_NUMEL = 256  # gradients with more entries are stored as sampled entries (+ row / column sums of matrices)


def sample_indices(j: int, n: int) -> np.ndarray:
    idx = (hash_uniform(SAMPLE_SEED + j, (N_SAMPLED,), 0.0, 1.0).astype(np.float64) * n).astype(np.int64)
    return idx.clip(0, n - 1)


def case_inputs(name: str):
    """(spec (B, F, T) f32 numpy in [-1, 1), y one-hot (B, C) f32 numpy) of a case."""
    _, kw, shape, (sx, sl, _, _) = CASES[name]
    spec = hash_uniform(sx, shape)
    C = kw["num_classes"]
    labels = (hash_uniform(sl, (shape[0],), 0.0, 1.0).astype(np.float64) * C).astype(np.int64).clip(0, C - 1)
    y = np.zeros((shape[0], C), dtype=np.float32)
    y[np.arange(shape[0]), labels] = 1.0
    return spec, y


def case_seeds(name: str, depth: int = 2) -> np.ndarray:
    """(depth, 3) mask seeds of a case: block i uses seed_masks + 3 i + (0 attention, 1 after GELU, 2 after fc2)."""
    sm = CASES[name][3][3]
    return np.array([[sm + 3 * i + j for j in range(3)] for i in range(depth)], dtype=np.int64)


def case_geometry(name: str):
    """(B, N, D, H, stride) of a case."""
    cls, kw, (B, Fm, Tf), _ = CASES[name]
    st = kw["patch_stride"]
    N = ((Fm - 16) // st + 1) * ((Tf - 16) // st + 1) + 1
    D = 384 if cls == "ASTViTSmall" else 192
    return B, N, D, HEADS[cls], st


def run_case(name: str, keys_shapes, masked: bool, dtype=torch.float64, autocast_bf16: bool = False) -> dict:
    """One forward + loss + backward of the restatement on a case: dict(probs, loss, grads {key: tensor})."""
    B, N, D, H, st = case_geometry(name)
    init = hash_init(keys_shapes, CASES[name][3][2])
    sd = {k: torch.from_numpy(v.copy()).to(dtype).requires_grad_(True) for k, v in init.items()}
    spec, y = case_inputs(name)
    masks = None
    if masked:
        masks = [block_masks(s, B, H, N, D, P_DROP, dtype) for s in case_seeds(name)]
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast_bf16):
        probs = forward(sd, torch.from_numpy(spec).to(dtype), st, H, masks)
    loss = soft_ce(probs.to(dtype), torch.from_numpy(y).to(dtype))
    loss.backward()
    return dict(probs=probs.detach().double(), loss=loss.detach().double(),
                grads={k: v.grad.detach().double() for k, v in sd.items()})


def quantities(run: dict, order) -> dict:
    """{name: float64 numpy} of a run in the fixture's form: probs, loss, g:<param> in full for small gradients,
    gs:<param> (sampled entries) + gsum:<param> (sums along the longer side) for those above LARGE_NUMEL entries."""
    out = {"probs": run["probs"].numpy(), "loss": run["loss"].numpy()}
    for j, k in enumerate(order):
        g = run["grads"][k].double().cpu().numpy()
        if g.size > LARGE_NUMEL:
            out["gs:" + k] = g.ravel()[sample_indices(j, g.size)]
            if sum(d > 1 for d in g.shape) > 1:
                # sums along the longer side of the matrix (first axis x the rest, leading 1s dropped) -- but never
                # over the residual stream's width: every path from it to the loss ends in a LayerNorm, so those sums
                # are exactly 0 (rounding noise): the position table is summed over tokens, the patch filter over pixels
                g2 = g.reshape([s for s in g.shape if s > 1][0], -1)
                if k == "pos_embed":
                    out["gsum:" + k] = g2.sum(0)
                elif g2.shape[0] <= g2.shape[1] or k == "patch_embed.proj.weight":
                    out["gsum:" + k] = g2.sum(1)
                else:
                    out["gsum:" + k] = g2.sum(0)
        else:
            out["g:" + k] = g
    return out


def fixture_quantities(gm: dict, name: str, mode: str) -> dict:
    pre = f"{name}__{mode}__"
    return {k[len(pre):].replace("__", ":", 1) if k[len(pre)] == "g" else k[len(pre):]: v
            for k, v in gm.items() if k.startswith(pre)}
