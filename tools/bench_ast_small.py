#!/usr/bin/env python
"""Time what the small-AST family (ASTViTSmall / ASTMiniViT) adds, on one MI355X.

    python tools/bench_ast_small.py [--batch 64] [--iters 20] [--warmup 3] [--skip-torch] [--out FILE]

Protocol as tools/bench_leaf_model.py: HIP events, median of --iters after --warmup.  ESC-50 clips (5 s, 128 mel
bins x 1379 frames): 689 tokens for model=ast_small (stride 16), 1645 for model=ast_mini (stride 10).  Records
  * attention forward and backward at ast_small's token count (N = 689, H = 6) for p = 0 (the existing entry
    points) and p = 0.1 (mia_attn_fwd_dropout / mia_attn_bwd_dropout), bf16 (saved-Q' forward, two-kernel backward)
    and f32 (exact kernels), and the dropout / no-dropout ratio of each;
  * the three mia_dropout_apply passes of one block at that shape: after GELU (on gelu(u) and gelu'(u), bf16 in
    place), after fc2 (f32, residual add, in place), and the masked copy of the residual gradient (bf16);
  * the bf16 train step (forward, backward, FusedAdam with clip) of both models, and the MLP passes' share of it;
  * the same module tree run through torch ops (the model's own nn.MultiheadAttention / Sequential modules under
    bf16 autocast) on the same GPU: forward and backward.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "dl-sound-classification_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

F_MEL, T_FRAMES, CLASSES = 128, 1379, 50
P = 0.1


def timed(fn, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def bench_attention(B, N, H, iters, warmup, dev):
    from src.miaudio import lib as L
    lib = L.load()
    out = []
    for dt, tdt in ((L.BF16, torch.bfloat16), (L.F32, torch.float32)):
        g = torch.Generator().manual_seed(1)
        qkv = (torch.randn(B, N, 3 * H * 64, generator=g) * 1.5).to(dev, tdt)
        do = torch.randn(B, N, H * 64, generator=g).to(dev, tdt)
        o = torch.empty(B, N, H * 64, dtype=tdt, device=dev)
        dq = torch.empty_like(qkv)
        lse = torch.empty(B, H, N, device=dev)
        work = torch.empty(int(lib.mia_attn_bwd_workspace_bytes(dt, B, N, H)), dtype=torch.uint8, device=dev)
        bf = dt == L.BF16
        row = {"dtype": "bf16" if bf else "f32", "B": B, "N": N, "H": H}
        for p in (0.0, P):
            def fwd():
                if p == 0.0 and bf:
                    L.check(lib.mia_attn_fwd_save_q(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), None, None,
                                                    work.data_ptr(), B, N, H, 0.125, L.stream_ptr()), "fwd")
                elif p == 0.0:
                    L.check(lib.mia_attn_fwd(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), dt, B, N, H, 0.125,
                                             L.stream_ptr()), "fwd")
                else:
                    L.check(lib.mia_attn_fwd_dropout(qkv.data_ptr(), o.data_ptr(), lse.data_ptr(),
                                                     work.data_ptr() if bf else None, dt, B, N, H, 0.125, p, 17,
                                                     L.stream_ptr()), "fwd")

            def bwd():
                if p == 0.0 and bf:
                    L.check(lib.mia_attn_bwd_saved_q(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                                     dq.data_ptr(), work.data_ptr(), B, N, H, 0.125, L.stream_ptr()),
                            "bwd")
                elif p == 0.0:
                    L.check(lib.mia_attn_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(), dq.data_ptr(),
                                             work.data_ptr(), dt, B, N, H, 0.125, L.stream_ptr()), "bwd")
                else:
                    L.check(lib.mia_attn_bwd_dropout(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                                     dq.data_ptr(), work.data_ptr(), dt, B, N, H, 0.125, p, 17,
                                                     int(bf), L.stream_ptr()), "bwd")
            tag = "p0" if p == 0.0 else "drop"
            row[f"fwd_ms_{tag}"] = timed(fwd, iters, warmup)
            row[f"bwd_ms_{tag}"] = timed(bwd, iters, warmup)
        row["fwd_drop_over_p0"] = row["fwd_ms_drop"] / row["fwd_ms_p0"]
        row["bwd_drop_over_p0"] = row["bwd_ms_drop"] / row["bwd_ms_p0"]
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def bench_dropout_apply(T, D, iters, warmup, dev):
    from src.models.ast_hip import _dropout_apply
    gu = torch.randn(T, 4 * D, device=dev).to(torch.bfloat16)
    y = torch.randn(T, D, device=dev)
    xm = torch.randn(T, D, device=dev)
    dxb = torch.randn(T, D, device=dev).to(torch.bfloat16)
    dy = torch.empty_like(dxb)
    row = {"tokens": T, "D": D,
           "after_gelu_ms": timed(lambda: _dropout_apply(gu, None, gu, P, 5), iters, warmup),  # once per tensor
           "after_fc2_residual_ms": timed(lambda: _dropout_apply(y, xm, y, P, 6), iters, warmup),
           "masked_dy_ms": timed(lambda: _dropout_apply(dxb, None, dy, P, 6), iters, warmup)}
    row["per_block_ms"] = 2 * row["after_gelu_ms"] + row["after_fc2_residual_ms"] + row["masked_dy_ms"]
    print(json.dumps(row), flush=True)
    return row


def make(name, dev):
    from src.models.ast_mini import ASTMiniViT
    from src.models.ast_small import ASTViTSmall
    torch.manual_seed(0)
    kw = dict(patch_stride=16, overlap=0) if name == "ast_small" else {}
    m = (ASTViTSmall if name == "ast_small" else ASTMiniViT)(num_classes=CLASSES, **kw)
    m.compute_dtype = "bf16"
    return m.to(dev).train()


def bench_hip_step(name, B, iters, warmup, dev):
    from src.miaudio import kernels as K
    from src.training.optim import FusedAdam
    m = make(name, dev)
    opt = FusedAdam(m.parameters(), lr=1e-4, clip=1.0)
    x = torch.randn(B, F_MEL, T_FRAMES, device=dev) * 0.5
    y = torch.zeros(B, CLASSES, device=dev)
    y[torch.arange(B), torch.arange(B) % CLASSES] = 1.0
    fw, bw, st = [], [], []
    for i in range(warmup + iters):
        for q in m.parameters():
            q.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        probs = m(x)
        e[1].record()
        _, dz, _ = K.soft_ce(probs.detach().float(), y, input_sigmoid=False)
        probs.backward(dz)
        e[2].record()
        opt.step()
        e[3].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            st.append(e[2].elapsed_time(e[3]))
    stride = m.patch_stride
    N = ((F_MEL - 16) // stride + 1) * ((T_FRAMES - 16) // stride + 1) + 1
    r = {"name": f"hip_{name}_bf16", "batch": B, "tokens": N, "depth": len(m.blocks), "fwd_ms": statistics.median(fw),
         "bwd_ms": statistics.median(bw), "optim_ms": statistics.median(st)}
    r["step_ms"] = r["fwd_ms"] + r["bwd_ms"] + r["optim_ms"]
    r["clips_per_s"] = B / r["step_ms"] * 1e3
    print(json.dumps(r), flush=True)
    return r


def torch_forward(m, x):
    """The module tree through torch ops (what the reference's forward does with these modules)."""
    t = m.patch_embed.proj(x[:, None]).flatten(2).transpose(1, 2)
    t = torch.cat((m.cls_token.expand(t.shape[0], -1, -1).to(t.dtype), t), dim=1)
    t = t + m.pos_embed[:, :t.shape[1]]
    for blk in m.blocks:
        h = blk.norm1(t)
        t = t + blk.attn(h, h, h)[0]
        t = t + blk.mlp(blk.norm2(t))
    return torch.sigmoid(m.head(m.norm(t)[:, 0]))


def bench_torch(name, B, iters, warmup, dev):
    m = make(name, dev)
    x = torch.randn(B, F_MEL, T_FRAMES, device=dev) * 0.5
    gl = torch.ones(B, CLASSES, device=dev) / B
    fw, bw = [], []
    for i in range(warmup + iters):
        for q in m.parameters():
            q.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            probs = torch_forward(m, x)
        e[1].record()
        probs.float().backward(gl)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
    r = {"name": f"torch_{name}_bf16_autocast", "batch": B, "fwd_ms": statistics.median(fw),
         "bwd_ms": statistics.median(bw)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "ast_small_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B = a.batch
    n_small = 8 * ((T_FRAMES - 16) // 16 + 1) + 1
    res = {"config": {"mel": F_MEL, "frames": T_FRAMES, "classes": CLASSES, "p": P,
                      "device": torch.cuda.get_device_name(0), "method": "HIP events, median"},
           "attention": bench_attention(B, n_small, 6, a.iters, a.warmup, dev),
           "dropout_apply": bench_dropout_apply(B * n_small, 384, a.iters, a.warmup, dev), "steps": [], "ratios": []}
    for name in ("ast_small", "ast_mini"):
        h = bench_hip_step(name, B, a.iters, a.warmup, dev)
        res["steps"].append(h)
        ratio = {"model": name}
        if name == "ast_small":  # the passes were timed at this model's shape
            ratio["mlp_dropout_passes_share_of_step"] = h["depth"] * res["dropout_apply"]["per_block_ms"] / h["step_ms"]
        if not a.skip_torch:
            t = bench_torch(name, B, a.iters, a.warmup, dev)
            res["steps"].append(t)
            ratio["hip_over_torch_fwd_bwd"] = (h["fwd_ms"] + h["bwd_ms"]) / (t["fwd_ms"] + t["bwd_ms"])
        res["ratios"].append(ratio)
        print(json.dumps(ratio), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
