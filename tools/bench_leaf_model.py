#!/usr/bin/env python
"""Time LeafModel (frontend + trunk + classifier) forward, backward and the clip + Adam step on one MI355X.

    python tools/bench_leaf_model.py [--batches 64,4] [--modes bf16,f32] [--iters 20] [--warmup 3] [--out FILE]

Protocol as tools/bench_leaf.py: HIP events, median of --iters after --warmup.  Shipped config: F = 128 filters,
Kt = 401 taps, 5 s clips (T = 220 500), 50 classes.  Per (mode, batch):
  * forward, backward and optimizer-step times of the whole model (FusedAdam, clip 1.0);
  * per-tag times from the kernels' own event probes (miaudio.kernels.PROBE), so the frontend (leaf.energy.*),
    channels-last PCEN, each trunk block (its conv GEMMs and its glue kernels) and the MLP are separable;
  * the same trunk + classifier (the model's own nn.Sequential modules: Conv1d / BatchNorm1d / ReLU / MaxPool1d,
    AdaptiveAvgPool1d, Linear / BatchNorm1d / ReLU / Dropout) as torch ops on the same GPU, fed the frontend's
    output, as it comes: bf16 autocast for the bf16 mode, f32 for the f32 mode, no tuning either way.
Ratios per run: the HIP trunk (everything but leaf.energy.*, channels-last PCEN included) over the frontend's time in
the same run and over the torch-op trunk, and the HIP trunk without PCEN over the torch-op trunk (the torch-op
sequence starts behind PCEN: the same scope).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "dl-sound-classification_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

F, KT, T, CLASSES = 128, 401, 220_500, 50
TAGS = ["leaf.energy.fwd", "leaf.pcen_cl.fwd"] + \
       [f"leaf.b{l}.{k}.fwd" for l in range(3) for k in ("conv", "glue")] + ["leaf.mlp.fwd", "leaf.mlp.bwd"] + \
       [f"leaf.b{l}.{k}" for l in (2, 1, 0) for k in ("glue.bwd", "conv.wgrad", "conv.dgrad")] + \
       ["leaf.pcen_cl.bwd", "leaf.energy.bwd", "optim.step"]


def med(v):
    return statistics.median(v) if v else float("nan")


def inputs(B, dev):
    from oracle.synth import synth_waveform
    x = torch.from_numpy(synth_waveform(11, 4, T)).to(dev).repeat(B // 4 + 1, 1)[:B].contiguous()
    y = torch.zeros(B, CLASSES, device=dev)
    y[torch.arange(B), torch.arange(B) % CLASSES] = 1.0
    return x, y


def bench_hip(mode, B, iters, warmup, dev):
    from src.miaudio import kernels as K
    from src.models.leaf import LeafModel
    from src.training.optim import FusedAdam
    torch.manual_seed(0)
    m = LeafModel(n_filters=F, kernel_size=KT, num_classes=CLASSES, compute_dtype=mode).to(dev).train()
    opt = FusedAdam(m.parameters(), lr=1e-4, clip=1.0)
    x, y = inputs(B, dev)
    fw, bw, st = [], [], []
    per_tag = {t: [] for t in TAGS}
    for i in range(warmup + iters):
        K.PROBE = {t: [] for t in TAGS}
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        for q in m.parameters():
            q.grad = None
        e[0].record()
        logits = m(x)
        e[1].record()
        _, dlogits, _ = K.soft_ce(logits.detach(), y, input_sigmoid=False)
        logits.backward(dlogits)
        e[2].record()
        opt.step()
        e[3].record()
        torch.cuda.synchronize()
        probes, K.PROBE = K.PROBE, None
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            st.append(e[2].elapsed_time(e[3]))
            for t, recs in probes.items():
                per_tag[t].append(sum(r[0].elapsed_time(r[1]) for r in recs))
    tags = {t: med(v) for t, v in per_tag.items()}
    fe_f, fe_b = tags["leaf.energy.fwd"], tags["leaf.energy.bwd"]
    r = {"name": f"hip_{mode}", "batch": B, "iters": iters, "fwd_ms": med(fw), "bwd_ms": med(bw), "step_ms": med(st),
         "fwd_ms_min": min(fw), "bwd_ms_min": min(bw), "clips_per_s": B / (med(fw) + med(bw) + med(st)) * 1e3,
         "frontend_fwd_ms": fe_f, "frontend_bwd_ms": fe_b, "trunk_fwd_ms": med(fw) - fe_f, "trunk_bwd_ms": med(bw) - fe_b,
         # the torch-op baseline starts behind PCEN: the same scope on this side
         "trunk_no_pcen_fwd_ms": med(fw) - fe_f - tags["leaf.pcen_cl.fwd"],
         "trunk_no_pcen_bwd_ms": med(bw) - fe_b - tags["leaf.pcen_cl.bwd"], "tags_ms": tags}
    print(json.dumps(r), flush=True)
    return r


def bench_torch_trunk(mode, B, iters, warmup, dev):
    """The trunk + classifier on torch ops (the model's own nn modules), fed the frontend output."""
    from src.models.leaf import LeafModel
    torch.manual_seed(0)
    m = LeafModel(n_filters=F, kernel_size=KT, num_classes=CLASSES, compute_dtype=mode).to(dev).train()
    x, _ = inputs(B, dev)
    with torch.no_grad():
        from src.models.leaf import LeafFrontend
        fe = LeafFrontend(n_filters=F, kernel_size=KT, compute_dtype=mode).to(dev)
        yin = fe(x).detach().requires_grad_(True)  # conv1's data gradient is part of the HIP trunk's backward too
    gl = torch.ones(B, CLASSES, device=dev) / B
    fw, bw = [], []
    for i in range(warmup + iters):
        for q in m.parameters():
            q.grad = None
        yin.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "bf16"):
            logits = m.classifier(m.pooling(m.conv_block(yin)).squeeze(-1))
        e[1].record()
        logits.float().backward(gl)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
    r = {"name": f"torch_trunk_{mode}", "batch": B, "iters": iters, "fwd_ms": med(fw), "bwd_ms": med(bw),
         "fwd_ms_min": min(fw), "bwd_ms_min": min(bw)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,4")
    ap.add_argument("--modes", default="bf16,f32")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "leaf_model_bench.json"))
    a = ap.parse_args()
    if a.iters < 20:
        print("note: the documented numbers are medians of >= 20", file=sys.stderr)
    dev = torch.device("cuda:0")
    res = {"config": {"F": F, "Kt": KT, "T": T, "classes": CLASSES, "device": torch.cuda.get_device_name(0),
                      "method": "HIP events, median"}, "runs": [], "ratios": []}
    for B in (int(b) for b in a.batches.split(",")):
        for mode in a.modes.split(","):
            h = bench_hip(mode, B, a.iters, a.warmup, dev)
            res["runs"].append(h)
            ratio = {"mode": mode, "batch": B,
                     "trunk_over_frontend_fwd": h["trunk_fwd_ms"] / h["frontend_fwd_ms"],
                     "trunk_over_frontend_bwd": h["trunk_bwd_ms"] / h["frontend_bwd_ms"]}
            if not a.skip_torch:
                t = bench_torch_trunk(mode, B, a.iters, a.warmup, dev)
                res["runs"].append(t)
                ratio.update(same_scope_hip_over_torch_fwd=h["trunk_no_pcen_fwd_ms"] / t["fwd_ms"],
                             same_scope_hip_over_torch_bwd=h["trunk_no_pcen_bwd_ms"] / t["bwd_ms"],
                             same_scope_hip_over_torch_fwd_bwd=(h["trunk_no_pcen_fwd_ms"] + h["trunk_no_pcen_bwd_ms"]) /
                             (t["fwd_ms"] + t["bwd_ms"]),
                             hip_trunk_over_torch_trunk_fwd=h["trunk_fwd_ms"] / t["fwd_ms"],
                             hip_trunk_over_torch_trunk_bwd=h["trunk_bwd_ms"] / t["bwd_ms"],
                             hip_trunk_over_torch_trunk_fwd_bwd=(h["trunk_fwd_ms"] + h["trunk_bwd_ms"]) /
                             (t["fwd_ms"] + t["bwd_ms"]))
            res["ratios"].append(ratio)
            print(json.dumps(ratio), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
