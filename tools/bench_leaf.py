#!/usr/bin/env python
"""Time LeafFrontend (fused Gabor energy + pool, PCEN) forward and backward on one MI355X.

    python tools/bench_leaf.py [--batch 64] [--torch-batch 4] [--iters 20] [--warmup 3] [--out FILE]

Shipped config: F = 128 filters, Kt = 401 taps, 5 s clips (T = 220 500), pool 160.  Per mode (bf16, f32):
HIP-event times of the forward and the backward, median of --iters after --warmup, clips/s, and the counted
FLOP over time as a fraction of the 2.5 PFLOP/s bf16 MFMA peak.  Counted FLOP: forward 2 * 2F * Kt * T per
clip (the filterbank as a GEMM; square, pool and PCEN are not counted), backward twice that (the tile is
recomputed, then contracted into dw).
At --torch-batch the same math runs as torch ops on the same GPU (conv1d x 2, square, avg_pool1d, the PCEN
expression; forward and autograd backward), next to the fused path at that batch.  The torch path is run
as it comes: f32 tensors, MIOpen's default find mode, no tuning either way.
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

PEAK = 2.5e15
F, KT, T, POOL = 128, 401, 220_500, 160


def timed(fn_fwd, fn_bwd, iters, warmup):
    fw, bw = [], []
    for i in range(warmup + iters):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        out = fn_fwd()
        e[1].record()
        fn_bwd(out)
        e[2].record()
        torch.cuda.synchronize()
        if i >= warmup:
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
    return statistics.median(fw), statistics.median(bw), min(fw), min(bw)


def report(name, B, fwd_ms, bwd_ms, fmin, bmin, iters):
    flop_f = 2.0 * 2 * F * KT * T * B
    r = {"name": name, "batch": B, "iters": iters, "fwd_ms": fwd_ms, "bwd_ms": bwd_ms, "fwd_ms_min": fmin,
         "bwd_ms_min": bmin, "fwd_clips_per_s": B / fwd_ms * 1e3, "fwd_bwd_clips_per_s": B / (fwd_ms + bwd_ms) * 1e3,
         "fwd_flop": flop_f, "bwd_flop": 2 * flop_f, "fwd_frac_of_bf16_peak": flop_f / (fwd_ms * 1e-3 * PEAK),
         "bwd_frac_of_bf16_peak": 2 * flop_f / (bwd_ms * 1e-3 * PEAK)}
    print(json.dumps(r), flush=True)
    return r


def bench_fused(mode, B, iters, warmup, dev):
    from oracle.synth import synth_waveform
    from src.models.leaf import LeafFrontend
    m = LeafFrontend(n_filters=F, kernel_size=KT, pool=POOL, compute_dtype=mode).to(dev)
    x = torch.from_numpy(synth_waveform(11, 4, T)).to(dev).repeat(B // 4 + 1, 1)[:B].contiguous()
    gy = torch.ones(B, F, T // POOL, device=dev)

    def bwd(y):
        for q in m.parameters():
            q.grad = None
        y.backward(gy)

    return report(f"fused_{mode}", B, *timed(lambda: m(x), bwd, iters, warmup), iters)


def bench_torch(B, iters, warmup, dev):
    from oracle.synth import synth_waveform
    from src.models.leaf import LeafFrontend
    m = LeafFrontend(n_filters=F, kernel_size=KT, pool=POOL).to(dev)
    x = torch.from_numpy(synth_waveform(11, B, T)).to(dev)[:, None, :]
    gy = torch.ones(B, F, T // POOL, device=dev)
    Fn = torch.nn.functional

    def fwd():
        w = m.gabor.filters()
        xr = Fn.conv1d(x, w[0][:, None, :], padding=KT // 2)
        xi = Fn.conv1d(x, w[1][:, None, :], padding=KT // 2)
        P = Fn.avg_pool1d(xr ** 2 + xi ** 2, POOL)
        M = Fn.avg_pool1d(P, 5, stride=1, padding=2)
        return torch.log(P / (m.pcen.eps + M) ** m.pcen.r.view(1, -1, 1) + m.pcen.delta.view(1, -1, 1))

    def bwd(y):
        for q in m.parameters():
            q.grad = None
        y.backward(gy)

    return report("torch_ops_f32", B, *timed(fwd, bwd, iters, warmup), iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--torch-batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="bf16,f32")
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=str(REPO / "profiles" / "leaf_frontend_bench.json"))
    a = ap.parse_args()
    if a.iters < 20:
        print("note: the documented numbers are medians of >= 20", file=sys.stderr)
    dev = torch.device("cuda:0")
    res = {"config": {"F": F, "Kt": KT, "T": T, "pool": POOL, "peak_flops": PEAK,
                      "device": torch.cuda.get_device_name(0), "method": "HIP events, median"}, "runs": []}
    for mode in a.modes.split(","):
        res["runs"].append(bench_fused(mode, a.batch, a.iters, a.warmup, dev))
    for mode in a.modes.split(","):
        res["runs"].append(bench_fused(mode, a.torch_batch, a.iters, a.warmup, dev))
    if not a.skip_torch:
        res["runs"].append(bench_torch(a.torch_batch, a.iters, a.warmup, dev))
        by = {(r["name"], r["batch"]): r for r in res["runs"]}
        t, f = by[("torch_ops_f32", a.torch_batch)], by.get(("fused_bf16", a.torch_batch))
        if f:
            res["fused_bf16_vs_torch"] = {"batch": a.torch_batch, "fwd_speedup": t["fwd_ms"] / f["fwd_ms"],
                                          "bwd_speedup": t["bwd_ms"] / f["bwd_ms"],
                                          "fwd_bwd_speedup": (t["fwd_ms"] + t["bwd_ms"]) / (f["fwd_ms"] + f["bwd_ms"])}
            print(json.dumps(res["fused_bf16_vs_torch"]), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
