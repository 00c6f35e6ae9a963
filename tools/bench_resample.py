#!/usr/bin/env python
"""Time mia_resample (GpuResample) on one MI355X against the reference's form of the same transform.

    python tools/bench_resample.py [--batch 256] [--iters 30] [--warmup 5] [--miopen-find-mode MODE] [--out FILE]

Shapes: B clips of 220 500 samples 44.1 -> 16 kHz (o / n = 441 / 160, K = 475 taps, 80 000 samples out) and B clips of
80 000 samples 16 -> 44.1 kHz (160 / 441, K = 174, 220 500 out).  Per shape, HIP-event times (median and minimum of
--iters launches after --warmup):
  * the kernel: ms per launch, TFLOP/s of the counted 2 * K * Tout * B, that over the 157.3 TFLOP/s f32 peak
    (vector and f32-MFMA peaks are equal), and GB/s of the clips read once plus the output written once;
  * torchaudio's form on the same GPU, as torch runs it: F.pad(x, (width, width + o)), F.conv1d(x[:, None],
    taps[:, None], stride=o), transpose(1, 2).reshape(B, -1)[..., :Tout] -- the whole expression, and the conv1d
    call alone.  --miopen-find-mode sets MIOPEN_FIND_MODE before torch loads MIOpen (default: MIOpen's own).
The two results are compared elementwise before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
for p in (str(REPO), str(REPO / "dl-sound-classification_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_F32 = 157.3e12
SHAPES = [(44_100, 16_000, 220_500), (16_000, 44_100, 80_000)]


def timed(fn, iters, warmup):
    import torch
    ms = []
    for i in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--miopen-find-mode", default=None)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.miopen_find_mode:
        os.environ["MIOPEN_FIND_MODE"] = a.miopen_find_mode
    import torch
    import torch.nn.functional as Fn

    from src.datasets.resample import GpuResample
    dev = torch.device("cuda:0")
    res = {"config": {"batch": a.batch, "iters": a.iters, "warmup": a.warmup, "peak_f32_flops": PEAK_F32,
                      "miopen_find_mode": os.environ.get("MIOPEN_FIND_MODE", "default"),
                      "device": torch.cuda.get_device_name(0), "method": "HIP events, median"}, "runs": []}
    for orig, new, T in SHAPES:
        rs = GpuResample(orig, new)
        B, Tout = a.batch, rs.out_len(T)
        x = torch.randn(B, T, device=dev, generator=torch.Generator(device=dev).manual_seed(orig))
        taps = rs.taps_on(dev)
        flop, nbytes = 2.0 * rs.K * Tout * B, 4.0 * B * (T + Tout)
        out = rs(x)
        r = {"shape": f"{orig}->{new}", "o": rs.o, "n": rs.n, "K": rs.K, "T": T, "Tout": Tout, "flop": flop,
             "bytes": nbytes}

        def conv_form():
            y = Fn.conv1d(Fn.pad(x, (rs.width, rs.width + rs.o))[:, None], taps[:, None], stride=rs.o)
            return y.transpose(1, 2).reshape(B, -1)[..., :Tout]

        if not a.skip_torch:
            print(f"{r['shape']}: conv1d form, first call ...", flush=True)
            ref = conv_form()
            r["max_abs_diff_vs_conv1d"] = float((out - ref).abs().max())
            r["max_abs_out"] = float(out.abs().max())
            del ref
        ms, ms_min = timed(lambda: rs(x), a.iters, a.warmup)
        r.update(kernel_ms=ms, kernel_ms_min=ms_min, tflops=flop / ms * 1e-9, frac_of_f32_peak=flop / (ms * 1e-3) / PEAK_F32,
                 gbytes_per_s=nbytes / ms * 1e-6)
        if not a.skip_torch:
            r["conv1d_form_ms"], r["conv1d_form_ms_min"] = timed(conv_form, a.iters, a.warmup)
            xp = Fn.pad(x, (rs.width, rs.width + rs.o))[:, None]
            w3 = taps[:, None]
            r["conv1d_alone_ms"], r["conv1d_alone_ms_min"] = timed(lambda: Fn.conv1d(xp, w3, stride=rs.o), a.iters, a.warmup)
            r["kernel_vs_conv1d_form"] = r["conv1d_form_ms"] / ms
            del xp
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
        del x, out
    if a.out:
        outp = Path(a.out)
        outp.parent.mkdir(parents=True, exist_ok=True)
        outp.write_text(json.dumps(res, indent=1) + "\n")
        print(f"wrote {outp}")


if __name__ == "__main__":
    main()
