"""The data path alone: clips/s of the host loader against the device-resident loader on one bundle
tree, and ``mia_crop_gather``'s GB/s beside this box's streaming-copy rate (bench.py's calibration).

A 400-clip tree of 220 500-sample bundles is written to a temporary directory (5 folds x 80 clips, 10 classes).
``ESC50DataModule`` then serves its training split (288 clips: one full batch of 256 and a partial one) three times
per configuration at B = 256, every batch brought to the device as the trainer does, the device idle at the end of
each pass: ``resident=false`` at each ``--workers`` count (persistent workers: the first pass pays their start),
then ``resident=true`` at each ``--window-lengths`` (seconds; the host passes use the first).  The resident loader's
full batch is also timed alone with HIP events (``batch_ms``: the kernel and the epoch's index and draw launches
spread over its batches), and the kernel alone through its ``crop_gather`` probe.  One JSON line at the end.

The ``fit`` leg times ``mia_fit_gather`` against ``mia_crop_gather`` at one output shape, in this
process and from one store: ``--fit-clips`` random clips with lengths uniform in [0.3 s, 4 s] at 44.1 kHz (fixed
seed), output B = ``--batch`` rows of 176 400 samples.  The yardstick is ``mia_crop_gather`` at pad 0, start 0 --
the zero-padding copy that ``mode=zero`` reproduces for clips no longer than the output.  The three launches
alternate for ``--fit-rounds`` rounds; medians and minima of their probe times, and the ratios to the yardstick.

    python tools/bench_data.py [--clips 400] [--workers 8,16] [--window-lengths 1.5,5.0] [--passes 3] [--json F]
                               [--legs host,resident,fit] [--fit-clips 512] [--fit-rounds 50]
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (hbm_calibration; puts this checkout's package on the path)

ap = argparse.ArgumentParser()
ap.add_argument("--clips", type=int, default=400)
ap.add_argument("--samples", type=int, default=220_500)
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--workers", default="8,16")
ap.add_argument("--window-lengths", default="1.5,5.0")
ap.add_argument("--passes", type=int, default=3)
ap.add_argument("--steps", type=int, default=20, help="timed launches of one full batch / of the kernel")
ap.add_argument("--legs", default="host,resident,fit", help="which of host, resident, fit to run")
ap.add_argument("--fit-clips", type=int, default=512)
ap.add_argument("--fit-rounds", type=int, default=50)
ap.add_argument("--json", default=None, help="also write the result line to this file")
args = ap.parse_args()

import torch  # noqa: E402

from src.datasets.esc50 import ESC50DataModule  # noqa: E402
from src.miaudio import kernels as K  # noqa: E402
from src.training.lite import _to  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
calib = bench.hbm_calibration(dev)
print(f"streaming copy on this box: {calib['gbs']} GB/s", flush=True)
windows = [float(w) for w in args.window_lengths.split(",")]
legs = set(args.legs.split(","))
if not legs <= {"host", "resident", "fit"}:
    ap.error(f"--legs {args.legs}: host, resident and fit are the legs")


def write_tree(root: Path):
    per = args.clips // 5
    for f in range(5):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(per):
            g = torch.Generator().manual_seed(1000 * f + i)
            w = 0.1 * torch.randn(1, args.samples, generator=g)
            torch.save({"waveform": w / w.abs().max(), "label": (f + i) % 10}, d / f"{i:03d}.pt")


def module(root, resident, workers, wl):
    dm = ESC50DataModule(root=str(root), fold=0, batch_size=args.batch, num_workers=workers, num_classes=10,
                         resident=resident, preprocessing_config={"window_length": wl})
    dm.attach(dev)
    t0 = time.perf_counter()
    dm.setup()
    torch.cuda.synchronize()
    return dm, time.perf_counter() - t0


def passes(loader):
    """Wall-clock passes over the loader, each batch on the device and the device idle at the end of the pass."""
    out = []
    for e in range(args.passes):
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(e)
        n, t0 = 0, time.perf_counter()
        for batch in loader:
            x, _ = _to(batch, dev)
            n += x.shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out.append({"clips": n, "s": round(dt, 4), "clips_per_s": round(n / dt, 1)})
    return out


def fit_leg():
    """mia_fit_gather (wrap, zero) against mia_crop_gather (pad 0, start 0) at (batch, 176 400), one store."""
    rate, length = 44_100, 176_400
    g = torch.Generator().manual_seed(2020)
    lens = torch.randint(int(0.3 * rate), 4 * rate + 1, (args.fit_clips,), generator=g)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)])
    data = torch.randn(int(offsets[-1]), device=dev, generator=torch.Generator(device=dev).manual_seed(2021))
    offs = offsets.to(dev)
    idx = torch.randperm(args.fit_clips, generator=g)[:args.batch].repeat(-(-args.batch // args.fit_clips))
    idx = idx[:args.batch].to(device=dev, dtype=torch.int32).contiguous()
    zero = torch.zeros_like(idx)
    out = torch.empty(args.batch, length, device=dev)
    runs = {"crop_gather": lambda: K.crop_gather(data, offs, idx, zero, 0, length, out=out.view(1, *out.shape)),
            "fit_wrap": lambda: K.fit_gather(data, offs, idx, length, "wrap", out=out),
            "fit_zero": lambda: K.fit_gather(data, offs, idx, length, "zero", out=out)}
    zero_bits = runs["fit_zero"]().clone().view(torch.int32).view(-1)
    same = torch.equal(zero_bits, runs["crop_gather"]().view(torch.int32).view(-1))
    if not same:
        raise RuntimeError("fit leg: mia_fit_gather(mode=zero) and mia_crop_gather(pad 0, start 0) differ")
    times = {k: [] for k in runs}
    for r in range(args.fit_rounds + 3):  # alternating launches; the first three rounds warm
        for name, fn in runs.items():
            tag = "crop_gather" if name == "crop_gather" else "fit_gather"
            K.PROBE = {tag: []}
            fn()
            ev, K.PROBE = K.PROBE[tag], None
            if r >= 3:
                times[name].append(ev[0])
    torch.cuda.synchronize()
    nbytes = 8.0 * out.numel()
    leg = {"clips": args.fit_clips, "batch": args.batch, "length": length, "bytes": int(nbytes),
           "clip_seconds": [0.3, 4.0], "store_mib": round(data.numel() * 4 / 2 ** 20, 1),
           "zero_equals_crop_gather": bool(same), "rounds": args.fit_rounds}
    for name, evs in times.items():
        ms = [e0.elapsed_time(e1) for e0, e1, _, _ in evs]
        med = statistics.median(ms)
        leg[name] = {"ms": round(med, 4), "min_ms": round(min(ms), 4), "gbs": round(nbytes / (med * 1e-3) / 1e9, 1),
                     "frac_of_copy": round(nbytes / (med * 1e-3) / 1e9 / calib["gbs"], 4)}
    for name in ("fit_wrap", "fit_zero"):
        leg[name]["ratio_to_crop_gather"] = round(leg[name]["ms"] / leg["crop_gather"]["ms"], 4)
    return leg


res = {"tool": "bench_data", "clips": args.clips, "samples": args.samples, "batch": args.batch,
       "copy_gbs": calib["gbs"], "host": {}, "resident": {}, "kernel": {}}
if "fit" in legs:
    res["fit"] = fit_leg()
    print(f"fit gather: {res['fit']}", flush=True)
with tempfile.TemporaryDirectory() as tmp:
    root = Path(tmp) / "tree"
    if legs & {"host", "resident"}:
        write_tree(root)
    for workers in (int(w) for w in args.workers.split(",") if "host" in legs):
        dm, setup_s = module(root, False, workers, windows[0])
        loader = dm.train_dataloader()
        res["host"][f"workers_{workers}"] = {"setup_s": round(setup_s, 3), "window_length": windows[0],
                                             "passes": passes(loader)}
        print(f"host, {workers} workers: {res['host'][f'workers_{workers}']}", flush=True)
        del loader, dm
    for wl in windows if "resident" in legs else ():
        dm, setup_s = module(root, True, 0, wl)
        loader = dm.train_dataloader()
        entry = {"setup_s": round(setup_s, 3), "window": loader.window, "passes": passes(loader)}
        # one full batch alone: HIP events around whole passes, over the number of full-batch equivalents in them
        per_pass = len(loader.clip) / args.batch
        for _ in loader:  # warm
            pass
        ms = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in loader:
                pass
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / per_pass)
        entry["batch_ms"] = round(statistics.median(ms), 4)
        # the kernel alone on the loader's own store, one full batch
        st = dm._rstore
        idx = loader.clip[:args.batch].repeat(-(-args.batch // len(loader.clip)))[:args.batch].contiguous()
        start = torch.arange(args.batch, dtype=torch.int32, device=dev) * 7 + 1  # every alignment mod 4
        out = torch.empty(1, args.batch, loader.window, device=dev)
        K.PROBE = {"crop_gather": []}
        for _ in range(args.steps + 2):
            K.crop_gather(st.data, st.offsets, idx, start, loader.pad, loader.window, out=out)
        torch.cuda.synchronize()
        ev, K.PROBE = K.PROBE["crop_gather"][2:], None
        kms = statistics.median(e0.elapsed_time(e1) for e0, e1, _, _ in ev)
        gbs = ev[0][3] / (kms * 1e-3) / 1e9
        res["kernel"][f"window_{loader.window}"] = {"ms": round(kms, 4), "bytes": int(ev[0][3]), "gbs": round(gbs, 1),
                                                   "frac_of_copy": round(gbs / calib["gbs"], 4)}
        res["resident"][f"window_{loader.window}"] = entry
        print(f"resident, window {loader.window}: {entry}\n  kernel: {res['kernel'][f'window_{loader.window}']}",
              flush=True)
        del loader, dm, st, out
line = json.dumps(res)
print(line, flush=True)
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(line + "\n")
