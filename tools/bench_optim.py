"""optim.step alone for the fused optimizer family on the EnvNet-v2 parameter set (363.4 M f32 parameters), FC1's
weight gradient deferred as in training (batch 256: the update runs inside its GEMM, the bf16 operand copy is live):
Adam, AdamW, SGD with Nesterov momentum and plain SGD.  Each step is timed by the optimizer's own ``optim.step``
probe (HIP events around the clip + update launches and the deferred GEMM; the sums-only GEMM of the backward is
outside), over interleaved rounds, and set against the bytes the optimizer states and this box's streaming-copy
rate (bench.py's calibration).  One JSON line at the end.

    python tools/bench_optim.py [--rounds R] [--steps S] [--only adam,adamw,sgd,sgd-plain] [--package DIR] [--json F]

``--package`` times another checkout's package (its own libmiaudio.so), e.g. the parent commit's FusedAdam as the
yardstick, in the same call."""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
import bench  # noqa: E402  (hbm_calibration; puts this checkout's package on the path)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--only", default="adam,adamw,sgd,sgd-plain")
ap.add_argument("--package", default=None, help="package root to time instead of this checkout's")
ap.add_argument("--json", default=None, help="also write the result line to this file")
args = ap.parse_args()
if args.package:
    sys.path.insert(0, str(Path(args.package).resolve()))

import torch  # noqa: E402

from src.miaudio import kernels as K  # noqa: E402
from src.miaudio import lib as L  # noqa: E402
from src.models.envnet_v2 import EnvNetV2  # noqa: E402
from src.training import optim as O  # noqa: E402

MAKE = {
    "adam": lambda ps: O.FusedAdam(ps, lr=1e-4, weight_decay=1e-4, clip=1.0),
    "adamw": lambda ps: O.FusedAdamW(ps, lr=1e-4, weight_decay=1e-2, clip=1.0),
    "sgd": lambda ps: O.FusedSGD(ps, lr=1e-2, momentum=0.9, nesterov=True, weight_decay=5e-4, clip=1.0),
    "sgd-plain": lambda ps: O.FusedSGD(ps, lr=1e-2, weight_decay=5e-4, clip=1.0),
}
kinds = [k for k in args.only.split(",") if k]
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
calib = bench.hbm_calibration(dev)
print(f"streaming copy on this box: {calib['gbs']} GB/s", flush=True)

BATCH = 256
g = torch.Generator(device=dev).manual_seed(0)
runs = {}
for kind in kinds:
    m = EnvNetV2(num_classes=50).to(dev)
    named = dict(m.named_parameters())
    fc1 = named["classifier.1.weight"]
    Mr, Nc = fc1.shape
    runs[kind] = dict(params=list(named.values()), fc1=fc1, opt=MAKE[kind](m.parameters()),
                      grads=[None if p is fc1 else torch.randn(p.shape, generator=g, device=dev) * 1e-3
                             for p in named.values()], ms=[])
    K.bf16_shadow(fc1)
dy = (torch.randn(BATCH, Mr, generator=g, device=dev) * 0.01).to(torch.bfloat16)
x = torch.randn(BATCH, Nc, generator=g, device=dev).to(torch.bfloat16)
A, B = K.dense(dy, L.RC, BATCH, Mr), K.dense(x, L.RC, BATCH, Nc)


def step(run):
    for p, gr in zip(run["params"], run["grads"]):
        p.grad = gr  # None for FC1: its gradient is deferred
    K.defer_weight_grad(run["fc1"], A, B, Mr, Nc, BATCH, keep=(dy, x))
    run["opt"].step()
    assert run["opt"].last_deferred == 1


nbytes = {}
for r in range(args.rounds + 1):  # round 0 warms every optimizer up and is not kept
    for kind in kinds:
        K.PROBE = {"optim.step": []}
        for _ in range(args.steps):
            step(runs[kind])
        torch.cuda.synchronize()
        ev = K.PROBE["optim.step"]
        K.PROBE = None
        assert len(ev) == args.steps
        nbytes[kind] = ev[0][3]
        if r:
            runs[kind]["ms"].append(statistics.median(e0.elapsed_time(e1) for e0, e1, _, _ in ev))

nel = sum(p.numel() for p in runs[kinds[0]]["params"])
out = {"tool": "bench_optim", "package": str(Path(args.package).resolve()) if args.package else "this checkout",
       "params": nel, "batch": BATCH, "rounds": args.rounds, "steps_per_round": args.steps,
       "copy_gbs": calib["gbs"], "optim_step": {}}
for kind in kinds:
    ms = runs[kind]["ms"]
    med = statistics.median(ms)
    gbs = nbytes[kind] / (med * 1e-3) / 1e9
    out["optim_step"][kind] = {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                               "bytes": int(nbytes[kind]), "bytes_per_param": round(nbytes[kind] / nel, 2),
                               "gbs": round(gbs, 1), "frac_of_copy": round(gbs / calib["gbs"], 4)}
    print(f"{kind:10s} {med:7.3f} ms (rounds {min(ms):.3f} .. {max(ms):.3f})  {nbytes[kind] / 1e9:6.2f} GB  "
          f"{gbs:7.1f} GB/s  {gbs / calib['gbs']:.3f} of the copy rate", flush=True)
line = json.dumps(out)
print(line, flush=True)
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(line + "\n")
