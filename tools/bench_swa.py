"""The two stochastic-weight-averaging passes alone on the EnvNet-v2 parameter set (363.4 M f32 parameters, FC1's
bf16 operand copy live as in training): K.swa_update (first sample: 8 B per parameter; later ones: 12 B) and
K.swa_transfer (8 B, + 2 B where shadowed), timed by their own ``swa.update`` / ``swa.transfer`` probes over
interleaved rounds.  Beside them, in the same process and on the same tensors: torch's multi-tensor lerp
(``torch._foreach_lerp_(avg, params, 1 / (n + 1))``, what AveragedModel.update_parameters runs: the path the kernel
replaces, 12 B per parameter), torch's multi-tensor copy (``torch._foreach_copy_``, the transfer it replaces) and one
flat device copy of the parameters' bytes (8 B per parameter), all set against this box's streaming-copy rate
(bench.py's calibration).  One JSON line at the end.

    python tools/bench_swa.py [--rounds R] [--steps S] [--json F] [--grids 8192,2048]
"""
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
ap.add_argument("--json", default=None, help="also write the result line to this file")
ap.add_argument("--grids", default=None, help="comma-separated blocks per tensor to also time mia_swa_update at")
args = ap.parse_args()

import torch  # noqa: E402

from src.miaudio import kernels as K  # noqa: E402
from src.models.envnet_v2 import EnvNetV2  # noqa: E402

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
calib = bench.hbm_calibration(dev)
print(f"streaming copy on this box: {calib['gbs']} GB/s", flush=True)

m = EnvNetV2(num_classes=50).to(dev)
params = list(m.parameters())
fc1 = dict(m.named_parameters())["classifier.1.weight"]
K.bf16_shadow(fc1)  # live, as after any bf16 training step
avg = [torch.randn_like(p) for p in params]
nel = sum(p.numel() for p in params)
flat_src = torch.randn(nel, device=dev)
flat_dst = torch.empty_like(flat_src)
raw = [p.detach() for p in params]


def probed(tag, fn):
    def run():
        K.PROBE = {tag: []}
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        ev, K.PROBE = K.PROBE[tag], None
        assert len(ev) == args.steps
        return [e0.elapsed_time(e1) for e0, e1, _, _ in ev], ev[0][3]
    return run


def evented(nbytes, fn):
    def run():
        ev = []
        for _ in range(args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        return [e0.elapsed_time(e1) for e0, e1 in ev], nbytes
    return run


with torch.no_grad():
    CASES = {
        "swa_update_first": probed("swa.update", lambda: K.swa_update(avg, params, 0)),
        "swa_update": probed("swa.update", lambda: K.swa_update(avg, params, 7)),
        # (torch's copy below moves FC1's version: the operand copy is made live again outside the probe)
        "swa_transfer": probed("swa.transfer", lambda: (K.bf16_shadow(fc1), K.swa_transfer(params, avg))),
        "torch_foreach_lerp": evented(12 * nel, lambda: torch._foreach_lerp_(avg, raw, 1.0 / 8.0)),
        "torch_foreach_copy": evented(8 * nel, lambda: torch._foreach_copy_(raw, avg)),
        # the whole torch-side transfer: the copy, then the recast of FC1's operand copy it made stale
        "torch_copy_and_recast": evented(8 * nel + 6 * fc1.numel(),
                                         lambda: (torch._foreach_copy_(raw, avg), K.bf16_shadow(fc1))),
        "flat_copy": evented(8 * nel, lambda: flat_dst.copy_(flat_src)),
    }
    if args.grids:
        # the update pass launched with a smaller max_numel (fewer blocks per tensor; the walker strides over the
        # rest): how much of the time is the 47 small tensors' idle blocks
        from src.miaudio import lib as L
        sizes = [p.numel() for p in params]
        table = K._swa_table("update", [[a.data_ptr() for a in avg], [p.data_ptr() for p in params], sizes], dev)
        for blocks in (int(b) for b in args.grids.split(",")):
            CASES[f"swa_update_{blocks}_blocks"] = evented(12 * nel, lambda blocks=blocks: L.check(
                L.load().mia_swa_update(table[0].data_ptr(), table[1].data_ptr(), table[2].data_ptr(), len(params),
                                        blocks * 8192, 7, L.stream_ptr()), "mia_swa_update"))
    ms = {k: [] for k in CASES}
    nbytes = {}
    for r in range(args.rounds + 1):  # round 0 warms everything up and is not kept
        for name, run in CASES.items():
            t, nbytes[name] = run()
            if r:
                ms[name].append(statistics.median(t))

out = {"tool": "bench_swa", "params": nel, "rounds": args.rounds, "steps_per_round": args.steps,
       "copy_gbs": calib["gbs"], "passes": {}}
for name in CASES:
    med = statistics.median(ms[name])
    gbs = nbytes[name] / (med * 1e-3) / 1e9
    out["passes"][name] = {"ms": round(med, 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                           "bytes": int(nbytes[name]), "bytes_per_param": round(nbytes[name] / nel, 2),
                           "gbs": round(gbs, 1), "frac_of_copy": round(gbs / calib["gbs"], 4)}
    print(f"{name:20s} {med:7.3f} ms (rounds {min(ms[name]):.3f} .. {max(ms[name]):.3f})  {nbytes[name] / 1e9:6.2f} GB  "
          f"{gbs:7.1f} GB/s  {gbs / calib['gbs']:.3f} of the copy rate", flush=True)
line = json.dumps(out)
print(line, flush=True)
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(line + "\n")
