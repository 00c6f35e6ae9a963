"""Per-launch kernel times over the timed steps of a rocprofv3 kernel trace of bench.py.

    python tools/kernel_trace_steps.py BEFORE_kernel_trace.csv AFTER_kernel_trace.csv [--steps 5 --warmup 3] [--match pool_]

A kernel that runs k times a step appears (steps + warmup) * k times in the trace; its dispatches are taken in start
order, the warm-up steps dropped, and launch j of the step gets mean (min-max) over the timed steps.  For every
(kernel, j) present in both traces the drop of the mean is set against the larger of the two min-max spreads, the
acceptance rule of DESIGN.md section 6.  Kernels renamed between the traces are listed side by side by hand."""
import argparse
import csv
from collections import defaultdict


def per_launch(path, steps, warmup):
    rows = defaultdict(list)
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows[r["Kernel_Name"]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    out = {}
    for name, d in rows.items():
        d.sort()
        if len(d) % (steps + warmup):
            continue  # not a per-step kernel (set-up work)
        k = len(d) // (steps + warmup)
        for j in range(k):
            t = [(d[s * k + j][1] - d[s * k + j][0]) / 1e3 for s in range(warmup, warmup + steps)]
            out[(name, j)] = (sum(t) / len(t), min(t), max(t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--match", default="")
    a = ap.parse_args()
    b, c = per_launch(a.before, a.steps, a.warmup), per_launch(a.after, a.steps, a.warmup)
    for tag, d in (("before", b), ("after", c)):
        print(f"{tag}: {sum(v[0] for v in d.values()) / 1e3:.3f} ms of per-step kernel time")
    for key in sorted(set(b) | set(c), key=lambda k: -(b.get(k) or c.get(k))[0]):
        if a.match not in key[0]:
            continue
        name = key[0][:90]
        x, y = b.get(key), c.get(key)
        fmt = lambda v: f"{v[0]:8.1f} ({v[1]:.1f}-{v[2]:.1f})" if v else "       -"  # noqa: E731
        verdict = ""
        if x and y:
            spread = max(x[2] - x[1], y[2] - y[1])
            verdict = f"drop {x[0] - y[0]:7.1f} vs spread {spread:6.1f}"
        print(f"{name:90s} #{key[1]}  {fmt(x)} -> {fmt(y)}  {verdict}")


if __name__ == "__main__":
    main()
