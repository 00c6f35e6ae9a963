"""WAV ingestion alone: a synthetic tree of mixed-format .wav files through the host parser, the
staging read, ``mia_pcm_decode``, ``mia_clip_peak`` and ``mia_clip_scale``, beside this box's streaming-copy rate
(bench.py's calibration) and the numpy restatement of the same work on the host (tests/_wav_ref.py).

``--clips`` files of ``--samples`` frames at 44.1 kHz are written to a temporary directory, the six sample formats
in turn, every other file stereo.  Reported: parse + read wall time (files already in the page cache), the decode
launch over the whole tree and over ``--format-clips`` clips of each format alone (HIP-event medians through the
``pcm_decode`` probe; GB/s = file bytes + 4 B per output sample over the time), the peak and scale passes, one
``ingest_wavs`` call end to end, and the numpy time.  One JSON line at the end.

    python tools/bench_ingest.py [--clips 480] [--samples 220500] [--steps 20] [--json profiles/ingest_bench.json]
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
ap.add_argument("--clips", type=int, default=480)
ap.add_argument("--format-clips", type=int, default=320, help="clips of the per-format decode launches")
ap.add_argument("--samples", type=int, default=220_500)
ap.add_argument("--steps", type=int, default=20, help="timed launches of each kernel")
ap.add_argument("--json", default=None, help="also write the result line to this file")
args = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.datasets.ingest import ingest_wavs, plan_groups  # noqa: E402
from src.datasets.wav import parse_wav  # noqa: E402
from src.miaudio import kernels as K  # noqa: E402
from tests import _wav_ref as R  # noqa: E402  (the writers and the numpy restatement)

dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
calib = bench.hbm_calibration(dev)
print(f"streaming copy on this box: {calib['gbs']} GB/s", flush=True)


def probe_ms(tag, fn):
    """Median HIP-event time of ``fn`` through its kernels.probe, and the algorithmic bytes it reports."""
    K.PROBE = {tag: []}
    for _ in range(args.steps + 2):
        fn()
    torch.cuda.synchronize()
    ev, K.PROBE = K.PROBE[tag][2:], None
    return statistics.median(e0.elapsed_time(e1) for e0, e1, _, _ in ev), ev[0][3]


def rate(ms, nbytes):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"ms": round(ms, 4), "bytes": int(nbytes), "gbs": round(gbs, 1), "frac_of_copy": round(gbs / calib["gbs"], 4)}


res = {"tool": "bench_ingest", "clips": args.clips, "samples": args.samples, "copy_gbs": calib["gbs"]}
with tempfile.TemporaryDirectory() as tmp:
    paths, meta = [], []
    for k in range(args.clips):
        fmt, channels = k % 6, 1 + (k // 6) % 2
        raw = R.random_raw(fmt, args.samples, channels, seed=k)
        p = Path(tmp) / f"{k:04d}.wav"
        (R.write_pcm if fmt <= R.S32 else R.write_any)(p, raw, fmt, channels, 44_100)
        paths.append(p)
        meta.append((fmt, channels))

    # ---- host: parse every header, read every data chunk into one pinned buffer
    t0 = time.perf_counter()
    infos = [parse_wav(p) for p in paths]
    t_parse = time.perf_counter() - t0
    (ids, offs, used), = plan_groups([i.data_bytes for i in infos], 1 << 62)
    pinned = torch.empty(used, dtype=torch.uint8, pin_memory=True)
    view = memoryview(pinned.numpy())
    t0 = time.perf_counter()
    for info, off, p in zip(infos, offs, paths):
        with open(p, "rb") as f:
            f.seek(info.data_offset)
            f.readinto(view[off:off + info.data_bytes])
    t_read = time.perf_counter() - t0
    file_bytes = sum(i.data_bytes for i in infos)
    res["host"] = {"parse_s": round(t_parse, 4), "read_s": round(t_read, 4), "file_mb": round(file_bytes / 1e6, 1),
                   "read_gbs": round(file_bytes / t_read / 1e9, 2)}
    print(f"host: {res['host']}", flush=True)

    # ---- device: decode (all formats in one launch, then each format alone), peak, scale
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    stage = pinned.to(dev, non_blocking=True)
    e1.record()
    torch.cuda.synchronize()
    res["upload"] = {"ms": round(e0.elapsed_time(e1), 3), "gbs": round(used / e0.elapsed_time(e1) / 1e6, 1)}
    out_offs = [0]
    for i in infos:
        out_offs.append(out_offs[-1] + i.frames)
    store = torch.empty(out_offs[-1], dtype=torch.float32, device=dev)
    table = [(off, i.frames, i.channels, i.device_format) for off, i in zip(offs, infos)]
    ms, nb = probe_ms("pcm_decode", lambda: K.pcm_decode(stage, table, out_offs[:-1], store))
    res["decode"] = {"all": rate(ms, nb)}
    # each format alone: --format-clips copies of one clip of that format, enough bytes to leave the last-level cache
    for fmt in range(6):
        for channels in (1, 2):
            raw = np.frombuffer(R.random_raw(fmt, args.samples, channels, seed=fmt), np.uint8)
            nb = -(-raw.size // 16) * 16
            one = torch.zeros(nb, dtype=torch.uint8)
            one[:raw.size] = torch.from_numpy(raw.copy())
            buf = one.to(dev).repeat(args.format_clips)
            tab = [(k * nb, args.samples, channels, fmt) for k in range(args.format_clips)]
            oo = [k * args.samples for k in range(args.format_clips)]
            dst = torch.empty(args.format_clips * args.samples, dtype=torch.float32, device=dev)
            ms, nbytes = probe_ms("pcm_decode", lambda: K.pcm_decode(buf, tab, oo, dst))
            res["decode"][f"{R.NAMES[fmt]}_x{channels}"] = rate(ms, nbytes)
            del buf, dst
    print(f"decode: {res['decode']}", flush=True)
    peak, _ = K.pcm_decode(stage, table, out_offs[:-1], store)
    off_dev = torch.tensor(out_offs, dtype=torch.int64, device=dev)
    res["peak"] = rate(*probe_ms("clip_peak", lambda: K.clip_peak(store, off_dev)))
    res["scale"] = rate(*probe_ms("clip_scale", lambda: K.clip_scale(store, off_dev, peak)))
    print(f"peak: {res['peak']}\nscale: {res['scale']}", flush=True)
    del stage, store, pinned, view

    # ---- end to end, and the same work in numpy on this host
    ingest_wavs(paths[:6], dev)  # warm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    store, offsets, _, skipped = ingest_wavs(paths, dev)
    torch.cuda.synchronize()
    res["ingest_wavs_s"] = round(time.perf_counter() - t0, 4)
    assert not skipped
    t0 = time.perf_counter()
    refs = []
    for p, info, (fmt, channels) in zip(paths, infos, meta):
        with open(p, "rb") as f:
            f.seek(info.data_offset)
            refs.append(R.ingest(f.read(info.data_bytes), fmt, channels))
    res["numpy_s"] = round(time.perf_counter() - t0, 4)
    host = store.cpu().numpy()
    res["bit_exact_vs_numpy"] = all(np.array_equal(host[offsets[k]:offsets[k + 1]], r) for k, r in enumerate(refs))
    print(f"ingest_wavs: {res['ingest_wavs_s']} s, numpy: {res['numpy_s']} s, "
          f"bit-exact: {res['bit_exact_vs_numpy']}", flush=True)
line = json.dumps(res)
print(line, flush=True)
if args.json:
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    Path(args.json).write_text(line + "\n")
