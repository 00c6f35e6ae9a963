"""Dataset preparation shared by scripts/prepare_esc50.py and scripts/prepare_urbansound8k.py: the metadata CSV
-> a list of (wav file, bundle path, label) -> ``ingest_wavs`` -> ``{"waveform": (1, T) f32, "label": int
[, "sample_rate": int]}`` bundles written with ``torch.save``, and ``dataset_stats.json``.

Planning (``plan_esc50`` / ``plan_urbansound8k``) touches only the CSV and the file system and runs anywhere; the
rest needs the GPU (``ingest._require_cuda``)."""
from __future__ import annotations

import csv
import hashlib
import json
import logging
from pathlib import Path
from typing import NamedTuple

log = logging.getLogger("prepare")


class PlanItem(NamedTuple):
    wav: Path        # the file to read
    out: Path        # the bundle to write: <out_dir>/fold_<fold - 1>/<stem>.pt
    label: int
    category: str    # the class histogram's key


def _read_csv(meta_csv: Path, columns):
    meta_csv = Path(meta_csv)
    if not meta_csv.exists():
        raise FileNotFoundError(f"{meta_csv}: the dataset's metadata table is not there")
    with meta_csv.open(newline="") as f:
        reader = csv.DictReader(f)
        missing = [c for c in columns if c not in (reader.fieldnames or [])]
        if missing:
            raise ValueError(f"{meta_csv}: missing column(s) {missing} (found {reader.fieldnames})")
        return list(reader)


def _plan(rows, wav_of, out_dir: Path, name_col: str, label_col: str, category_col: str):
    plan, missing = [], []
    for row in rows:
        fold, name = int(row["fold"]), str(row[name_col])
        wav = wav_of(row, fold, name)
        if not wav.exists():
            log.warning("%s is listed in the CSV but absent from the tree: left out", wav)
            missing.append(str(wav))
            continue
        out = Path(out_dir) / f"fold_{fold - 1}" / (Path(name).stem + ".pt")
        plan.append(PlanItem(wav, out, int(row[label_col]), str(row[category_col])))
    return plan, missing


def plan_esc50(raw_dir, out_dir):
    """``raw_dir/meta/esc50.csv`` (filename, fold 1..5, target, category) and ``raw_dir/audio/*.wav`` ->
    ``(plan, missing)``; a file the CSV names but the tree lacks is warned about and left out."""
    raw_dir = Path(raw_dir)
    rows = _read_csv(raw_dir / "meta" / "esc50.csv", ("filename", "fold", "target", "category"))
    return _plan(rows, lambda row, fold, name: raw_dir / "audio" / name, out_dir, "filename", "target", "category")


def plan_urbansound8k(raw_dir, out_dir):
    """``raw_dir/metadata/UrbanSound8K.csv`` (slice_file_name, fold 1..10, classID) and
    ``raw_dir/audio/fold<k>/*.wav`` -> ``(plan, missing)``."""
    raw_dir = Path(raw_dir)
    rows = _read_csv(raw_dir / "metadata" / "UrbanSound8K.csv", ("slice_file_name", "fold", "classID"))
    for row in rows:
        row.setdefault("class", str(row["classID"]))
    return _plan(rows, lambda row, fold, name: raw_dir / "audio" / f"fold{fold}" / name, out_dir,
                 "slice_file_name", "classID", "class")


def file_sha256(path) -> str:
    """Hex SHA-256 of a file's bytes, read through one reused 1 MiB buffer."""
    digest = hashlib.sha256()
    block = bytearray(1 << 20)
    window = memoryview(block)
    with open(path, "rb", buffering=0) as stream:
        got = stream.readinto(block)
        while got:
            digest.update(window[:got])
            got = stream.readinto(block)
    return digest.hexdigest()


def write_bundles(plan, missing, out_dir, device, target_rate=None, write_rate: bool = False, strict: bool = False,
                  validate_hash: bool = False, max_stage_bytes: int | None = None, batch_files: int = 1024) -> dict:
    """Ingest the plan's files on ``device`` and write one bundle each; -> the stats also written to
    ``out_dir/dataset_stats.json``.  ``write_rate`` adds the integer ``"sample_rate"`` key (native-rate bundles).
    The files go through ``ingest_wavs`` ``batch_files`` at a time, which bounds the host and device memory held."""
    import torch

    from .ingest import _require_cuda, ingest_wavs
    device = _require_cuda(device)
    kw = {} if max_stage_bytes is None else {"max_stage_bytes": int(max_stage_bytes)}
    stats = {"num_clips": 0, "total_duration_sec": 0.0, "class_histogram": {},
             "skipped": [{"file": m, "reason": "missing file"} for m in missing]}
    if validate_hash:
        stats["file_hashes"] = {}
    for s0 in range(0, len(plan), int(batch_files)):
        part = plan[s0:s0 + int(batch_files)]
        store, offsets, rates, skipped = ingest_wavs([it.wav for it in part], device, target_rate=target_rate,
                                                     strict=strict, **kw)
        host = store.cpu()
        reasons = {i: r for i, _, r in skipped}
        stats["skipped"] += [{"file": p, "reason": r} for _, p, r in skipped]
        for i, it in enumerate(part):
            if i in reasons:
                log.warning("Skipping %s: %s", it.wav, reasons[i])
                continue
            wave = host[offsets[i]:offsets[i + 1]].clone().view(1, -1)
            bundle = {"waveform": wave, "label": int(it.label)}
            if write_rate:
                bundle["sample_rate"] = int(rates[i])
            it.out.parent.mkdir(parents=True, exist_ok=True)
            torch.save(bundle, it.out)
            if validate_hash:
                stats["file_hashes"][it.wav.name] = file_sha256(it.wav)
            stats["num_clips"] += 1
            stats["total_duration_sec"] += wave.shape[-1] / rates[i]
            stats["class_histogram"][it.category] = stats["class_histogram"].get(it.category, 0) + 1
    Path(out_dir).mkdir(parents=True, exist_ok=True)
    with (Path(out_dir) / "dataset_stats.json").open("w") as f:
        json.dump(stats, f, indent=2)
    log.info("Finished: %d bundles in %s (%d skipped)", stats["num_clips"], out_dir, len(stats["skipped"]))
    return stats
