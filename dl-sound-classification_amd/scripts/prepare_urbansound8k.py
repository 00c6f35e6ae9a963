#!/usr/bin/env python
"""Prepare UrbanSound8K for training (the reference has no such step).

    $DATA_DIR/raw/urbansound8k/{metadata/UrbanSound8K.csv, audio/fold{1..10}/*.wav}
        ->  $DATA_DIR/processed/urbansound8k/fold_{fold-1}/{stem}.pt  and  dataset_stats.json

    DATA_DIR=/data python scripts/prepare_urbansound8k.py                      # native-rate bundles
    DATA_DIR=/data python scripts/prepare_urbansound8k.py --target-rate 44100  # bundles already at 44.1 kHz

By default each bundle keeps its clip's own rate: ``{"waveform": (1, T) f32, "label": int, "sample_rate": int}``,
peak-normalised at that rate, the form src/datasets/urbansound8k.py documents; ``UrbanSound8KDataModule.setup()``
then resamples once on the GPU.  ``--target-rate R`` resamples here and writes bundles at R without the key.
The dataset mixes 8/16/24/32-bit PCM, float and extensible headers, mono and stereo, 8 to 192 kHz; files in a
format outside src/datasets/wav.py's list (ADPCM, ...) are skipped with their reason in dataset_stats.json
(``--strict`` raises instead).  Needs a GPU: there is no CPU path.
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from src.datasets.prepare import plan_urbansound8k, write_bundles  # noqa: E402


def prepare_urbansound8k(data_dir=None, target_rate: int | None = None, validate_hash: bool = False,
                         device="cuda:0", strict: bool = False) -> dict:
    data_dir = Path(data_dir if data_dir is not None else os.getenv("DATA_DIR", "data"))
    raw_dir, out_dir = data_dir / "raw" / "urbansound8k", data_dir / "processed" / "urbansound8k"
    plan, missing = plan_urbansound8k(raw_dir, out_dir)
    return write_bundles(plan, missing, out_dir, device, target_rate=target_rate, write_rate=target_rate is None,
                         strict=strict, validate_hash=validate_hash)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="[%(levelname)s %(name)s] %(message)s")
    parser = argparse.ArgumentParser(
        description="UrbanSound8K .wav files + metadata/UrbanSound8K.csv -> per-fold bundle files (GPU).")
    parser.add_argument("--target-rate", type=int, default=None, help="Resample to this rate (default: keep native).")
    parser.add_argument("--hash", action="store_true", help="Record SHA-256 of every file.")
    parser.add_argument("--data-dir", default=None, help="Overrides $DATA_DIR (default: data).")
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--strict", action="store_true", help="Raise on a file that would be skipped.")
    args = parser.parse_args()
    prepare_urbansound8k(args.data_dir, args.target_rate, validate_hash=args.hash, device=args.device,
                         strict=args.strict)
