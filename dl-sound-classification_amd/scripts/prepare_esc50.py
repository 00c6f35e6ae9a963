#!/usr/bin/env python
"""Prepare ESC-50 for training -- drop-in for the reference scripts/prepare_esc50.py (same layout, same
``--no-hash``), without torchaudio or pandas: the containers are parsed in Python (src/datasets/wav.py) and the
samples are decoded, downmixed, resampled to 44.1 kHz and peak-normalised on the GPU (src/datasets/ingest.py).

    $DATA_DIR/raw/esc50/{meta/esc50.csv, audio/*.wav}  ->  $DATA_DIR/processed/esc50/fold_{fold-1}/{name}.pt
                                                            $DATA_DIR/processed/esc50/dataset_stats.json

    DATA_DIR=/data python scripts/prepare_esc50.py --no-hash

Each bundle is ``{"waveform": (1, T) f32 CPU tensor, peak-normalised, "label": int}``.  A file the CSV names but
the tree lacks is warned about and skipped; so is a file the parser rejects or a clip with NaN / Inf samples
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

from src.datasets.prepare import plan_esc50, write_bundles  # noqa: E402

ESC50_RATE = 44_100  # the rate ESC-50 is published at, and the one every bundle is written at


def prepare_esc50(data_dir=None, validate_hash: bool = True, device="cuda:0", strict: bool = False) -> dict:
    data_dir = Path(data_dir if data_dir is not None else os.getenv("DATA_DIR", "data"))
    raw_dir, out_dir = data_dir / "raw" / "esc50", data_dir / "processed" / "esc50"
    plan, missing = plan_esc50(raw_dir, out_dir)
    return write_bundles(plan, missing, out_dir, device, target_rate=ESC50_RATE, strict=strict,
                         validate_hash=validate_hash)


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO, format="[%(levelname)s %(name)s] %(message)s")
    parser = argparse.ArgumentParser(description="ESC-50 .wav files + meta/esc50.csv -> per-fold bundle files (GPU).")
    parser.add_argument("--no-hash", action="store_true",
                        help="Leave the per-file SHA-256 digests out of dataset_stats.json.")
    parser.add_argument("--data-dir", default=None, help="Overrides $DATA_DIR (default: data).")
    parser.add_argument("--device", default="cuda:0")
    parser.add_argument("--strict", action="store_true", help="Raise on a file that would be skipped.")
    args = parser.parse_args()
    prepare_esc50(args.data_dir, validate_hash=not args.no_hash, device=args.device, strict=args.strict)
