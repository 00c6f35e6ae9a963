"""CPU: the host side of GPU resampling -- the sinc taps against the float64 restatement (tests/_resample_ref.py),
the restatement's own sanity, mia_resample_out_len, the header / contract-case table of
include/miaudio_resample.h, and the data module's resampling path up to the point where it needs the device."""
import math
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import data as odata
from src.miaudio import lib as L
from tests import _resample_ref as R

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio_resample.h"
GEOMETRY = {(44100, 16000): (441, 160, 17, 475), (16000, 44100): (160, 441, 7, 174), (44100, 22050): (2, 1, 13, 28),
            (22050, 44100): (1, 2, 7, 15), (44100, 48000): (147, 160, 7, 161), (8000, 44100): (80, 441, 7, 94)}


# ------------------------------------------------------------------------------------------------ taps
@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_taps_equal_the_restatement_bit_for_bit(orig, new):
    from src.datasets.resample import sinc_resample_taps
    taps, width, o, n = sinc_resample_taps(orig, new)
    assert (o, n, width, taps.shape[1]) == GEOMETRY[(orig, new)] == R.geometry(orig, new)
    assert taps.dtype == torch.float32 and tuple(taps.shape) == (n, 2 * width + o)
    ref = R.taps32(orig, new)
    assert np.array_equal(taps.numpy().view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_restatement_resamples_a_sine(orig, new):
    """A 1 kHz sine at ``orig`` comes out as the 1 kHz sine at ``new`` (2e-3, 100 samples in from each end): a wrong
    phase order, frame stride or scale fails this; it does not rate the filter."""
    o, n, width, _ = R.geometry(orig, new)
    T = 4000
    x = np.sin(2 * np.pi * 1000.0 * np.arange(T) / orig)[None]
    out, _ = R.apply(x, R.taps64(orig, new), o, n, width)
    assert out.shape == (1, math.ceil(new * T / orig))
    want = np.sin(2 * np.pi * 1000.0 * np.arange(out.shape[1]) / new)
    err = float(np.abs(out[0] - want)[100:-100].max())
    print(f"{orig} -> {new}: max error {err:.2e}")
    assert err < 2e-3


def test_restatement_exact_and_float_forms_agree():
    rng = np.random.default_rng(0)
    x = rng.integers(-8, 9, (2, 37))
    taps = rng.integers(-3, 4, (2, 2 * 2 + 3))
    lengths = [37, 11]
    a = R.apply_exact(x, taps, 3, 2, 2, lengths)
    b, mag = R.apply(x, taps, 3, 2, 2, lengths)
    assert np.array_equal(a, b.astype(np.int64)) and np.all(mag >= np.abs(b))
    # by hand: m = f*n + j -> sum_k xz[f*o + k - width] * taps[j][k]
    xz = lambda r, i: int(x[r, i]) if 0 <= i < lengths[r] else 0  # noqa: E731
    for r in range(2):
        for m in range(a.shape[1]):
            f, j = divmod(m, 2)
            want = sum(xz(r, f * 3 + k - 2) * int(taps[j, k]) for k in range(7)) if m < -(-2 * lengths[r] // 3) else 0
            assert a[r, m] == want


# ------------------------------------------------------------------------------------------------ output length
def test_out_len_is_the_ceiling():
    lib = L.load()
    for orig, new in R.PAIRS + [(3, 2), (2, 3), (1, 1)]:
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        for T in (0, 1, 2, o - 1, o, o + 1, 2 * o + 1, 40_000, 80_000, 220_500, 2**31 + 7):
            assert lib.mia_resample_out_len(T, o, n) == -(-n * T // o) == R.out_len(T, o, n), (o, n, T)
    assert lib.mia_resample_out_len(-1, 3, 2) < 0 and lib.mia_resample_out_len(5, 0, 2) < 0
    assert lib.mia_resample_out_len(5, 3, 0) < 0


# ------------------------------------------------------------------------------------------------ header table
def _writes_caller_memory(params: str) -> bool:  # the rule of tests/test_memory_contract_table_cpu.py
    for prm in params.split(","):
        prm = " ".join(prm.split())
        if "*" not in prm:
            continue
        if prm.startswith(("const MiaEpilogue*", "const MiaPackJob*")):
            return True
        if not prm.startswith("const "):
            return True
    return False


def test_every_entry_point_of_the_resample_header_has_a_contract_case():
    from tests import test_gpu_resample_contract as T
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bint\s+(mia_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    names = {name for name, params in decls if _writes_caller_memory(params)}
    assert names == {"mia_resample"}, names
    covered = {n for covers in T.COVERS.values() for n in covers}
    assert names == covered, (sorted(names - covered), sorted(covered - names))
    every = set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", text))
    assert every == {"mia_resample", "mia_resample_out_len"}
    assert every <= set(L.SIGNATURES) and every <= L.exported_symbols()


def test_miaudio_h_does_not_declare_the_resampler():
    text = (HEADER.parent / "miaudio.h").read_text()
    assert "mia_resample" not in text


# ------------------------------------------------------------------------------------------------ data module
def _bundles(root, rate, seconds, folds=5, per_fold=2, tag=False):
    g = torch.Generator().manual_seed(7)
    files = []
    for f in range(folds):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(per_fold):
            b = {"waveform": torch.randn(1, int(rate * seconds) + 3 * i, generator=g), "label": i % 2}
            if tag:
                b["sample_rate"] = rate
            torch.save(b, d / f"clip_{f}_{i}.pt")
            files.append(d / f"clip_{f}_{i}.pt")
    return files


def test_differing_rates_on_a_cpu_device_raise(tmp_path):
    from src.datasets.esc50 import ESC50DataModule, SyntheticDataModule
    _bundles(tmp_path, 8000, 0.05)
    dm = ESC50DataModule(str(tmp_path), sample_rate=8000, num_classes=3, val_split=0.25,
                         preprocessing_config={"sample_rate": 44100, "window_length": 0.1})
    with pytest.raises(ValueError, match="resampling runs on the GPU"):
        dm.setup()
    sm = SyntheticDataModule(num_clips=10, clip_samples=800, sample_rate=16000,
                             preprocessing_config={"sample_rate": 44100})
    with pytest.raises(ValueError, match="resampling runs on the GPU"):
        sm.setup()


def test_equal_rates_build_no_store_and_keep_the_window(tmp_path):
    from src.datasets.esc50 import SR, ESC50DataModule
    _bundles(tmp_path, 8000, 0.05)
    for pc in ({"window_length": 0.1}, {"window_length": 0.1, "sample_rate": 16000}):
        dm = ESC50DataModule(str(tmp_path), sample_rate=16000, num_classes=3, val_split=0.25, preprocessing_config=pc)
        dm.setup()
        assert dm.target_rate == 16000 and dm._store is None
        for ds in (dm._train_set, dm._val_set, dm._test_set):
            assert ds.store is None and ds.window == int(0.1 * SR) and ds.pad == int(int(0.1 * SR) * 0.5)
        w, _ = dm._train_set.load(0)
        assert w.shape[-1] in (400, 403)  # the raw bundle


def test_gpu_resample_rejects_a_cpu_tensor():
    from src.datasets.resample import GpuResample
    with pytest.raises(RuntimeError, match="no CPU path"):
        GpuResample(8000, 44100)(torch.zeros(2, 100))


def test_pad_crop_and_multi_crop_with_a_store_follow_the_oracle(tmp_path):
    """A hand-made store at 16 kHz: the dataset pads, crops and multi-crops its clips in 16 kHz samples, as
    oracle.data's functions called with sample_rate=16000."""
    from src.datasets.esc50 import ESC50Dataset
    from src.datasets.resample import ResampledStore
    target, wl = 16000, 0.1  # window 1600, pad 800
    files = _bundles(tmp_path, 8000, 0.05, folds=1, per_fold=3)
    g = torch.Generator().manual_seed(3)
    lens = [700, 1600, 2500]  # a raw clip below, at and above the window
    clips = [torch.randn(n, generator=g) for n in lens]
    offs = [0, 700, 2300, 4800]
    store = ResampledStore(files, torch.cat(clips), offs, [2, 0, 1], target)
    kw = dict(files=files, window_length=wl, sample_rate=target, store=store)
    window, pad = odata.envnet_samples(wl, 0.5, target)
    for i, clip in enumerate(clips):
        w = clip.view(1, -1)
        ds = ESC50Dataset(tmp_path, pad_crop=True, training=False, **kw)
        assert (ds.window, ds.pad) == (window, pad) == (1600, 800)
        got, label = ds[i]
        assert label == [2, 0, 1][i] and torch.equal(ds.load(i)[0], w)
        padded = odata.envnet_preprocess(w, wl, 0.5, target)
        assert torch.equal(got, odata.envnet_random_crop(padded, False, wl, sample_rate=target))
        random.seed(11)
        got, _ = ESC50Dataset(tmp_path, pad_crop=True, training=True, **kw)[i]
        assert torch.equal(got, odata.envnet_random_crop(padded, True, wl, rng=random.Random(11), sample_rate=target))
        crops, _ = ESC50Dataset(tmp_path, pad_crop=True, training=False, multi_crop_test=True, test_crops=4, **kw)[i]
        want = odata.envnet_multi_crop(padded, 4, wl, sample_rate=target)
        crops = crops if isinstance(crops, list) else [crops]
        assert len(crops) == len(want) and all(torch.equal(a, b) for a, b in zip(crops, want))
        # the BC-mixing path: no padding, the crop alone
        got, _ = ESC50Dataset(tmp_path, pad_crop=False, training=False, **kw)[i]
        assert torch.equal(got, odata.envnet_random_crop(w, False, wl, sample_rate=target))
