"""CPU: the device-resident dataset's host-side rules (src/datasets/resident.py, include/miaudio_data.h).

ABI sync of the new header, the crop-start rules against the oracle's restatement of the reference
(oracle.data.envnet_random_crop / envnet_multi_crop), the training draw's distribution, the epoch order against
DistributedSampler itself, the config pass-through and the CPU-device error."""
import importlib.util
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from oracle import data as odata

REPO = Path(__file__).resolve().parents[1]
PKG = REPO / "dl-sound-classification_amd"

WL, SR = 0.1, 44_100
WINDOW, PAD = 4410, 2205
LENGTHS = [1000, 1001, 4410, 9000, 13230]


def declared():
    text = (REPO / "include" / "miaudio_data.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mia_[a-z0-9_]+)\s*\(", text)))


def test_data_header_abi_in_sync():
    from src.miaudio import lib as L
    names = declared()
    assert "mia_crop_gather" in names
    if not L.LIB_PATH.exists():
        pytest.fail(f"{L.LIB_PATH} missing: run `make -C dl-sound-classification_amd`")
    lib = L.load()
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, f"missing exports: {missing}"
    assert set(names) <= set(L.SIGNATURES), "ctypes signatures out of sync with the header"


def _clips():
    g = torch.Generator().manual_seed(7)
    return [torch.randn(1, n, generator=g) for n in LENGTHS]


def _cut(w, pad, start, window):
    """The kernel's rule restated with F.pad and slicing: pad each side, right-pad a short clip, slice."""
    p = F.pad(w, (pad, pad))
    if p.shape[-1] < window:
        p = F.pad(p, (0, window - p.shape[-1]))
    return p[..., start:start + window]


def test_window_matches_oracle():
    assert odata.envnet_samples(WL, 0.5, SR) == (WINDOW, PAD)


def test_center_starts_reproduce_oracle():
    from src.datasets import resident as R
    starts = R.center_starts(torch.tensor(LENGTHS), PAD, WINDOW)
    for w, s in zip(_clips(), starts.tolist()):
        ref = odata.envnet_random_crop(odata.envnet_preprocess(w, WL, 0.5, SR), False, WL, sample_rate=SR)
        assert torch.equal(_cut(w, PAD, s, WINDOW), ref)


@pytest.mark.parametrize("crops", [5, 10])
def test_multi_crop_starts_reproduce_oracle(crops):
    from src.datasets import resident as R
    starts, counts = R.multi_crop_starts(LENGTHS, PAD, WINDOW, crops)
    assert starts.shape == (len(LENGTHS), crops) and starts.dtype == torch.int32
    for w, row, cnt in zip(_clips(), starts.tolist(), counts.tolist()):
        ref = odata.envnet_multi_crop(odata.envnet_preprocess(w, WL, 0.5, SR), crops, WL, SR)
        assert cnt == len(ref)
        for c in range(cnt):
            assert torch.equal(_cut(w, PAD, row[c], WINDOW), ref[c])


def test_short_clip_starts_without_padding():
    from src.datasets import resident as R
    lens = torch.tensor([1000, 4410])
    assert R.max_starts(lens, 0, WINDOW).tolist() == [0, 0]
    assert R.center_starts(lens, 0, WINDOW).tolist() == [0, 0]
    starts, counts = R.multi_crop_starts(lens, 0, WINDOW, 5)
    assert counts.tolist() == [1, 1] and not starts.any()
    assert R.max_starts(torch.tensor(LENGTHS), PAD, WINDOW).tolist() == [n + 2 * PAD - WINDOW for n in LENGTHS]


def test_draw_is_uniform_over_the_range():
    from src.datasets import resident as R
    g = torch.Generator().manual_seed(4321)
    d = R.draw_starts(torch.full((4000,), 3, dtype=torch.int64), g)
    assert d.dtype == torch.int64 and int(d.min()) >= 0 and int(d.max()) <= 3
    counts = torch.bincount(d, minlength=4).tolist()
    print("draw counts", counts)
    assert all(abs(c - 1000) <= 150 for c in counts), counts  # 5.5 sigma of the binomial's 27.4
    assert not R.draw_starts(torch.zeros(16, dtype=torch.int64), g).any()


@pytest.mark.parametrize("shuffle", [True, False])
def test_epoch_indices_are_the_distributed_samplers(shuffle):
    from torch.utils.data.distributed import DistributedSampler

    from src.datasets import resident as R
    n = 23
    for rank in (0, 1):
        for epoch in (0, 1):
            s = DistributedSampler(list(range(n)), num_replicas=2, rank=rank, shuffle=shuffle, seed=42,
                                   drop_last=False)
            s.set_epoch(epoch)
            assert R.epoch_indices(n, 2, rank, epoch, shuffle).tolist() == list(s)


def test_epoch_indices_world_one():
    from src.datasets import resident as R
    e0, e1 = R.epoch_indices(23, 1, 0, 0, True), R.epoch_indices(23, 1, 0, 1, True)
    assert sorted(e0.tolist()) == list(range(23)) and sorted(e1.tolist()) == list(range(23))
    assert e0.tolist() != e1.tolist()
    assert R.epoch_indices(23, 1, 0, 3, False).tolist() == list(range(23))


def test_datamodule_config_passes_resident():
    from src.utils.config import compose
    spec = importlib.util.spec_from_file_location("train_script_resident", PKG / "scripts" / "train.py")
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    for ds in ("esc50", "urbansound8k"):
        off = ts.datamodule_config(compose(PKG / "configs", "training", [f"dataset={ds}"]))
        assert off["resident"] is False
        on = ts.datamodule_config(compose(PKG / "configs", "training",
                                          [f"dataset={ds}", "dataset.resident=true", "dataset.resident_max_gib=2"]))
        assert on["resident"] is True and on["resident_max_gib"] == 2


def test_resident_on_cpu_raises(tmp_path):
    from src.datasets.esc50 import ESC50DataModule
    dm = ESC50DataModule(root=str(tmp_path), resident=True)
    assert dm.resident and dm.resident_max_gib == 8.0
    dm.attach("cpu")
    with pytest.raises(ValueError, match="resident"):
        dm.setup()
    assert ESC50DataModule(root=str(tmp_path)).resident is False
