"""GPU: clip-length fitting through the data module and scripts/train.py.

* The two loader paths agree: the same ragged ESC-50-layout tree set up with ``resident=true`` (mia_fit_gather per
  batch) and with ``resident=false`` (fit_clip in the Dataset, the default collate) yields bit-identical val and
  test batches and bit-identical Mixup pools.
* End to end: ``dataset=urbansound8k model=ast`` on a tree whose clips run from 0.3 s to 1.6 s, with
  ``preprocessing_config.clip_length=1.0`` (set with ``+``: the model configs ship the key commented out), fits and
  tests on both paths with Mixup and SpecAugment on.  Without the feature the run dies in collate
  (``resident=false``) or in _ResidentLoader (``resident=true``).
* ``model=ast_mini`` on the same tree, resident, as a smoke of the small family (its patch grid takes 1 s: 276
  frames give 27 x 12 patches, inside its positional table)."""
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from src.utils.config import compose
from tests.test_fit_cpu import L, RATE, SECONDS, ragged_tree

pytestmark = pytest.mark.gpu
PKG = Path(__file__).resolve().parents[1] / "dl-sound-classification_amd"
KEY = "model.dataset_overrides.preprocessing_config"


def _script():
    spec = importlib.util.spec_from_file_location("train_script", PKG / "scripts" / "train.py")
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


def _module(root, cuda, resident, **pc):
    from src.datasets.esc50 import ESC50DataModule
    dm = ESC50DataModule(root=str(root), fold=1, sample_rate=RATE, batch_size=4, num_workers=0, is_spectrogram=True,
                         enable_mixup=True, num_classes=2, preprocessing_config=pc, resident=resident)
    dm.attach(cuda)
    dm.setup()
    return dm


@pytest.mark.parametrize("mode", ["wrap", "zero"])
def test_resident_and_host_paths_serve_the_same_bits(cuda, tmp_path, mode):
    from src.datasets.resident import _ResidentLoader
    ragged_tree(tmp_path, per_fold=12)
    res = _module(tmp_path, cuda, True, clip_length=SECONDS, clip_fit=mode)
    host = _module(tmp_path, cuda, False, clip_length=SECONDS, clip_fit=mode)
    assert min(res._rstore.lengths_host) < L < max(res._rstore.lengths_host)
    for name in ("val_dataloader", "test_dataloader"):
        a, b = getattr(res, name)(), getattr(host, name)()
        assert isinstance(a, _ResidentLoader) and a.mode == "fit" and a.window == L
        batches_a, batches_b = list(a), list(b)
        assert len(batches_a) == len(batches_b) == len(a) > 1
        for (xa, ya), (xb, yb) in zip(batches_a, batches_b):
            assert xa.is_cuda and xa.shape == xb.shape and xa.shape[1:] == (1, L)
            assert torch.equal(xa.cpu().view(torch.int32), xb.contiguous().view(torch.int32))
            assert torch.equal(ya.cpu(), yb)
    tr = res.train_dataloader()
    assert tr.mode == "fit" and sum(x.shape[0] for x, _ in tr) == len(res._train_set)
    res._pools()
    host._pools()
    assert res._pool.shape == host._pool.shape == (len(res._train_set), 128, 1 + L // 160)
    assert torch.equal(res._pool.view(torch.int32), host._pool.view(torch.int32))
    assert torch.equal(res._pool_labels, host._pool_labels)
    assert bool(torch.isfinite(res._pool).all())


def test_without_clip_length_a_ragged_tree_fails_as_before(cuda, tmp_path):
    ragged_tree(tmp_path, per_fold=12)
    res = _module(tmp_path, cuda, True)
    with pytest.raises(ValueError, match="resident AST mode serves whole clips as one"):
        res.val_dataloader()
    with pytest.raises(ValueError, match="the Mixup pool holds whole clips of one length"):
        res._pools()
    host = _module(tmp_path, cuda, False)
    with pytest.raises(ValueError, match="clip_length"):
        next(iter(host.val_dataloader()))


# ------------------------------------------------------------------------------------------ scripts/train.py
@pytest.fixture(scope="module")
def us8k_ragged(tmp_path_factory):
    """Ten folds of 12 .pt bundles at 44.1 kHz, 10 classes, clip lengths 0.3 s .. 1.6 s from a seeded generator."""
    root = tmp_path_factory.mktemp("us8k_ragged") / "us8k"
    rng = np.random.default_rng(8)
    lens = rng.integers(int(0.3 * 44_100), int(1.6 * 44_100) + 1, size=120)
    lens[0], lens[1] = int(0.3 * 44_100), int(1.6 * 44_100)
    for f in range(10):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(12):  # >= 10 clips per class: the stratified val split needs one per class
            g = torch.Generator().manual_seed(100 * f + i)
            w = 0.1 * torch.randn(1, int(lens[12 * f + i]), generator=g)
            torch.save({"waveform": w / w.abs().max(), "label": (f + i) % 10}, d / f"{i}.pt")
    return root


def _finite(out):
    assert {"test/acc", "test/f1", "test/auroc", "test/loss"} <= set(out)
    assert all(math.isfinite(v) for v in out.values()), out


def _overrides(root, tmp_path, model, resident):
    return ["dataset=urbansound8k", f"dataset.root={root}", "dataset.fold=9",
            f"dataset.resident={'true' if resident else 'false'}", f"model={model}", "trainer.precision=bf16-mixed",
            "trainer.max_epochs=1", "batch_size=8", "num_workers=0", f"+{KEY}.clip_length=1.0",
            f"checkpoint.dirpath={tmp_path}/ck", "checkpoint.monitor=val/loss", "checkpoint.mode=min"]


@pytest.mark.parametrize("resident", [True, False])
def test_train_script_ast_on_ragged_urbansound8k(cuda, us8k_ragged, tmp_path, monkeypatch, resident):
    from src.datasets.resident import _ResidentLoader
    ts = _script()
    monkeypatch.chdir(tmp_path)
    cfg = compose(PKG / "configs", "training", _overrides(us8k_ragged, tmp_path, "ast", resident) + ["+model.depth=2"])
    assert cfg.model.dataset_overrides.enable_mixup and cfg.model.dataset_overrides.augment.time_mask > 0
    _finite(ts.train(cfg))
    dm = ts.LAST_TRAINER.datamodule
    assert dm.fit_length == 44_100 and dm.clip_fit == "wrap" and dm.resident is resident
    assert dm._pool.shape == (len(dm._train_set), 128, 1 + 44_100 // 160)  # Mixup drew from the fitted clips
    loader = dm.test_dataloader()
    if resident:
        assert isinstance(loader, _ResidentLoader) and loader.mode == "fit"
        lens = dm._rstore.lengths_host
    else:
        lens = [dm._test_set.load(i)[0].shape[-1] for i in range(len(dm._test_set))]
    assert min(lens) < 44_100 < max(lens)
    x, _ = next(iter(loader))
    assert x.shape == (8, 1, 44_100)


def test_train_script_ast_mini_on_ragged_urbansound8k(cuda, us8k_ragged, tmp_path, monkeypatch):
    ts = _script()
    monkeypatch.chdir(tmp_path)
    cfg = compose(PKG / "configs", "training", _overrides(us8k_ragged, tmp_path, "ast_mini", True))
    assert cfg.model["_target_"] == "src.models.ast_mini.ASTMiniViT"
    _finite(ts.train(cfg))
    assert ts.LAST_TRAINER.datamodule.train_dataloader().mode == "fit"
