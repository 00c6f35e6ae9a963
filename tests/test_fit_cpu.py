"""CPU: clip-length fitting on the host path (src/datasets/esc50.py::fit_clip).

fit_clip against the reference's src/utils/audio.py::pad_or_trim (tests/golden/golden_fit.npz, written by
tests/golden/make_golden_fit.py) and against the numpy restatement in tests/_fit_ref.py (both modes, the empty clip,
bit patterns); an ESC50DataModule over a ragged tree set up on the CPU with ``clip_length``; the configuration
errors; the shipped configs leave the key unset.  Every comparison is on the int32 view of the floats."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests._fit_ref import MODES, fit_ref

REPO = Path(__file__).resolve().parents[1]
PKG = REPO / "dl-sound-classification_amd"

NS = (1, 2, 3, 4, 5, 7, 11, 64, 129)
LS = (1, 4, 5, 64)
RATE, SECONDS = 8000, 0.1
L = int(SECONDS * RATE)  # 800 samples, above the log-mel kernel's 513


@pytest.fixture(scope="module")
def golden_fit():
    return dict(np.load(REPO / "tests" / "golden" / "golden_fit.npz", allow_pickle=False))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _fit(x: np.ndarray, length: int, mode: str) -> np.ndarray:
    from src.datasets.esc50 import fit_clip
    out = fit_clip(torch.from_numpy(x.copy())[None], length, mode)
    assert out.shape == (1, length) and out.dtype == torch.float32
    return out[0].contiguous().numpy()


def test_golden_covers_every_case(golden_fit):
    assert tuple(golden_fit["ns"]) == NS and tuple(golden_fit["ls"]) == LS
    assert len(golden_fit) == 2 + 3 * len(NS) * len(LS)


@pytest.mark.parametrize("n", NS)
def test_fit_clip_wrap_equals_reference_pad_or_trim(golden_fit, n):
    for length in LS:
        pre = f"n{n}_L{length}__"
        got = _fit(np.arange(n, dtype=np.float32), length, "wrap")
        assert np.array_equal(_bits(got), _bits(golden_fit[pre + "arange_out"])), (n, length)
        got = _fit(golden_fit[pre + "rand_in"], length, "wrap")
        assert np.array_equal(_bits(got), _bits(golden_fit[pre + "rand_out"])), (n, length)


def test_issue_examples():
    assert _fit(np.arange(3, dtype=np.float32), 10, "wrap").tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    assert _fit(np.arange(7, dtype=np.float32), 5, "wrap").tolist() == [1, 2, 3, 4, 5]
    assert _fit(np.arange(11, dtype=np.float32), 5, "zero").tolist() == [3, 4, 5, 6, 7]
    assert _fit(np.arange(3, dtype=np.float32), 5, "zero").tolist() == [0, 1, 2, 0, 0]


@pytest.mark.parametrize("mode", MODES)
def test_fit_clip_equals_numpy_restatement(mode):
    rng = np.random.default_rng(5)
    for n in (0,) + NS + (799, 800, 801, 1841):
        for length in LS + (800, 1031):
            x = rng.standard_normal(n).astype(np.float32)
            if n >= 4:  # a signalling NaN with a payload, -0.0, +inf and a denormal: copied, never computed with
                x.view(np.uint32)[:4] = [0x7FA12345, 0x80000000, 0x7F800000, 0x00000001]
            got = _fit(x, length, mode)
            assert np.array_equal(_bits(got), _bits(fit_ref(x, length, mode))), (n, length)
            if n == 0:
                assert not _bits(got).any()  # +0.0, sign bit clear


def test_fit_clip_rejects_bad_arguments():
    from src.datasets.esc50 import fit_clip
    with pytest.raises(ValueError, match="mode"):
        fit_clip(torch.zeros(1, 4), 4, "reflect")
    with pytest.raises(ValueError, match="length"):
        fit_clip(torch.zeros(1, 4), 0)


# ------------------------------------------------------------------------------------------ the data module
def ragged_tree(root: Path, folds: int = 5, per_fold: int = 6, length: int = L, classes: int = 2, seed: int = 0):
    """ESC-50 layout with clip lengths spread over 0.4 .. 2.3 of ``length`` (both ends, ``length`` itself and its
    neighbours included) -> {path: (1, n) waveform}."""
    rng = np.random.default_rng(seed)
    fixed = [int(0.4 * length), int(2.3 * length), length, length - 1, length + 1, length + 2]
    files, k = {}, 0
    for f in range(folds):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(per_fold):
            n = fixed[k] if k < len(fixed) else int(rng.integers(int(0.4 * length), int(2.3 * length) + 1))
            g = torch.Generator().manual_seed(1000 * f + i)
            w = torch.randn(1, n, generator=g)
            w = w / w.abs().max()
            torch.save({"waveform": w, "label": (f + i) % classes}, d / f"{i}.pt")
            files[str(d / f"{i}.pt")] = w
            k += 1
    return files


def _module(root, **pc):
    from src.datasets.esc50 import ESC50DataModule
    return ESC50DataModule(root=str(root), fold=1, sample_rate=RATE, batch_size=4, num_workers=0,
                           is_spectrogram=True, enable_mixup=True, num_classes=2, preprocessing_config=pc)


@pytest.mark.parametrize("mode", MODES)
def test_datamodule_on_a_ragged_tree_serves_fitted_batches(tmp_path, mode):
    files = ragged_tree(tmp_path)
    lens = sorted(w.shape[-1] for w in files.values())
    assert lens[0] == int(0.4 * L) and lens[-1] == int(2.3 * L)
    dm = _module(tmp_path, clip_length=SECONDS, clip_fit=mode)
    assert dm.fit_length == L and dm.clip_fit == mode
    dm.attach("cpu")
    dm.setup()
    for ds, loader in ((dm._val_set, dm.val_dataloader()), (dm._test_set, dm.test_dataloader()),
                       (dm._train_set, dm.train_dataloader())):
        order, seen = [str(f) for f in ds.files], 0
        for x, y in loader:
            assert x.shape[1:] == (1, L) and x.dtype == torch.float32 and y.shape == (x.shape[0],)
            if ds.training:  # shuffled: the shapes are the check
                seen += x.shape[0]
                continue
            for r in range(x.shape[0]):
                ref = fit_ref(files[order[seen + r]][0].numpy(), L, mode)
                assert np.array_equal(_bits(x[r, 0].numpy()), _bits(ref))
            seen += x.shape[0]
        assert seen == len(ds)
    # what the Mixup pool stacks on the host path
    w, _ = dm._train_set.clip(0)
    assert w.shape == (1, L)
    assert np.array_equal(_bits(w[0].numpy()), _bits(fit_ref(files[str(dm._train_set.files[0])][0].numpy(), L, mode)))


def test_ragged_batch_without_clip_length_names_the_key(tmp_path):
    ragged_tree(tmp_path)
    dm = _module(tmp_path)
    assert dm.fit_length is None
    dm.attach("cpu")
    dm.setup()
    with pytest.raises(ValueError, match="clip_length"):
        next(iter(dm.val_dataloader()))


def test_equal_length_clips_without_clip_length_still_stack(tmp_path):
    ragged_tree(tmp_path, length=600)
    for f in tmp_path.glob("fold_*/*.pt"):
        b = torch.load(f, weights_only=True)
        torch.save({"waveform": b["waveform"][:, :240], "label": b["label"]}, f)
    dm = _module(tmp_path)
    dm.attach("cpu")
    dm.setup()
    x, y = next(iter(dm.val_dataloader()))
    assert x.shape[1:] == (1, 240)


@pytest.mark.parametrize("samples", [1000, 500])
def test_synthetic_module_fits_its_clips_once(samples):
    from src.datasets.esc50 import SyntheticDataModule
    kw = dict(num_clips=20, clip_samples=samples, sample_rate=RATE, is_spectrogram=True, num_classes=2)
    whole = SyntheticDataModule(**kw)
    fitted = SyntheticDataModule(preprocessing_config={"clip_length": SECONDS}, **kw)
    for dm in (whole, fitted):
        dm.attach("cpu")
        dm.setup()
    for (xw, yw), (xf, yf) in ((whole._train_set, fitted._train_set), (whole._test_set, fitted._test_set)):
        assert xw.shape[1:] == (1, samples) and xf.shape[1:] == (1, L) and torch.equal(yw, yf)
        for r in range(xw.shape[0]):
            assert np.array_equal(_bits(xf[r, 0].numpy()), _bits(fit_ref(xw[r, 0].numpy(), L, "wrap")))


def test_config_errors_name_the_key(tmp_path):
    from src.datasets.esc50 import MIN_LOGMEL_SAMPLES, ESC50DataModule
    from src.datasets.urbansound8k import UrbanSound8KDataModule
    with pytest.raises(ValueError, match="clip_length"):  # the window rule owns the waveform path
        ESC50DataModule(root=str(tmp_path), is_spectrogram=False, preprocessing_config={"clip_length": 1.0})
    with pytest.raises(ValueError, match="clip_fit"):
        _module(tmp_path, clip_length=SECONDS, clip_fit="reflect")
    with pytest.raises(ValueError, match="clip_fit"):  # checked with the length unset as well
        _module(tmp_path, clip_fit="reflect")
    assert MIN_LOGMEL_SAMPLES == 513
    with pytest.raises(ValueError, match=r"clip_length.*513"):  # 512 samples at 8 kHz: one short of the log-mel's
        _module(tmp_path, clip_length=0.064)
    assert _module(tmp_path, clip_length=513 / RATE + 1e-9).fit_length == 513
    with pytest.raises(ValueError, match=r"clip_length.*513"):  # counted at the preprocessor's rate
        UrbanSound8KDataModule(root=str(tmp_path), sample_rate=44_100, is_spectrogram=True,
                               preprocessing_config={"clip_length": 0.05, "sample_rate": 8000})
    dm = UrbanSound8KDataModule(root=str(tmp_path), sample_rate=22_050, is_spectrogram=True,
                                preprocessing_config={"clip_length": 4.0, "sample_rate": 44_100})
    assert dm.fit_length == 176_400 and dm.clip_fit == "wrap"
    assert _module(tmp_path, clip_length=None).fit_length is None  # null is off


def test_shipped_configs_leave_clip_length_unset():
    from src.utils.config import compose
    spec = importlib.util.spec_from_file_location("train_script_fit", PKG / "scripts" / "train.py")
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    for model in ("ast", "ast_small", "ast_mini"):
        cfg = compose(PKG / "configs", "training", [f"model={model}"])
        pc = cfg.model.dataset_overrides.preprocessing_config
        assert "clip_length" not in pc and "clip_fit" not in pc
        key = "model.dataset_overrides.preprocessing_config"
        on = ts.datamodule_config(compose(PKG / "configs", "training",
                                          [f"model={model}", "dataset=urbansound8k", f"+{key}.clip_length=4.0",
                                           f"+{key}.clip_fit=zero"]))
        assert on["preprocessing_config"]["clip_length"] == 4.0 and on["preprocessing_config"]["clip_fit"] == "zero"
    assert dict(compose(PKG / "configs", "training", ["model=ast"]).model.dataset_overrides.preprocessing_config) == {
        "n_mels": 128, "normalize": True, "target_mean": 0.0, "target_std": 0.5, "multi_crop_test": False}
