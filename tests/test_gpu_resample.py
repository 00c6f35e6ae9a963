"""GPU: mia_resample (include/miaudio_resample.h), its wrapper and the data modules' resampling path.

* exact: integer taps in [-3, 3] and integer samples in [-8, 8] handed straight to the entry point; every partial
  sum stays below 475 * 24 < 2^24, so f32 is exact in any order and the output must equal the int64 direct sum bit
  for bit.  Lengths: 1, o - 1, o, 2 o + 1 and one under 40 000.  The kernel's tile along frames is the 32-frame
  MFMA tile of one wave, four of them to a workgroup; the long length crosses at least two of those and leaves a
  remainder for every geometry (441 -> 160 has 91 frames at 39 999 samples) and crosses a workgroup boundary for
  all but 441 -> 160, whose 128 frames would need 56 448 samples (the value test below has that case).
* values: the real taps of six rate pairs on randn clips against the float64 restatement (tests/_resample_ref.py)
  under the f32 dot-product bound gamma_K * sum |x||tap| + 2^-149, gamma_K = K u / (1 - K u), u = 2^-24: the
  standard bound for K terms in any order, with or without FMA -- not a fitted tolerance.
"""
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from src.miaudio import lib as L
from src.utils.config import compose
from tests import _resample_ref as R

pytestmark = pytest.mark.gpu
PKG = Path(__file__).resolve().parents[1] / "dl-sound-classification_amd"
SENTINEL = -12345.5


def _call(dev, x, T, taps, o, n, width, lengths=None, slack=3):
    """mia_resample on x (B, ldx >= T) -> (B, Tout) CPU; ldo = Tout + slack with a sentinel in the slack."""
    lib = L.load()
    B, ldx = x.shape
    Tout = lib.mia_resample_out_len(T, o, n)
    assert Tout == R.out_len(T, o, n)
    out = torch.full((B, Tout + slack), SENTINEL, dtype=torch.float32, device=dev)
    xd, td = x.to(dev), taps.to(dev)
    ld = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    L.check(lib.mia_resample(xd.data_ptr(), ldx, B, T, L.ptr(ld), td.data_ptr(), o, n, width, out.data_ptr(),
                             Tout + slack, Tout, L.stream_ptr()), "mia_resample")
    out = out.cpu()
    assert bool((out[:, Tout:] == SENTINEL).all()), "the slack columns [Tout, ldo) were written"
    return out[:, :Tout]


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("o,n,width,long_T", [(3, 2, 2, 1000), (2, 3, 1, 777), (1, 2, 7, 300), (441, 160, 17, 39_999),
                                              (160, 441, 7, 39_999)])
def test_integer_operands_are_exact(cuda, o, n, width, long_T):
    rng = np.random.default_rng(o * 1000 + n)
    K = 2 * width + o
    taps = rng.integers(-3, 4, (n, K))
    frames = math.ceil(R.out_len(long_T, o, n) / n)
    assert frames > 64 and frames % 32 and long_T < 40_000  # two 32-frame tiles and a remainder
    for T in sorted({1, o - 1, o, 2 * o + 1, long_T} - {0}):
        x = rng.integers(-8, 9, (3, T + 5))  # ldx > T; the 5 extra columns are never part of a clip
        for lengths in (None, [0, T, T // 2 + 1]):
            want = R.apply_exact(x[:, :T], taps, o, n, width, lengths)
            got = _call(cuda, torch.from_numpy(x).float(), T, torch.from_numpy(taps).float(), o, n, width, lengths)
            assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
            g = got.numpy()
            assert np.array_equal(g.astype(np.int64), want) and np.array_equal(g, want.astype(np.float32)), \
                (o, n, T, lengths, int((g != want).sum()))
            for b in range(3):  # the tail behind each clip's own output length: +0.0, sign bit clear
                ol = R.out_len(T if lengths is None else lengths[b], o, n)
                assert not g[b, ol:].view(np.uint32).any(), (o, n, T, lengths, b)


def test_bad_arguments_are_rejected_before_any_launch(cuda):
    lib = L.load()
    x = torch.zeros(2, 100, device=cuda)
    out = torch.full((2, 5000), SENTINEL, device=cuda)  # room for every call below, were one of them not rejected
    taps = torch.zeros(4097 * 4097, device=cuda)

    def rc(o, n, width, T=100, Tout=None, ldx=100, ldo=5000, B=2):
        Tout = R.out_len(T, o, n) if Tout is None else Tout
        return lib.mia_resample(x.data_ptr(), ldx, B, T, None, taps.data_ptr(), o, n, width, out.data_ptr(), ldo, Tout,
                                L.stream_ptr())
    assert rc(4, 2, 1) < 0 and rc(441, 147, 3) < 0  # not coprime
    assert rc(3, 2, 2, Tout=66) < 0 and rc(3, 2, 2, ldx=99) < 0 and rc(3, 2, 2, ldo=66) < 0
    assert rc(3, 2, 2047) < 0 and rc(1, 4097, 1, T=1, ldx=1, ldo=4097) < 0  # K = 4097, n = 4097: over the limits
    assert rc(0, 2, 1, Tout=0) < 0 and rc(3, 2, -1) < 0
    assert rc(3, 2, 2) == 0 and rc(3, 2, 2, B=0) == 0
    torch.cuda.synchronize()
    assert bool((out[:, 67:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ values
VALUE_T = {(44100, 16000): 60_000, (16000, 44100): 21_000, (44100, 22050): 1000, (22050, 44100): 700,
           (44100, 48000): 20_000, (8000, 44100): 10_500}  # 131..500 frames: past a 128-frame workgroup, ragged


@pytest.mark.parametrize("orig,new", R.PAIRS)
def test_values_within_the_f32_dot_product_bound(cuda, orig, new):
    from src.datasets.resample import GpuResample
    rs = GpuResample(orig, new)
    o, n, width, K = R.geometry(orig, new)
    assert (rs.o, rs.n, rs.width, rs.K) == (o, n, width, K)
    T = VALUE_T[(orig, new)]
    x = torch.randn(2, T, generator=torch.Generator().manual_seed(orig + new))
    lengths = [T, T // 3 + 1]
    ref, mag = R.apply(x.numpy(), rs.taps.numpy(), o, n, width)
    got = rs(x.to(cuda))
    assert tuple(got.shape) == (2, rs.out_len(T)) == ref.shape
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    bound = R.bound(K, mag)
    print(f"{orig} -> {new}: max |err| {err.max():.3e}, max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    ref2, mag2 = R.apply(x.numpy(), rs.taps.numpy(), o, n, width, lengths)
    got2 = rs(x.to(cuda), lengths=torch.tensor(lengths)).cpu().numpy()
    assert bool((np.abs(got2.astype(np.float64) - ref2) <= R.bound(K, mag2)).all())
    assert not got2[1, R.out_len(lengths[1], o, n):].view(np.uint32).any()
    # same inputs, same bits
    again = rs(x.to(cuda))
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ------------------------------------------------------------------------------------------------ wrapper
def test_wrapper_shapes_and_identity(cuda):
    from src.datasets.resample import GpuResample
    x = torch.randn(3, 1, 801, device=cuda)
    assert GpuResample(44100, 44100)(x) is x
    rs = GpuResample(8000, 44100)
    y = rs(x)
    assert tuple(y.shape) == (3, 1, math.ceil(801 * 441 / 80)) and y.dtype == torch.float32
    assert torch.equal(y[:, 0], rs(x[:, 0]))
    assert len(rs._dev) == 1 and rs.taps_on(cuda) is rs.taps_on(cuda)
    with pytest.raises(ValueError):
        rs(torch.zeros(2, 2, 100, device=cuda))


# ------------------------------------------------------------------------------------------------ data module
def _bundles(root, tagged=None):
    """Eight bundles of 0.25 s at 8 kHz (2000 samples and a few more) over five folds; ``tagged`` maps a bundle
    index to a sample rate of its own."""
    g = torch.Generator().manual_seed(5)
    files, k = [], 0
    for f, count in enumerate((2, 2, 2, 1, 1)):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(count):
            b = {"waveform": 0.3 * torch.randn(1, 2000 + 7 * k, generator=g), "label": k % 2}
            if tagged and k in tagged:
                b["sample_rate"] = tagged[k]
            torch.save(b, d / f"clip_{k}.pt")
            files.append(d / f"clip_{k}.pt")
            k += 1
    return files


def _dm(root, dev, **kw):
    from src.datasets.esc50 import ESC50DataModule
    dm = ESC50DataModule(str(root), fold=0, sample_rate=8000, num_classes=2, val_split=0.3, batch_size=2, num_workers=0,
                         preprocessing_config={"sample_rate": 44100, "window_length": 0.1}, **kw)
    dm.attach(dev)
    dm.setup()
    return dm


def test_data_module_resamples_once_in_setup(cuda, tmp_path, capsys):
    from src.datasets.resample import GpuResample
    files = _bundles(tmp_path)
    dm = _dm(tmp_path, cuda, enable_bc_mixing=True)
    assert "resampled 8 clips to 44100 Hz" in capsys.readouterr().out
    store = dm._store
    assert len(store) == 8 and store.data.is_shared() and store.nbytes == 4 * store.offsets[-1]
    rs = GpuResample(8000, 44100)
    o, n, width, K = R.geometry(8000, 44100)
    for f in files:
        raw = torch.load(f, weights_only=True)
        clip, label = store.get(f)
        assert label == int(raw["label"]) and tuple(clip.shape) == (1, rs.out_len(raw["waveform"].shape[-1]))
        assert torch.equal(clip, rs(raw["waveform"].to(cuda)).cpu())
        ref, mag = R.apply(raw["waveform"].numpy(), rs.taps.numpy(), o, n, width)
        assert bool((np.abs(clip.numpy().astype(np.float64) - ref) <= R.bound(K, mag)).all())
    # window and padding in 44.1 kHz samples; the three datasets read the store
    for ds in (dm._train_set, dm._val_set, dm._test_set):
        assert ds.store is store and (ds.window, ds.pad) == (4410, 2205)
    assert len(dm._train_set) + len(dm._val_set) == 6 and len(dm._test_set) == 2
    w, _ = dm._val_set[0]
    assert tuple(w.shape) == (1, 4410)
    # the BC pool: the resampled training clips, cut to the window
    dm._pools()
    assert tuple(dm._pool.shape) == (len(dm._train_set), 4410) and dm._pool.is_cuda
    for i, f in enumerate(dm._train_set.files):
        assert torch.equal(dm._pool[i].cpu(), store.get(f)[0][0, :4410])
    assert dm._pool_labels.tolist() == [store.get(f)[1] for f in dm._train_set.files]
    xb, yb = next(iter(dm.train_dataloader()))  # the BC path crops to the window without padding
    assert tuple(xb.shape) == (2, 1, 4410) and tuple(yb.shape) == (2,)


def test_ast_mode_builds_its_logmel_at_the_target_rate(cuda, tmp_path):
    from src.datasets.esc50 import ESC50DataModule
    dm = ESC50DataModule(str(tmp_path), sample_rate=8000, is_spectrogram=True,
                         preprocessing_config={"sample_rate": 44100, "n_mels": 64})
    assert dm.logmel().cfg.sample_rate == 44100 and dm.logmel().n_mels == 64
    same = ESC50DataModule(str(tmp_path), sample_rate=16000, is_spectrogram=True, preprocessing_config={})
    assert same.logmel().cfg.sample_rate == 16000


def test_a_bundle_with_its_own_rate_is_resampled_from_it(cuda, tmp_path):
    from src.datasets.resample import GpuResample
    files = _bundles(tmp_path, tagged={1: 16000, 4: 44100, 6: 8000})
    store = _dm(tmp_path, cuda)._store
    for k, rate in ((0, 8000), (1, 16000), (4, 44100), (6, 8000)):
        raw = torch.load(files[k], weights_only=True)["waveform"]
        want = raw if rate == 44100 else GpuResample(rate, 44100)(raw.to(cuda)).cpu()
        assert torch.equal(store.get(files[k])[0], want), (k, rate)


# ------------------------------------------------------------------------------------------------ train script
def test_train_script_resamples_synthetic_16k_clips_to_44k1(cuda, tmp_path, monkeypatch):
    """dataset=synthetic at 16 kHz with 80 000-sample clips, the EnvNet preprocessor at 44.1 kHz: the clips become
    exactly 220 500 samples in setup(); two training steps at B = 4, then validation and test."""
    spec = importlib.util.spec_from_file_location("train_script", PKG / "scripts" / "train.py")
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    monkeypatch.chdir(tmp_path)
    over = ["dataset=synthetic", "dataset.num_clips=20", "dataset.sample_rate=16000", "dataset.clip_samples=80000",
            "model=envnet_v2", "+model.dataset_overrides.preprocessing_config.sample_rate=44100",
            "trainer.precision=bf16-mixed", "trainer.max_epochs=1", "+trainer.limit_train_batches=2", "batch_size=4", "num_workers=0",
            f"checkpoint.dirpath={tmp_path}/ck", "checkpoint.monitor=val/loss", "checkpoint.mode=min"]
    out = ts.train(compose(PKG / "configs", "training", over))
    dm = ts.LAST_TRAINER.datamodule
    assert dm.target_rate == 44100 and dm.sample_rate == 16000
    assert tuple(dm._train_set[0].shape) == (16, 1, 220_500) and dm._train_set[0].is_cuda
    assert ts.LAST_TRAINER._module.global_step == 2
    assert math.isfinite(out["test/loss"]) and all(math.isfinite(v) for v in out.values()), out
