"""GPU: WAV files -> peak-normalised clips in HBM (src/datasets/ingest.py) and the two prepare scripts, against the
numpy restatement of tests/_wav_ref.py.  The trees are generated here: integer PCM through the stdlib ``wave``
module, float / f64 / extensible / ADPCM-tagged headers through the ``struct`` helper."""
import importlib.util
import json
import logging

import numpy as np
import pytest
import torch

from src.datasets.ingest import ingest_wavs, plan_groups
from src.datasets.wav import WavError, parse_wav
from src.miaudio import lib as L
from tests import _wav_ref as R

pytestmark = pytest.mark.gpu
PKG = L.PKG_ROOT


def _script(name):
    spec = importlib.util.spec_from_file_location(name, PKG / "scripts" / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _write(path, raw, fmt, channels, rate, **kw):
    if fmt in (R.U8, R.S16, R.S24, R.S32) and not kw:
        R.write_pcm(path, raw, fmt, channels, rate)
    else:
        R.write_any(path, raw, fmt, channels, rate, **kw)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Twelve files: all six formats, mono and stereo, at 8 and 22.05 kHz, odd lengths; one s24 file extensible,
    one s16 file with a LIST chunk before fmt and a chunk after data.  -> [(path, raw, fmt, channels, rate)]"""
    root = tmp_path_factory.mktemp("wavs")
    files = []
    for k, fmt in enumerate([R.U8, R.S16, R.S24, R.S32, R.F32, R.F64] * 2):
        channels = 1 + (k + k // 6) % 2
        rate = 8000 if k % 3 else 22_050
        frames = 1500 + 211 * k
        raw = R.random_raw(fmt, frames, channels, seed=200 + k, peak_last=bool(k % 2))
        p = root / f"clip_{k:02d}.wav"
        kw = {}
        if k == 8:
            kw = {"extensible": True}
        if k == 7:
            kw = {"pre": [R.chunk(b"LIST", b"INFOabc")], "post": [R.chunk(b"LIST", b"INFOxyz")]}
        _write(p, raw, fmt, channels, rate, **kw)
        files.append((p, raw, fmt, channels, rate))
    return files


def test_native_rate_equals_the_restatement(cuda, tree):
    store, offsets, rates, skipped = ingest_wavs([f[0] for f in tree], cuda)
    assert skipped == [] and rates == [f[4] for f in tree]
    assert store.is_cuda and store.dtype == torch.float32 and offsets[0] == 0 and offsets[-1] == store.numel()
    host = store.cpu().numpy()
    for i, (p, raw, fmt, ch, rate) in enumerate(tree):
        got = host[offsets[i]:offsets[i + 1]]
        ref = R.ingest(raw, fmt, ch)
        assert got.shape == ref.shape and np.array_equal(got, ref), p.name
        assert np.abs(got).max() == 1.0, p.name


def test_target_rate_is_resample_of_the_mono_clip_then_its_own_peak(cuda, tree):
    from src.datasets.resample import GpuResample
    from src.miaudio import kernels as K
    target = 22_050
    store, offsets, rates, skipped = ingest_wavs([f[0] for f in tree], cuda, target_rate=target)
    assert skipped == [] and rates == [target] * len(tree)
    rs = GpuResample(8000, target)
    for i, (p, raw, fmt, ch, rate) in enumerate(tree):
        mono = torch.from_numpy(R.downmix(R.decode(raw, fmt, ch))).to(cuda)
        if rate != target:
            mono = rs(mono[None])[0].contiguous()
            assert mono.numel() == -(-target * (len(raw) // (R.BYTES[fmt] * ch)) // rate)  # ceil(new * len / orig)
        ref = R.normalise(mono.cpu().numpy())
        got = store[offsets[i]:offsets[i + 1]].cpu().numpy()
        assert got.shape == ref.shape and np.array_equal(got, ref), p.name
        assert np.abs(got).max() == 1.0
    # the peak used is the resampled clip's own
    off = torch.tensor(offsets, dtype=torch.int64, device=cuda)
    pk, nf = K.clip_peak(store, off)
    assert (pk.cpu().numpy().view(np.float32) == 1.0).all() and int(nf.sum()) == 0


def test_three_staging_groups_give_the_same_bits(cuda, tree):
    paths = [f[0] for f in tree]
    sizes = [parse_wav(p).data_bytes for p in paths]
    limit = next(m for m in range(max(sizes), sum(sizes), 256) if len(plan_groups(sizes, m)) == 3)
    for ids, offs, used in plan_groups(sizes, limit):
        assert all(o % 16 == 0 for o in offs) and used <= limit
    one = ingest_wavs(paths, cuda)
    three = ingest_wavs(paths, cuda, max_stage_bytes=limit)
    assert torch.equal(one[0], three[0]) and one[1:] == three[1:]


def test_rejected_files_are_skipped_or_raise_under_strict(cuda, tree, tmp_path):
    adpcm = tmp_path / "adpcm.wav"
    adpcm.write_bytes(R.wav_bytes(R.fmt_chunk(0x11, 1, 8000, 4, block_align=256), bytes(512)))
    nan = tmp_path / "nan.wav"
    vals = np.array([0.5, np.nan, -0.25, 0.125], "<f4")
    R.write_any(nan, vals.tobytes(), R.F32, 1, 8000)
    empty = tmp_path / "empty.wav"
    R.write_pcm(empty, b"", R.S16, 2, 8000)
    paths = [tree[1][0], adpcm, tree[2][0], nan, empty, tree[3][0]]
    store, offsets, rates, skipped = ingest_wavs(paths, cuda)
    assert [(i, p) for i, p, _ in skipped] == [(1, str(adpcm)), (3, str(nan)), (4, str(empty))]
    assert "format tag 0x11" in skipped[0][2] and "non-finite" in skipped[1][2] and "no whole frame" in skipped[2][2]
    assert offsets[1] == offsets[2] and offsets[4] == offsets[5] and rates[1] == 0 and rates[4] == 0
    for i, k in ((0, 1), (2, 2), (5, 3)):  # the good files are what they are alone
        _, raw, fmt, ch, _ = tree[k]
        assert np.array_equal(store[offsets[i]:offsets[i + 1]].cpu().numpy(), R.ingest(raw, fmt, ch))
    with pytest.raises(WavError, match="adpcm.wav.*format tag 0x11"):
        ingest_wavs(paths, cuda, strict=True)
    with pytest.raises(WavError, match="nan.wav.*non-finite"):
        ingest_wavs([tree[1][0], nan], cuda, strict=True)


def test_a_file_that_shrinks_after_parsing_is_skipped(cuda, tree, monkeypatch):
    """The short read goes through ``skipped`` like every other rejection; the other clips are what they are alone."""
    import shutil
    from src.datasets import ingest
    victim = tree[4][0].with_name("shrinks.wav")
    shutil.copy(tree[4][0], victim)

    def parse_then_truncate(p):
        info = parse_wav(p)
        if str(p) == str(victim):
            with open(p, "r+b") as f:
                f.truncate(info.data_offset + info.data_bytes // 2)
        return info

    monkeypatch.setattr(ingest, "parse_wav", parse_then_truncate)
    paths = [tree[1][0], victim, tree[2][0]]
    store, offsets, rates, skipped = ingest_wavs(paths, cuda)
    assert [(i, p) for i, p, _ in skipped] == [(1, str(victim))] and "the file changed" in skipped[0][2]
    for i, k in ((0, 1), (2, 2)):
        _, raw, fmt, ch, _ = tree[k]
        assert np.array_equal(store[offsets[i]:offsets[i + 1]].cpu().numpy(), R.ingest(raw, fmt, ch))
    shutil.copy(tree[4][0], victim)
    with pytest.raises(WavError, match="shrinks.wav.*the file changed"):
        ingest_wavs(paths, cuda, strict=True)


# ------------------------------------------------------------------------------------------------ the scripts
CLIPS_PER_FOLD, CLIP_SAMPLES = 12, 176_400  # the bundle trees of tests/test_gpu_train_script.py


def _s16(frames, channels, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-12_000, 12_000, frames * channels).astype("<i2").tobytes()


def test_prepare_esc50(cuda, tmp_path, caplog):
    raw_dir = tmp_path / "raw" / "esc50"
    (raw_dir / "meta").mkdir(parents=True)
    (raw_dir / "audio").mkdir()
    rows, truth = [], {}
    for f in range(5):
        for i in range(CLIPS_PER_FOLD):
            name, label, channels = f"{f + 1}-{1000 + i}-A-{(f + i) % 10}.wav", (f + i) % 10, 1 + (i % 3 == 0)
            raw = _s16(CLIP_SAMPLES, channels, seed=100 * f + i)
            R.write_pcm(raw_dir / "audio" / name, raw, R.S16, channels, 44_100)
            rows.append(f"{name},{f + 1},{label},class_{label},False,{1000 + i},A")
            truth[name] = (f, label, raw, channels)
    rows.append("9-9-A-0.wav,1,0,class_0,False,9,A")  # named by the CSV, absent from the tree
    (raw_dir / "meta" / "esc50.csv").write_text("filename,fold,target,category,esc10,src_file,take\n"
                                                + "\n".join(rows) + "\n")
    with caplog.at_level(logging.WARNING, logger="prepare"):
        stats = _script("prepare_esc50").prepare_esc50(tmp_path, validate_hash=False, device=cuda)
    assert "9-9-A-0.wav" in caplog.text and "left out" in caplog.text  # warned about, then skipped
    out = tmp_path / "processed" / "esc50"
    assert stats == json.loads((out / "dataset_stats.json").read_text())
    assert stats["num_clips"] == 60 and stats["total_duration_sec"] == pytest.approx(60 * 4.0)
    labels = [t[1] for t in truth.values()]
    assert stats["class_histogram"] == {f"class_{c}": labels.count(c) for c in range(10)}
    assert "file_hashes" not in stats
    assert stats["skipped"] == [{"file": str(raw_dir / "audio" / "9-9-A-0.wav"), "reason": "missing file"}]
    assert len(list(out.glob("fold_*/*.pt"))) == 60
    for name, (f, label, raw, channels) in truth.items():
        b = torch.load(out / f"fold_{f}" / name.replace(".wav", ".pt"), weights_only=True)
        assert set(b) == {"waveform", "label"} and b["label"] == label
        w = b["waveform"]
        assert w.dtype == torch.float32 and tuple(w.shape) == (1, CLIP_SAMPLES) and w.device.type == "cpu"
        assert np.array_equal(w.numpy()[0], R.ingest(raw, R.S16, channels)), name

    from src.datasets.esc50 import ESC50DataModule
    dm = ESC50DataModule(str(out), fold=0, sample_rate=44_100, num_classes=10, val_split=0.25, batch_size=8,
                         num_workers=0)
    dm.attach(cuda)
    dm.setup("fit")
    x, y = next(iter(dm.train_dataloader()))
    assert x.shape[0] == 8 and x.shape[1] == 1 and y.shape[0] == 8 and bool(torch.isfinite(x).all())


def test_prepare_esc50_hashes(cuda, tmp_path):
    import hashlib
    raw_dir = tmp_path / "raw" / "esc50"
    (raw_dir / "meta").mkdir(parents=True)
    (raw_dir / "audio").mkdir()
    R.write_pcm(raw_dir / "audio" / "1-1-A-3.wav", _s16(8000, 1, 1), R.S16, 1, 22_050)
    (raw_dir / "meta" / "esc50.csv").write_text("filename,fold,target,category\n1-1-A-3.wav,1,3,cow\n")
    stats = _script("prepare_esc50").prepare_esc50(tmp_path, device=cuda)
    digest = hashlib.sha256((raw_dir / "audio" / "1-1-A-3.wav").read_bytes()).hexdigest()
    assert stats["file_hashes"] == {"1-1-A-3.wav": digest}
    b = torch.load(tmp_path / "processed" / "esc50" / "fold_0" / "1-1-A-3.pt", weights_only=True)
    assert tuple(b["waveform"].shape) == (1, 16_000) and b["label"] == 3  # resampled 22.05 -> 44.1 kHz


def test_prepare_urbansound8k(cuda, tmp_path):
    raw_dir = tmp_path / "raw" / "urbansound8k"
    (raw_dir / "metadata").mkdir(parents=True)
    rates = (8000, 16_000, 22_050, 44_100)
    formats = (R.S16, R.S24, R.U8, R.F32, R.S32, R.F64)
    rows, truth = [], {}
    for f in range(10):
        (raw_dir / "audio" / f"fold{f + 1}").mkdir(parents=True)
        for i in range(CLIPS_PER_FOLD):
            k = CLIPS_PER_FOLD * f + i
            name, label = f"{1000 + k}-{(f + i) % 10}-0-{i}.wav", (f + i) % 10
            fmt, channels, rate = formats[k % 6], 1 + k % 2, rates[k % 4]
            raw = R.random_raw(fmt, rate // 4 + k, channels, seed=k)
            _write(raw_dir / "audio" / f"fold{f + 1}" / name, raw, fmt, channels, rate)
            rows.append(f"{name},{1000 + k},0.0,0.25,1,{f + 1},{label},class_{label}")
            truth[name] = (f, label, raw, fmt, channels, rate)
    (raw_dir / "metadata" / "UrbanSound8K.csv").write_text(
        "slice_file_name,fsID,start,end,salience,fold,classID,class\n" + "\n".join(rows) + "\n")
    us = _script("prepare_urbansound8k")
    stats = us.prepare_urbansound8k(tmp_path, device=cuda)
    out = tmp_path / "processed" / "urbansound8k"
    assert stats["num_clips"] == 120 and stats["skipped"] == []
    for name, (f, label, raw, fmt, channels, rate) in truth.items():
        b = torch.load(out / f"fold_{f}" / name.replace(".wav", ".pt"), weights_only=True)
        assert set(b) == {"waveform", "label", "sample_rate"}
        assert b["label"] == label and b["sample_rate"] == rate and isinstance(b["sample_rate"], int)
        assert np.array_equal(b["waveform"].numpy()[0], R.ingest(raw, fmt, channels)), name

    from src.datasets.urbansound8k import UrbanSound8KDataModule
    dm = UrbanSound8KDataModule(str(out), fold=9, sample_rate=22_050, val_split=0.1, batch_size=8, num_workers=0,
                                preprocessing_config={"sample_rate": 16_000, "window_length": 0.1})
    dm.attach(cuda)
    dm.setup("fit")
    assert len(dm._store) == 120 and dm._store.sample_rate == 16_000
    x, y = next(iter(dm.train_dataloader()))
    assert x.shape[0] == 8 and y.shape[0] == 8

    # --target-rate: bundles already at R, without the key
    stats = us.prepare_urbansound8k(tmp_path, target_rate=16_000, device=cuda)
    name, (f, label, raw, fmt, channels, rate) = next((n, t) for n, t in truth.items() if t[5] == 44_100)
    b = torch.load(out / f"fold_{f}" / name.replace(".wav", ".pt"), weights_only=True)
    frames = len(raw) // (R.BYTES[fmt] * channels)
    assert set(b) == {"waveform", "label"} and b["waveform"].shape[-1] == -(-16_000 * frames // 44_100)
    assert float(b["waveform"].abs().max()) == 1.0


def test_scripts_fail_without_a_gpu_device(tmp_path):
    raw_dir = tmp_path / "raw" / "esc50"
    (raw_dir / "meta").mkdir(parents=True)
    (raw_dir / "meta" / "esc50.csv").write_text("filename,fold,target,category\n")
    with pytest.raises(ValueError, match="no CPU path"):
        _script("prepare_esc50").prepare_esc50(tmp_path, device="cpu")


def test_library_exports_the_wav_entry_points():
    assert {"mia_pcm_decode", "mia_clip_peak", "mia_clip_scale"} <= L.exported_symbols()
    assert {"mia_pcm_decode", "mia_clip_peak", "mia_clip_scale"} <= set(L.SIGNATURES)
