"""CPU: the RIFF/WAVE container parser (src/datasets/wav.py), the CSV planning of the two prepare scripts
(src/datasets/prepare.py) and the numpy restatement the GPU decode is compared with (tests/_wav_ref.py).

Files are written by the tests: integer PCM through the stdlib ``wave`` module, everything else through the
``struct`` helper of _wav_ref."""
import logging
import struct

import numpy as np
import pytest
import torch

from src.datasets.prepare import plan_esc50, plan_urbansound8k
from src.datasets.wav import WavError, WavInfo, parse_wav
from src.miaudio import lib as L
from tests import _wav_ref as R

FORMATS = [R.U8, R.S16, R.S24, R.S32, R.F32, R.F64]


def _write(path, raw, fmt, channels, rate):
    if fmt in (R.U8, R.S16, R.S24, R.S32):
        R.write_pcm(path, raw, fmt, channels, rate)
    else:
        R.write_any(path, raw, fmt, channels, rate)


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS, ids=R.NAMES)
def test_header_round_trip(tmp_path, fmt, channels):
    frames, rate = 37, 22_050
    raw = R.random_raw(fmt, frames, channels, seed=fmt * 10 + channels)
    p = tmp_path / "a.wav"
    _write(p, raw, fmt, channels, rate)
    info = parse_wav(p)
    tag, bits = R.TAG_BITS[fmt]
    assert isinstance(info, WavInfo)
    assert (info.format_code, info.channels, info.sample_rate, info.bits, info.frames) == \
        (tag, channels, rate, bits, frames)
    assert info.data_bytes == len(raw) and info.device_format == fmt
    blob = p.read_bytes()
    assert blob[info.data_offset:info.data_offset + info.data_bytes] == raw
    assert parse_wav(blob) == info  # bytes in place of a path


def test_device_format_codes_match_the_library():
    assert (L.PCM_U8, L.PCM_S16, L.PCM_S24, L.PCM_S32, L.PCM_F32, L.PCM_F64) == tuple(FORMATS)
    assert L.PCM_BYTES == R.BYTES


@pytest.mark.parametrize("fmt", [R.S16, R.S32, R.F32], ids=["s16", "s32", "f32"])
@pytest.mark.parametrize("channels", [1, 2])
def test_samples_agree_with_scipy(tmp_path, fmt, channels):
    from scipy.io import wavfile
    raw = R.random_raw(fmt, 50, channels, seed=3)
    p = tmp_path / "a.wav"
    _write(p, raw, fmt, channels, 16_000)
    rate, data = wavfile.read(p)
    info = parse_wav(p)
    ours = R.decode(p.read_bytes()[info.data_offset:info.data_offset + info.data_bytes], fmt, channels)
    data = data.reshape(50, channels)
    if fmt == R.S16:
        theirs = data.astype(np.float32) / np.float32(32768)
    elif fmt == R.S32:
        theirs = data.astype(np.float32) * np.float32(2.0 ** -31)
    else:
        theirs = data
    assert rate == info.sample_rate and theirs.dtype == np.float32
    assert np.array_equal(ours, theirs)


def _fmt(tag=1, channels=2, rate=8000, bits=16, **kw):
    return R.fmt_chunk(tag, channels, rate, bits, **kw)


RAW = R.random_raw(R.S16, 10, 2, seed=1)  # 40 bytes, 10 stereo frames


def test_list_chunk_before_fmt():
    blob = R.wav_bytes(_fmt(), RAW, pre=[R.chunk(b"LIST", b"INFOabcd"), R.chunk(b"JUNK", b"\0" * 28)])
    info = parse_wav(blob)
    assert info.frames == 10 and blob[info.data_offset:info.data_offset + 40] == RAW


def test_odd_sized_chunk_has_a_pad_byte():
    blob = R.wav_bytes(_fmt(), RAW, pre=[R.chunk(b"bext", b"abc")])  # 3 bytes + 1 pad
    info = parse_wav(blob)
    assert info.frames == 10 and blob[info.data_offset:info.data_offset + 40] == RAW


def test_trailing_chunk_after_data_is_ignored():
    blob = R.wav_bytes(_fmt(), RAW, post=[R.chunk(b"LIST", b"INFOxyzw"), R.chunk(b"fmt ", b"garbage!")])
    info = parse_wav(blob)
    assert info.frames == 10 and info.data_bytes == 40


def test_declared_size_larger_than_the_file_is_clamped_to_whole_frames():
    blob = R.wav_bytes(_fmt(), RAW[:-1], declared=4000)  # 39 bytes present: 9 whole stereo s16 frames
    info = parse_wav(blob)
    assert info.frames == 9 and info.data_bytes == 36
    assert info.data_offset + info.data_bytes <= len(blob)


@pytest.mark.parametrize("declared", [0, 0xFFFFFFFF])
def test_declared_size_zero_or_all_ones_means_to_the_end(declared):
    info = parse_wav(R.wav_bytes(_fmt(), RAW, declared=declared))
    assert info.frames == 10 and info.data_bytes == 40


def test_extensible_pcm_and_float():
    raw24 = R.random_raw(R.S24, 7, 2, seed=2)
    info = parse_wav(R.wav_bytes(_fmt(1, 2, 48_000, 24, extensible=True), raw24))
    assert (info.format_code, info.bits, info.channels, info.frames, info.device_format) == (1, 24, 2, 7, R.S24)
    rawf = R.random_raw(R.F32, 7, 1, seed=2)
    info = parse_wav(R.wav_bytes(_fmt(3, 1, 96_000, 32, extensible=True), rawf))
    assert (info.format_code, info.bits, info.sample_rate, info.frames, info.device_format) == \
        (3, 32, 96_000, 7, R.F32)


@pytest.mark.parametrize("blob,reason", [
    (R.wav_bytes(_fmt(), RAW, riff=b"RIFX"), "RIFX"),
    (R.wav_bytes(_fmt(), RAW, riff=b"RF64"), "RF64"),
    (R.wav_bytes(None, RAW), "missing fmt"),
    (R.wav_bytes(_fmt(), None), "missing data"),
    (R.wav_bytes(_fmt(block_align=3), RAW), "block_align"),
    (R.wav_bytes(_fmt(channels=0, block_align=0), RAW), "zero channels"),
    (R.wav_bytes(_fmt(tag=2, bits=4, block_align=256), RAW), "format tag 0x2"),
    (R.wav_bytes(_fmt(tag=0x11, bits=4, block_align=256), RAW), "format tag 0x11"),
    (R.wav_bytes(_fmt(tag=6, bits=8), RAW), "format tag 0x6"),
    (R.wav_bytes(_fmt(tag=7, bits=8), RAW), "format tag 0x7"),
    (R.wav_bytes(_fmt(tag=1, bits=12, block_align=3), RAW), "bit depth 12"),
    (R.wav_bytes(_fmt(tag=3, bits=16), RAW), "bit depth 16"),
    (R.wav_bytes(_fmt(1, 2, 8000, 16, extensible=True, sub_tag=2), RAW), "sub-format"),
    (b"RIFF\x04\0\0\0WAVX", "not a RIFF/WAVE"),
], ids=["rifx", "rf64", "no-fmt", "no-data", "block-align", "zero-channels", "adpcm", "ima-adpcm", "alaw", "mulaw",
        "pcm12", "float16", "ext-adpcm", "not-wave"])
def test_rejections_name_the_reason(tmp_path, blob, reason):
    with pytest.raises(WavError, match=reason):
        parse_wav(blob)
    p = tmp_path / "bad.wav"
    p.write_bytes(blob)
    with pytest.raises(WavError, match="bad.wav") as e:
        parse_wav(p)
    assert reason in str(e.value)


def test_missing_path_is_a_wav_error(tmp_path):
    with pytest.raises(WavError, match="nothing.wav"):
        parse_wav(tmp_path / "nothing.wav")


# ------------------------------------------------------------------------------------------------ CSV planning
def test_plan_esc50(tmp_path, caplog):
    raw = tmp_path / "raw" / "esc50"
    (raw / "meta").mkdir(parents=True)
    (raw / "audio").mkdir()
    rows = [("1-100-A-0.wav", 1, 0, "dog"), ("2-7-B-49.wav", 2, 49, "hand_saw"), ("5-9-A-12.wav", 5, 12, "fire, crackling"),
            ("3-1-A-3.wav", 3, 3, "cow")]
    with (raw / "meta" / "esc50.csv").open("w") as f:
        f.write("filename,fold,target,category,esc10,src_file,take\n")
        for name, fold, target, cat in rows:
            f.write(f'{name},{fold},{target},"{cat}",False,1,A\n')
    for name, *_ in rows[:3]:
        (raw / "audio" / name).write_bytes(b"")
    out = tmp_path / "processed" / "esc50"
    with caplog.at_level(logging.WARNING, logger="prepare"):
        plan, missing = plan_esc50(raw, out)
    assert [(it.out, it.label, it.category) for it in plan] == [
        (out / "fold_0" / "1-100-A-0.pt", 0, "dog"), (out / "fold_1" / "2-7-B-49.pt", 49, "hand_saw"),
        (out / "fold_4" / "5-9-A-12.pt", 12, "fire, crackling")]
    assert [it.wav for it in plan] == [raw / "audio" / r[0] for r in rows[:3]]
    assert missing == [str(raw / "audio" / "3-1-A-3.wav")]
    assert "3-1-A-3.wav" in caplog.text and "left out" in caplog.text


def test_plan_urbansound8k(tmp_path, caplog):
    raw = tmp_path / "us8k"
    (raw / "metadata").mkdir(parents=True)
    rows = [("100032-3-0-0.wav", 5, 3, "dog_bark"), ("7061-6-0-0.wav", 1, 6, "gun_shot"),
            ("99812-1-2-0.wav", 10, 1, "car_horn"), ("1-1-1-1.wav", 2, 1, "car_horn")]
    with (raw / "metadata" / "UrbanSound8K.csv").open("w") as f:
        f.write("slice_file_name,fsID,start,end,salience,fold,classID,class\n")
        for name, fold, cid, cls in rows:
            f.write(f"{name},1,0.0,4.0,1,{fold},{cid},{cls}\n")
    for name, fold, *_ in rows[:3]:
        (raw / "audio" / f"fold{fold}").mkdir(parents=True, exist_ok=True)
        (raw / "audio" / f"fold{fold}" / name).write_bytes(b"")
    out = tmp_path / "out"
    with caplog.at_level(logging.WARNING, logger="prepare"):
        plan, missing = plan_urbansound8k(raw, out)
    assert [(it.wav, it.out, it.label) for it in plan] == [
        (raw / "audio" / "fold5" / rows[0][0], out / "fold_4" / "100032-3-0-0.pt", 3),
        (raw / "audio" / "fold1" / rows[1][0], out / "fold_0" / "7061-6-0-0.pt", 6),
        (raw / "audio" / "fold10" / rows[2][0], out / "fold_9" / "99812-1-2-0.pt", 1)]
    assert missing == [str(raw / "audio" / "fold2" / "1-1-1-1.wav")] and "1-1-1-1.wav" in caplog.text


def test_plan_rejects_a_csv_without_the_columns(tmp_path):
    (tmp_path / "meta").mkdir()
    (tmp_path / "meta" / "esc50.csv").write_text("filename,fold\n")
    with pytest.raises(ValueError, match="target"):
        plan_esc50(tmp_path, tmp_path / "out")
    with pytest.raises(FileNotFoundError):
        plan_urbansound8k(tmp_path, tmp_path / "out")


def test_prepare_scripts_refuse_a_cpu_device(tmp_path):
    from src.datasets.ingest import ingest_wavs
    with pytest.raises(ValueError, match="no CPU path"):
        ingest_wavs([], "cpu")


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", [R.U8, R.S16, R.S24, R.S32], ids=["u8", "s16", "s24", "s32"])
def test_downmix_equals_torch_mean(fmt, channels):
    x = R.decode(R.random_raw(fmt, 4097, channels, seed=fmt + 7 * channels), fmt, channels)
    ours = R.downmix(x)
    theirs = torch.mean(torch.from_numpy(x.T.copy()), dim=0).numpy()  # (C, T) as torchaudio.load returns
    assert np.array_equal(ours.view(np.int32), theirs.view(np.int32))


def test_decode_boundary_values():
    assert R.decode(bytes([0, 128, 255]), R.U8, 1).ravel().tolist() == [-1.0, 0.0, 127 / 128]
    assert R.decode(struct.pack("<hh", -32768, 32767), R.S16, 1).ravel().tolist() == [-1.0, 32767 / 32768]
    s24 = b"\x00\x00\x80" + b"\xff\xff\xff" + b"\xff\xff\x7f"
    assert R.decode(s24, R.S24, 1).ravel().tolist() == [-1.0, -(2.0 ** -23), 1 - 2.0 ** -23]
    s32 = struct.pack("<iiii", -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3)
    assert R.decode(s32, R.S32, 1).ravel().tolist() == [-1.0, 1.0, 2.0 ** -7, (2 ** 24 + 4) * 2.0 ** -31]
    big = R.decode(struct.pack("<dd", 1e39, 1 + 2.0 ** -30), R.F64, 1).ravel()
    assert np.isinf(big[0]) and big[1] == 1.0
    mono = np.array([0.5, np.nan, -0.75, np.inf], np.float32)
    assert R.peak(mono) == 0.75 and R.nonfinite(mono) == 2
    assert np.array_equal(R.normalise(np.zeros(4, np.float32)), np.zeros(4, np.float32))
