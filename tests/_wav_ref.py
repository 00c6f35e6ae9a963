"""CPU restatement of WAV ingestion (numpy only) and the WAV writers the tests use.

The restatement is what the GPU kernels of include/miaudio_wav.h are compared with, bit for bit:
``decode`` (np.frombuffer-based unpack, torchaudio's normalize=True scaling), ``downmix`` (sequential f32 channel
sum, ``/ np.float32(C)``), ``peak`` (max |x| over the finite samples) and ``normalise`` (``/ peak`` where peak > 0).

Writers: ``write_pcm`` goes through the stdlib ``wave`` module (independent of the parser under test);
``wav_bytes`` builds float / f64 / extensible / malformed files with ``struct``.
"""
from __future__ import annotations

import struct
import wave

import numpy as np

U8, S16, S24, S32, F32, F64 = range(6)
BYTES = (1, 2, 3, 4, 4, 8)
NAMES = ("u8", "s16", "s24", "s32", "f32", "f64")
TAG_BITS = {U8: (1, 8), S16: (1, 16), S24: (1, 24), S32: (1, 32), F32: (3, 32), F64: (3, 64)}


# ------------------------------------------------------------------------------------------------ restatement
def decode(raw: bytes, fmt: int, channels: int) -> np.ndarray:
    """Sample bytes -> (frames, channels) f32; trailing bytes short of a whole frame are dropped."""
    fb = BYTES[fmt] * channels
    frames = len(raw) // fb
    raw = bytes(raw[:frames * fb])
    if fmt == U8:
        x = (np.frombuffer(raw, np.uint8).astype(np.float32) - np.float32(128)) / np.float32(128)
    elif fmt == S16:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / np.float32(32768)
    elif fmt == S24:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v).astype(np.int32)
        x = v.astype(np.float32) / np.float32(1 << 23)
    elif fmt == S32:
        x = np.frombuffer(raw, "<i4").astype(np.float32) * np.float32(2.0 ** -31)  # int -> f32 rounds to even
    elif fmt == F32:
        x = np.frombuffer(raw, "<f4").astype(np.float32)
    elif fmt == F64:
        with np.errstate(over="ignore"):
            x = np.frombuffer(raw, "<f8").astype(np.float32)  # rounds to nearest even; Inf above FLT_MAX
    else:
        raise ValueError(fmt)
    return x.reshape(frames, channels)


def downmix(x: np.ndarray) -> np.ndarray:
    """(frames, C) f32 -> (frames,) f32: channels added in order in f32, one division by float(C)."""
    acc = x[:, 0].astype(np.float32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(1, x.shape[1]):
            acc = (acc + x[:, c]).astype(np.float32)
        return (acc / np.float32(x.shape[1])).astype(np.float32)


def peak(mono: np.ndarray) -> np.float32:
    a = np.abs(mono[np.isfinite(mono)])
    return np.float32(a.max()) if a.size else np.float32(0)


def nonfinite(mono: np.ndarray) -> int:
    return int((~np.isfinite(mono)).sum())


def normalise(mono: np.ndarray) -> np.ndarray:
    p = peak(mono)
    if not p > 0:
        return mono.copy()
    with np.errstate(invalid="ignore"):
        return (mono / p).astype(np.float32)


def ingest(raw: bytes, fmt: int, channels: int) -> np.ndarray:
    """decode -> mean -> / peak."""
    return normalise(downmix(decode(raw, fmt, channels)))


# ------------------------------------------------------------------------------------------------ test signals
def random_raw(fmt: int, frames: int, channels: int, seed: int, peak_last: bool = True) -> bytes:
    """Interleaved sample bytes of finite normal values below half scale; with ``peak_last`` every channel of the
    last frame holds one large negative value, the clip's largest |mono sample|."""
    rng = np.random.default_rng(seed)
    n = frames * channels
    if fmt == U8:
        v = rng.integers(64, 192, n).astype(np.uint8)
        if peak_last and frames:
            v[-channels:] = 3
        return v.tobytes()
    if fmt in (S16, S24, S32):
        bits = (16, 24, 32)[fmt - 1]
        half = 1 << (bits - 2)
        v = rng.integers(-half, half, n).astype(np.int64)
        if peak_last and frames:
            v[-channels:] = -(1 << (bits - 1)) + 5
        if fmt == S16:
            return v.astype("<i2").tobytes()
        if fmt == S32:
            return v.astype("<i4").tobytes()
        u = (v & 0xFFFFFF).astype(np.uint32)
        return np.stack([u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF], 1).astype(np.uint8).tobytes()
    v = rng.uniform(0.01, 0.5, n) * rng.choice([-1.0, 1.0], n)
    if peak_last and frames:
        v[-channels:] = -0.875 - 1.0 / 1024
    return v.astype("<f4" if fmt == F32 else "<f8").tobytes()


# ------------------------------------------------------------------------------------------------ writers
def write_pcm(path, raw: bytes, fmt: int, channels: int, rate: int):
    """Integer PCM through the stdlib ``wave`` module."""
    assert fmt in (U8, S16, S24, S32)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(BYTES[fmt])
        w.setframerate(rate)
        w.writeframes(raw)


def fmt_chunk(tag: int, channels: int, rate: int, bits: int, extensible: bool = False, block_align=None,
              sub_tag=None) -> bytes:
    ba = channels * bits // 8 if block_align is None else block_align
    if not extensible:
        body = struct.pack("<HHIIHH", tag, channels, rate, rate * ba, ba, bits)
        if tag != 1:
            body += struct.pack("<H", 0)
        return body
    guid_tail = bytes.fromhex("000000001000800000aa00389b71")
    return (struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * ba, ba, bits)
            + struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag if sub_tag is None else sub_tag) + guid_tail)


def chunk(cid: bytes, body: bytes, declared=None) -> bytes:
    size = len(body) if declared is None else declared
    return cid + struct.pack("<I", size) + body + (b"\0" if len(body) & 1 else b"")


def wav_bytes(fmt_body, raw: bytes, pre=(), post=(), declared=None, riff=b"RIFF", pad_data=True) -> bytes:
    """RIFF/WAVE file bytes: ``pre`` chunks, the fmt chunk (``None`` leaves it out), the data chunk (``raw=None``
    leaves it out; ``declared`` overrides its size field), ``post`` chunks."""
    body = b"WAVE" + b"".join(pre)
    if fmt_body is not None:
        body += chunk(b"fmt ", fmt_body)
    if raw is not None:
        data = b"data" + struct.pack("<I", len(raw) if declared is None else declared) + raw
        if pad_data and len(raw) & 1 and post:
            data += b"\0"
        body += data
    body += b"".join(post)
    return riff + struct.pack("<I", len(body)) + body


def write_any(path, raw: bytes, fmt: int, channels: int, rate: int, **kw):
    """Any of the six formats with a ``struct``-built header."""
    tag, bits = TAG_BITS[fmt]
    with open(path, "wb") as f:
        f.write(wav_bytes(fmt_chunk(tag, channels, rate, bits, extensible=kw.pop("extensible", False)), raw, **kw))
