"""RIFF/WAVE container parsing on the host: pure Python (``struct``), no third-party reader.

``parse_wav`` walks the chunks of a ``.wav`` file and says where its sample bytes are and how to read them; the
samples themselves are decoded on the device (``mia_pcm_decode``, include/miaudio_wav.h).  Replaces the container
half of ``torchaudio.load`` in the reference's scripts/prepare_esc50.py.
"""
from __future__ import annotations

import os
import struct
from typing import NamedTuple

from ..miaudio import lib as L

WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT, WAVE_FORMAT_EXTENSIBLE = 1, 3, 0xFFFE
_TAG_NAMES = {2: "MS ADPCM", 6: "A-law", 7: "mu-law", 0x11: "IMA ADPCM", 0x55: "MP3"}


class WavError(ValueError):
    """A file ``parse_wav`` rejects; the message names the file and the reason."""


class WavInfo(NamedTuple):
    format_code: int   # 1 = PCM, 3 = IEEE float (the sub-format of an extensible header)
    channels: int
    sample_rate: int
    bits: int          # container bits per sample (wBitsPerSample)
    frames: int        # whole frames present in the file
    data_offset: int   # byte position of the first sample in the file
    data_bytes: int    # frames * channels * bits / 8

    @property
    def device_format(self) -> int:
        """The ``L.PCM_*`` code ``mia_pcm_decode`` reads these samples with."""
        return _DEVICE_FORMAT[(self.format_code, self.bits)]


_DEVICE_FORMAT = {(1, 8): L.PCM_U8, (1, 16): L.PCM_S16, (1, 24): L.PCM_S24, (1, 32): L.PCM_S32,
                  (3, 32): L.PCM_F32, (3, 64): L.PCM_F64}


def parse_wav(path_or_bytes) -> WavInfo:
    """Parse the header of a WAV file given by path or as ``bytes``.

    Chunks are walked (``fmt `` may follow ``LIST`` / ``JUNK`` / ``bext``; an odd-sized chunk is followed by one pad
    byte; chunks after ``data`` are ignored).  Accepted: PCM at 8 / 16 / 24 / 32 bits, IEEE float at 32 / 64 bits,
    and ``WAVE_FORMAT_EXTENSIBLE`` whose sub-format GUID begins with 1 or 3.  ``frames = min(declared data size,
    bytes left in the file) // block_align``; a declared size of 0 or 0xFFFFFFFF means "to the end of the file".
    Everything else raises ``WavError``."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        name, buf = "<bytes>", bytes(path_or_bytes)
        return _parse(name, len(buf), lambda off, n: buf[off:off + n])
    name = os.fspath(path_or_bytes)
    try:
        size = os.path.getsize(name)
        with open(name, "rb") as f:
            def read(off, n):
                f.seek(off)
                return f.read(n)
            return _parse(name, size, read)
    except OSError as e:
        raise WavError(f"{name}: cannot read: {e}") from e


def _parse(name: str, size: int, read) -> WavInfo:
    def bad(reason):
        return WavError(f"{name}: {reason}")

    head = read(0, 12)
    if len(head) < 12:
        raise bad("not a RIFF/WAVE file (shorter than 12 bytes)")
    if head[:4] in (b"RIFX", b"RF64"):
        raise bad(f"{head[:4].decode()} containers are not supported")
    if head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        raise bad("not a RIFF/WAVE file")
    fmt = None
    pos = 12
    while pos + 8 <= size:
        cid, csize = struct.unpack("<4sI", read(pos, 8))
        body = pos + 8
        if cid == b"fmt ":
            if csize < 16:
                raise bad(f"fmt chunk of {csize} bytes (at least 16)")
            raw = read(body, min(csize, 40))
            if len(raw) < 16:
                raise bad("truncated fmt chunk")
            fmt = raw
        elif cid == b"data":
            if fmt is None:
                raise bad("missing fmt chunk before data")
            return _info(bad, fmt, body, csize, size)
        pos = body + csize + (csize & 1)
    raise bad("missing fmt chunk" if fmt is None else "missing data chunk")


def _info(bad, fmt: bytes, data_offset: int, declared: int, size: int) -> WavInfo:
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40 or struct.unpack("<H", fmt[16:18])[0] < 22:
            raise bad("extensible fmt chunk without a sub-format")
        sub = struct.unpack("<H", fmt[24:26])[0]
        if sub not in (WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT):
            raise bad(f"unsupported extensible sub-format {sub:#x}")
        tag = sub
    if tag not in (WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT):
        what = _TAG_NAMES.get(tag)
        raise bad(f"unsupported format tag {tag:#x}" + (f" ({what})" if what else ""))
    if (tag, bits) not in _DEVICE_FORMAT:
        raise bad(f"unsupported bit depth {bits} for format tag {tag}")
    if channels == 0:
        raise bad("zero channels")
    if block_align != channels * bits // 8:
        raise bad(f"block_align {block_align} != channels {channels} * bits {bits} / 8")
    left = max(0, size - data_offset)
    nbytes = left if declared in (0, 0xFFFFFFFF) else min(declared, left)
    frames = nbytes // block_align
    return WavInfo(tag, channels, rate, bits, frames, data_offset, frames * block_align)
