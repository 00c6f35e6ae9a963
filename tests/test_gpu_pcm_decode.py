"""GPU: mia_pcm_decode / mia_clip_peak / mia_clip_scale (include/miaudio_wav.h) against the numpy restatement of
tests/_wav_ref.py, bit for bit.  Inputs are finite normal values plus the named specials; the sign of a zero result
and subnormal inputs are not pinned (comparisons are value comparisons: +0 == -0, and NaN matches NaN)."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from src.miaudio import kernels as K
from src.miaudio import lib as L
from tests import _wav_ref as R

pytestmark = pytest.mark.gpu

FORMATS = [R.U8, R.S16, R.S24, R.S32, R.F32, R.F64]
FRAMES = [0, 1, 3, 5, 63, 64, 65, 4097]  # 4097: five workgroups' worth of 1024-frame chunks
CANARY = -777.25
CANARY_U32 = 0x5EEDBEEF


def _same(a: np.ndarray, b: np.ndarray) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _peak_f32(peak_bits: torch.Tensor) -> np.ndarray:
    return peak_bits.cpu().numpy().view(np.float32)


def _decode(cuda, clips, byte_offs=None, out_offs=None):
    """clips: [(raw, fmt, channels)] -> (monos, peaks f32, nonfinite) through K.pcm_decode, one launch; the output
    store has guard bands before, after and (where out_offs leave gaps) between the clips, checked here."""
    n = len(clips)
    frames = [len(raw) // (R.BYTES[f] * c) for raw, f, c in clips]
    if byte_offs is None:
        byte_offs, pos = [], 0
        for raw, _, _ in clips:
            byte_offs.append(pos)
            pos += len(raw)
    if out_offs is None:
        out_offs, pos = [], 5
        for m in frames:
            out_offs.append(pos)
            pos += m + 3
    total_bytes = max([o + len(raw) for o, (raw, _, _) in zip(byte_offs, clips)] + [1])
    host = np.full(total_bytes, 0xA5, np.uint8)
    for o, (raw, _, _) in zip(byte_offs, clips):
        host[o:o + len(raw)] = np.frombuffer(raw, np.uint8)
    data = torch.from_numpy(host).to(cuda)
    total_out = max(o + m for o, m in zip(out_offs, frames)) + 7
    out = torch.full((total_out,), CANARY, dtype=torch.float32, device=cuda)
    table = [(o, m, c, f) for o, m, (_, f, c) in zip(byte_offs, frames, clips)]
    peak, nf = K.pcm_decode(data, table, out_offs, out)
    got = out.cpu().numpy()
    untouched = np.ones(total_out, bool)
    monos = []
    for o, m in zip(out_offs, frames):
        monos.append(got[o:o + m].copy())
        untouched[o:o + m] = False
    assert (got[untouched] == np.float32(CANARY)).all(), "a write outside a clip's output range"
    assert peak.shape == (n,) and nf.shape == (n,)
    return monos, _peak_f32(peak), nf.cpu().numpy()


def _check(clips, monos, peaks, nfs):
    for (raw, fmt, ch), mono, pk, nf in zip(clips, monos, peaks, nfs):
        ref = R.downmix(R.decode(raw, fmt, ch)) if len(raw) else np.zeros(0, np.float32)
        what = f"{R.NAMES[fmt]} x{ch}, {len(ref)} frames"
        assert _same(mono, ref), what
        assert pk.view(np.uint32) == R.peak(ref).view(np.uint32), what
        assert nf == R.nonfinite(ref), what


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("fmt", FORMATS, ids=R.NAMES)
def test_formats_channels_frames(cuda, fmt, channels):
    for frames in FRAMES:
        clips = [(R.random_raw(fmt, frames, channels, seed=1000 * fmt + 10 * frames + channels), fmt, channels)]
        monos, peaks, nfs = _decode(cuda, clips)
        _check(clips, monos, peaks, nfs)
        if frames:
            # the largest |sample| is the negative one in the last frame: the peak crossed workgroups and lanes
            assert peaks[0] == -monos[0][-1] and (np.abs(monos[0][:-1]) < peaks[0]).all()
        else:
            assert peaks[0] == 0 and nfs[0] == 0


@pytest.mark.parametrize("fmt,channels", [(R.S24, 2), (R.S16, 1)], ids=["s24x2", "s16x1"])
def test_every_byte_and_output_alignment(cuda, fmt, channels):
    for frames in (5, 65, 1031):
        raw = R.random_raw(fmt, frames, channels, seed=frames)
        for boff in range(4):
            for ooff in range(4):
                clips = [(raw, fmt, channels)]
                monos, peaks, nfs = _decode(cuda, clips, byte_offs=[16 + boff], out_offs=[8 + ooff])
                _check(clips, monos, peaks, nfs)


def test_boundary_values(cuda):
    s24 = b"\x00\x00\x80" + b"\xff\xff\xff" + b"\xff\xff\x7f"
    clips = [(bytes([0, 128, 255]), R.U8, 1),
             (struct.pack("<hh", -32768, 32767), R.S16, 1),
             (s24, R.S24, 1),
             (struct.pack("<iiii", -2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, 2 ** 24 + 3), R.S32, 1),
             (struct.pack("<ddd", 1 + 2.0 ** -30, 1 + 2.0 ** -24, 0.1), R.F64, 1)]
    monos, peaks, nfs = _decode(cuda, clips)
    _check(clips, monos, peaks, nfs)
    assert monos[0].tolist() == [-1.0, 0.0, 127 / 128]
    assert monos[1].tolist() == [-1.0, 32767 / 32768]
    assert monos[2].tolist() == [-1.0, -(2.0 ** -23), 1 - 2.0 ** -23]
    assert monos[3].tolist() == [-1.0, 1.0, 2.0 ** -7, (2 ** 24 + 4) * 2.0 ** -31]  # ties to even
    assert monos[4].tolist() == [1.0, 1.0, float(np.float32(0.1))]  # f64 1 + 2^-24 is a tie: to even
    assert peaks.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0]


def test_nonfinite_samples_are_counted_and_kept_out_of_the_peak(cuda):
    f64 = struct.pack("<dddd", 0.25, 1e39, -0.5, -1e300)          # two above FLT_MAX -> +-Inf
    f32 = struct.pack("<ffff", 0.125, float("nan"), -0.75, 0.5)
    st = struct.pack("<ffffff", 0.5, 0.25, float("inf"), 1.0, -0.25, -0.25)  # stereo: the Inf frame's mean is Inf
    clips = [(f64, R.F64, 1), (f32, R.F32, 1), (st, R.F32, 2)]
    monos, peaks, nfs = _decode(cuda, clips)
    _check(clips, monos, peaks, nfs)
    assert nfs.tolist() == [2, 1, 1] and peaks.tolist() == [0.5, 0.75, 0.375]
    assert np.isinf(monos[0][1]) and np.isnan(monos[1][1])


def test_silent_clip_stays_zero(cuda):
    clips = [(bytes([128] * 70), R.U8, 2), (bytes(3 * 33), R.S24, 1), (R.random_raw(R.S16, 9, 1, seed=4), R.S16, 1)]
    monos, peaks, nfs = _decode(cuda, clips)
    assert peaks[:2].tolist() == [0.0, 0.0] and nfs.tolist() == [0, 0, 0]
    store = torch.from_numpy(np.concatenate(monos)).to(cuda)
    offsets = torch.tensor([0, 35, 68, 77], dtype=torch.int64, device=cuda)
    peak_bits = torch.from_numpy(peaks.view(np.int32).copy()).to(cuda)
    K.clip_scale(store, offsets, peak_bits)
    got = store.cpu().numpy()
    assert (got[:68].view(np.uint32) == 0).all()  # all +0, untouched
    assert _same(got[68:], R.normalise(monos[2]))


def _mixed_clips():
    spec = [(R.U8, 2, 1500), (R.S16, 1, 4097), (R.S24, 2, 777), (R.S32, 3, 64), (R.F32, 2, 2049), (R.F64, 1, 333),
            (R.S24, 1, 1)]
    return [(R.random_raw(f, m, c, seed=50 + i), f, c) for i, (f, c, m) in enumerate(spec)]


def test_one_launch_of_seven_mixed_clips(cuda):
    clips = _mixed_clips()
    byte_offs, pos = [], 3
    for raw, _, _ in clips:  # packed back to back from an odd start: every clip at whatever alignment falls out
        byte_offs.append(pos)
        pos += len(raw)
    monos, peaks, nfs = _decode(cuda, clips, byte_offs=byte_offs)
    _check(clips, monos, peaks, nfs)


def test_guard_bands_through_the_raw_entry_point(cuda):
    """The C entry point on caller-owned buffers: canaries before and after out, between the clips, and around
    peak_bits / nonfinite stay as they were.  Each clip is decoded from a tensor of exactly its size, started at
    0..3 bytes into it, so its last byte is the tensor's last.  That placement cannot by itself catch a read past the
    clip: the caching allocator rounds device blocks up to 512 B, so a few bytes beyond the tensor are still mapped,
    and the frames such bytes would feed are never stored.  That no load leaves the clip rests on the bounds checks
    of fetch_span in csrc/pcmdecode.hip (the whole span on the fast path; every aligned dword, then every byte, on
    the other), not on this test passing."""
    lib = L.load()
    for i, (raw, fmt, ch) in enumerate(_mixed_clips()):
        lead = i % 4
        frames = len(raw) // (R.BYTES[fmt] * ch)
        host = np.concatenate([np.full(lead, 0xA5, np.uint8), np.frombuffer(raw, np.uint8)])
        data = torch.from_numpy(host).to(cuda)  # lead + len(raw) bytes: the clip's last byte is the tensor's last
        assert data.numel() == lead + len(raw)
        out = torch.full((frames + 9,), CANARY, dtype=torch.float32, device=cuda)
        words = torch.tensor([lead, frames, ch | (fmt << 32), 6], dtype=torch.int64, device=cuda)  # clip, out_off
        peak = torch.full((3,), CANARY_U32, dtype=torch.int32, device=cuda)
        nf = peak.clone()
        table = (L.MiaWavClip * 1).from_buffer_copy(words[:3].cpu().numpy().tobytes())
        assert (table[0].byte_off, table[0].frames, table[0].channels, table[0].format) == (lead, frames, ch, fmt)
        L.check(lib.mia_pcm_decode(data.data_ptr(), words.data_ptr(), 1, words[3:].data_ptr(), out.data_ptr(),
                                   peak[1:].data_ptr(), nf[1:].data_ptr(), L.stream_ptr()), "mia_pcm_decode")
        got = out.cpu().numpy()
        ref = R.downmix(R.decode(raw, fmt, ch))
        assert _same(got[6:6 + frames], ref)
        assert (got[:6] == np.float32(CANARY)).all() and (got[6 + frames:] == np.float32(CANARY)).all()
        canary = CANARY_U32
        p, q = peak.cpu().numpy(), nf.cpu().numpy()
        assert p[0] == canary and p[2] == canary and q[0] == canary and q[2] == canary
        assert p[1:2].view(np.float32)[0] == R.peak(ref) and q[1] == 0


def test_argument_errors(cuda):
    data = torch.zeros(64, dtype=torch.uint8, device=cuda)
    out = torch.zeros(64, dtype=torch.float32, device=cuda)
    for clip, msg in [((0, 4, 0, R.S16), "channels"), ((0, 4, 9, R.U8), "channels"), ((0, 4, 1, 6), "format"),
                      ((0, 4, 1, -1), "format"), ((60, 4, 1, R.S16), "leaves data"), ((0, -1, 1, R.S16), "leaves")]:
        with pytest.raises(ValueError, match=msg):
            K.pcm_decode(data, [clip], [0], out)
    with pytest.raises(ValueError, match="leaves out"):
        K.pcm_decode(data, [(0, 8, 1, R.S16)], [60], out)
    with pytest.raises(RuntimeError, match="null pointer"):
        L.check(L.load().mia_pcm_decode(None, None, 1, None, None, None, None, L.stream_ptr()), "mia_pcm_decode")
    peak, nf = K.pcm_decode(data, [], [], out)
    assert peak.numel() == 0 and nf.numel() == 0


def test_eight_channels(cuda):
    clips = [(R.random_raw(R.S16, 130, 8, seed=8), R.S16, 8), (R.random_raw(R.F64, 67, 8, seed=9), R.F64, 8)]
    monos, peaks, nfs = _decode(cuda, clips)
    _check(clips, monos, peaks, nfs)


def test_clip_peak_and_scale_on_a_store(cuda):
    clips = _mixed_clips() + [(struct.pack("<ffff", 0.125, float("nan"), -0.75, 0.5), R.F32, 1)]
    monos, peaks, nfs = _decode(cuda, clips)
    for lead in range(4):  # the store's first clip at every 16-B phase
        lens = [len(m) for m in monos]
        offs = np.concatenate([[lead], lead + np.cumsum(lens)]).astype(np.int64)
        host = np.full(offs[-1] + 5, CANARY, np.float32)
        for o, m in zip(offs, monos):
            host[o:o + len(m)] = m
        store = torch.from_numpy(host).to(cuda)
        offsets = torch.from_numpy(offs).to(cuda)
        pk, nf = K.clip_peak(store, offsets)
        assert np.array_equal(_peak_f32(pk).view(np.uint32), peaks.view(np.uint32))  # what pcm_decode reported
        assert np.array_equal(nf.cpu().numpy(), nfs)
        K.clip_scale(store, offsets, pk)
        got = store.cpu().numpy()
        for o, m in zip(offs, monos):
            assert _same(got[o:o + len(m)], R.normalise(m))
            if len(m) > 1 and np.isfinite(m).all():
                assert np.abs(got[o:o + len(m)]).max() == 1.0
        assert (got[:lead] == np.float32(CANARY)).all() and (got[offs[-1]:] == np.float32(CANARY)).all()


def test_exports_and_signatures():
    header = (L.PKG_ROOT.parent / "include" / "miaudio_wav.h").read_text()
    names = ["mia_pcm_decode", "mia_clip_peak", "mia_clip_scale"]
    exported = L.exported_symbols()
    for name in names:
        assert f"int {name}(" in header and name in L.SIGNATURES and name in exported
    assert "miaudio_wav.h" not in (L.PKG_ROOT.parent / "include" / "miaudio.h").read_text()
    assert C.sizeof(L.MiaWavClip) == 24
