"""WAV files -> peak-normalised mono f32 clips in HBM.

The host parses the containers (``wav.parse_wav``) and reads each file's ``data`` bytes into a pinned staging
buffer; everything per sample runs on the device: ``mia_pcm_decode`` (unpack, scale, downmix, peak), the existing
``GpuResample`` where a target rate is set, ``mia_clip_peak`` after it, and ``mia_clip_scale``.  Replaces
``torchaudio.load`` + ``torch.mean(dim=0)`` + ``wave / wave.abs().max()`` of the reference's
scripts/prepare_esc50.py.  There is no CPU path.

Order of operations under ``target_rate``: the reference resamples each channel and then averages them; here the
channels are averaged by the decode kernel and the mono clip is resampled.  Resampling is linear, so the two
orders are equal in exact arithmetic and differ only in f32 rounding, and this order does half the filter work on
a stereo file.
"""
from __future__ import annotations

import os

import torch

from ..miaudio import kernels as K
from ..miaudio import lib as L
from .resample import MAX_CLIPS_PER_LAUNCH, GpuResample
from .wav import WavError, parse_wav

MIB = 1 << 20
STAGE_ALIGN = 16  # every clip's bytes start on a 16-B boundary of the staging buffer


def _require_cuda(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"WAV ingestion decodes, downmixes and normalises the samples with HIP kernels (there is no "
                         f"CPU path), but the device is {device}: run it on a machine with a GPU")
    return device


def plan_groups(nbytes, max_stage_bytes: int):
    """Clips (by their data sizes, in order) -> groups ``[(clip numbers, staging offsets, group bytes)]``: each
    clip starts on a 16-B boundary and a group stays within ``max_stage_bytes`` unless a single clip exceeds it."""
    groups, ids, offs, used = [], [], [], 0
    for i, n in enumerate(nbytes):
        start = -(-used // STAGE_ALIGN) * STAGE_ALIGN
        if ids and start + n > max_stage_bytes:
            groups.append((ids, offs, used))
            ids, offs, start = [], [], 0
        ids.append(i)
        offs.append(start)
        used = start + n
    if ids:
        groups.append((ids, offs, used))
    return groups


def ingest_wavs(paths, device, target_rate: int | None = None, max_stage_bytes: int = 256 * MIB,
                strict: bool = False):
    """-> ``(store, offsets, rates, skipped)``.

    ``store``: flat f32 device tensor; clip i (the i-th of ``paths``) is ``store[offsets[i]:offsets[i + 1]]``, mono,
    divided by its peak (a silent clip stays zeros), at ``rates[i]`` Hz -- its file's rate, or ``target_rate`` where
    that is set (clips at another rate are resampled after the downmix; length ``ceil(new * len / orig)``).
    ``offsets``: host list of ``len(paths) + 1`` ints.  ``skipped``: ``[(i, path, reason)]`` for files the parser
    rejects, files with no whole frame or more than 8 channels (all three have length 0 in the store), and clips
    that hold NaN / Inf samples or whose file shrank between parsing and reading (left in the store; not to be
    used).  ``strict=True`` raises ``WavError`` on the first of them instead."""
    device = _require_cuda(device)
    paths = [os.fspath(p) for p in paths]
    n = len(paths)
    skipped = []

    def skip(i, reason):
        if strict:
            raise WavError(f"{paths[i]}: {reason}" if not reason.startswith(paths[i]) else reason)
        skipped.append((i, paths[i], reason))

    infos = [None] * n
    for i, p in enumerate(paths):
        try:
            info = parse_wav(p)
        except WavError as e:
            skip(i, str(e))
            continue
        if info.channels > L.WAV_MAX_CHANNELS:
            skip(i, f"{info.channels} channels (at most {L.WAV_MAX_CHANNELS})")
        elif info.frames == 0:
            skip(i, "no whole frame of samples")
        else:
            infos[i] = info
    kept = [i for i in range(n) if infos[i] is not None]

    # ---- decode at the native rates: groups of files through one pinned buffer, one upload + one launch each
    native = [0]
    for i in kept:
        native.append(native[-1] + infos[i].frames)
    dec = torch.empty(native[-1], dtype=torch.float32, device=device)
    peak = torch.zeros(len(kept), dtype=torch.int32, device=device)
    bad = torch.zeros(len(kept), dtype=torch.int32, device=device)
    groups = plan_groups([infos[i].data_bytes for i in kept], int(max_stage_bytes))
    cap = max((g[2] for g in groups), default=0)
    pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
    stage = torch.empty(cap, dtype=torch.uint8, device=device)
    view = memoryview(pinned.numpy()) if cap else None
    uploaded = None
    for ids, offs, used in groups:
        if uploaded is not None:
            uploaded.synchronize()  # the previous group has left the pinned buffer
        for k, off in zip(ids, offs):
            info = infos[kept[k]]
            with open(paths[kept[k]], "rb") as f:
                f.seek(info.data_offset)
                got = f.readinto(view[off:off + info.data_bytes])
            if got != info.data_bytes:  # the file shrank since it was parsed: the rest decodes as zero bytes
                view[off + got:off + info.data_bytes] = bytes(info.data_bytes - got)
                skip(kept[k], f"read {got} of {info.data_bytes} data bytes (the file changed)")
        stage[:used].copy_(pinned[:used], non_blocking=True)
        uploaded = torch.cuda.Event()
        uploaded.record()
        clips = [(off, infos[kept[k]].frames, infos[kept[k]].channels, infos[kept[k]].device_format)
                 for k, off in zip(ids, offs)]
        pk, nf = K.pcm_decode(stage[:used], clips, [native[k] for k in ids], dec)
        peak[ids[0]:ids[-1] + 1] = pk
        bad[ids[0]:ids[-1] + 1] = nf

    # ---- bring every clip to target_rate (mono, after the downmix), then the peak of what came out
    rates = [infos[i].sample_rate for i in kept]
    if target_rate is not None and any(r != int(target_rate) for r in rates):
        target = int(target_rate)
        rs_by_rate = {r: GpuResample(r, target) for r in sorted(set(rates)) if r != target}
        lens = [native[k + 1] - native[k] if r == target else rs_by_rate[r].out_len(native[k + 1] - native[k])
                for k, r in enumerate(rates)]
        final = [0]
        for m in lens:
            final.append(final[-1] + m)
        store = torch.empty(final[-1], dtype=torch.float32, device=device)
        for rate in sorted(set(rates)):
            ks = [k for k, r in enumerate(rates) if r == rate]
            if rate == target:
                for k in ks:
                    store[final[k]:final[k + 1]].copy_(dec[native[k]:native[k + 1]])
                continue
            for s in range(0, len(ks), MAX_CLIPS_PER_LAUNCH):
                part = ks[s:s + MAX_CLIPS_PER_LAUNCH]
                T = max(native[k + 1] - native[k] for k in part)
                batch = torch.zeros(len(part), T, dtype=torch.float32, device=device)
                for r, k in enumerate(part):
                    batch[r, :native[k + 1] - native[k]].copy_(dec[native[k]:native[k + 1]])
                clip_len = torch.tensor([native[k + 1] - native[k] for k in part], dtype=torch.int32)
                out = rs_by_rate[rate](batch, clip_len)
                for r, k in enumerate(part):
                    store[final[k]:final[k + 1]].copy_(out[r, :lens[k]])
        off_dev = torch.tensor(final, dtype=torch.int64, device=device)
        peak, bad2 = K.clip_peak(store, off_dev)
        bad = bad + bad2
        rates = [target] * len(kept)
    else:
        store, final = dec, native
        off_dev = torch.tensor(final, dtype=torch.int64, device=device)
    K.clip_scale(store, off_dev, peak)

    already = {i for i, _, _ in skipped}
    for k, c in enumerate(bad.tolist()):
        if c and kept[k] not in already:
            skip(kept[k], f"{c} non-finite (NaN / Inf) samples")
    # offsets and rates over all of paths: a file that never reached the device has length 0 and rate 0
    offsets, all_rates, k = [0], [0] * n, 0
    for i in range(n):
        if infos[i] is not None:
            offsets.append(final[k + 1])
            all_rates[i] = rates[k]
            k += 1
        else:
            offsets.append(offsets[-1])
    skipped.sort()
    return store, offsets, all_rates, skipped
