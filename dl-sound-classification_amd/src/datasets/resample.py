"""Batched on-GPU sinc resampling -- replaces ``torchaudio.transforms.Resample`` on the data path
(reference ``resample_waveform``, src/datasets/preprocessing.py:61-76: the first step of
``EnvNetPreprocessor.preprocess`` :822 and ``ASTPreprocessor.preprocess`` :1021).

``sinc_resample_taps`` builds the Hann-windowed sinc filter bank on the host following torchaudio 2.7.1
``_get_sinc_resample_kernel`` (``dtype=None``, ``resampling_method="sinc_interp_hann"``); ``GpuResample`` applies
it with ``mia_resample`` (include/miaudio_resample.h) to a (B, T) batch resident in HBM.  ``ResampledStore`` is the
host-side result of resampling a whole dataset once (ESC50DataModule.setup when the bundles' rate differs from
the preprocessor's).
"""
from __future__ import annotations

import math

import torch

from ..miaudio import kernels as K
from ..miaudio import lib as L


def sinc_resample_taps(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """(taps f32 [n][K], width, o, n) with o, n = orig, new over their gcd and K = 2 * width + o."""
    orig, new = int(orig), int(new)
    if orig < 1 or new < 1 or lowpass_filter_width < 1:
        raise ValueError(f"sinc_resample_taps: orig {orig}, new {new}, lowpass_filter_width {lowpass_filter_width}")
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64)[None] / o
    # an int64 tensor over a python int: float32, as in torchaudio, before the float64 idx promotes it
    t = (torch.arange(0, -n, -1) / n)[:, None] + idx
    t *= base
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base / o
    taps = torch.where(t == 0, torch.tensor(1.0, dtype=t.dtype), t.sin() / t)
    taps *= window * scale
    return taps.to(torch.float32).contiguous(), width, o, n


class GpuResample:
    """``out = resample(x, lengths=None)``: (B, T) or (B, 1, T) f32 CUDA -> (B, Tout) or (B, 1, Tout) f32 CUDA,
    ``Tout = ceil(new * T / orig)``.  With ``lengths`` (B ints) row b holds a clip of ``lengths[b]`` samples: the
    output is that clip's ``ceil(new * lengths[b] / orig)`` samples followed by zeros.  Equal rates return ``x``."""

    def __init__(self, orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
        self.orig, self.new = int(orig), int(new)
        self.taps, self.width, self.o, self.n = sinc_resample_taps(orig, new, lowpass_filter_width, rolloff)
        self.K = self.taps.shape[1]
        self._dev = {}

    def out_len(self, T: int) -> int:
        return -(-self.n * int(T) // self.o)

    def taps_on(self, device) -> torch.Tensor:
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.taps.to(device)
        return self._dev[key]

    def __call__(self, x: torch.Tensor, lengths: torch.Tensor | None = None) -> torch.Tensor:
        L.require_device(x, "GpuResample")
        if self.orig == self.new:
            return x
        if x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[1] != 1):
            raise ValueError(f"GpuResample: expected (B, T) or (B, 1, T), got {tuple(x.shape)}")
        mono = x.dim() == 3
        w = x.reshape(x.shape[0], -1).contiguous().float()
        B, T = w.shape
        Tout = self.out_len(T)
        out = torch.empty(B, Tout, dtype=torch.float32, device=w.device)
        if lengths is not None:
            lengths = torch.as_tensor(lengths).to(device=w.device, dtype=torch.int32).contiguous()
            if lengths.numel() != B:
                raise ValueError(f"GpuResample: {lengths.numel()} lengths for {B} clips")
        lib = L.load()
        with K.probe("resample", 2.0 * self.K * Tout * B, (B * T + B * Tout) * 4):
            L.check(lib.mia_resample(w.data_ptr(), T, B, T, L.ptr(lengths), self.taps_on(w.device).data_ptr(),
                                     self.o, self.n, self.width, out.data_ptr(), Tout, Tout, L.stream_ptr()),
                    "mia_resample")
        return out.view(B, 1, Tout) if mono else out


class ResampledStore:
    """Every clip of a dataset at the target rate: one flat f32 host tensor in shared memory (DataLoader workers
    read it without a copy), per-clip offsets and labels, keyed by the bundle's path."""

    def __init__(self, paths, data: torch.Tensor, offsets, labels, sample_rate: int):
        self.paths = [str(p) for p in paths]
        self.index = {p: i for i, p in enumerate(self.paths)}
        self.data, self.offsets, self.labels, self.sample_rate = data, list(offsets), list(labels), int(sample_rate)

    def __len__(self):
        return len(self.paths)

    @property
    def nbytes(self) -> int:
        return self.data.numel() * 4

    def __contains__(self, path) -> bool:
        return str(path) in self.index

    def get(self, path):
        """((1, T') f32 view of the stored clip, label)."""
        i = self.index[str(path)]
        return self.data[self.offsets[i]:self.offsets[i + 1]].view(1, -1), self.labels[i]


MAX_CLIPS_PER_LAUNCH = 64


def build_store(files, default_rate: int, target: int, device) -> ResampledStore:
    """Resample every bundle of ``files`` once: a bundle's optional integer ``"sample_rate"`` overrides
    ``default_rate`` for that file (mixed-rate datasets); files are grouped by rate, each group goes through
    ``GpuResample`` in launches of at most 64 clips padded to the launch's longest and passed with ``lengths``."""
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"the bundles' sample rate differs from preprocessing_config.sample_rate={target}: "
                         f"resampling runs on the GPU (there is no CPU resampler), but the device is {device}")
    files = list(dict.fromkeys(str(f) for f in files))
    waves, labels, rates = [], [], []
    for f in files:
        b = torch.load(f, map_location="cpu", weights_only=True)
        waves.append(b["waveform"].float().reshape(-1))
        labels.append(int(b["label"]))
        rates.append(int(b.get("sample_rate", default_rate)))
    lens = []
    for w, r in zip(waves, rates):
        g = math.gcd(r, target)
        lens.append(-(-(target // g) * w.numel() // (r // g)))
    offsets = [0]
    for n in lens:
        offsets.append(offsets[-1] + n)
    data = torch.empty(offsets[-1], dtype=torch.float32).share_memory_()
    for rate in sorted(set(rates)):
        ids = [i for i, r in enumerate(rates) if r == rate]
        if rate == target:
            for i in ids:
                data[offsets[i]:offsets[i + 1]] = waves[i]
            continue
        rs = GpuResample(rate, target)
        for s in range(0, len(ids), MAX_CLIPS_PER_LAUNCH):
            part = ids[s:s + MAX_CLIPS_PER_LAUNCH]
            T = max(waves[i].numel() for i in part)
            batch = torch.zeros(len(part), T, dtype=torch.float32)
            for r, i in enumerate(part):
                batch[r, :waves[i].numel()] = waves[i]
            clip_len = torch.tensor([waves[i].numel() for i in part], dtype=torch.int32)
            out = rs(batch.to(device), clip_len).cpu()
            for r, i in enumerate(part):
                data[offsets[i]:offsets[i + 1]] = out[r, :lens[i]]
    store = ResampledStore(files, data, offsets, labels, target)
    print(f"resampled {len(store)} clips to {target} Hz (from {sorted(set(rates))} Hz): "
          f"{store.nbytes / 2**20:.1f} MiB held in host memory")
    return store
