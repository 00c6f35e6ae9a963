"""Device-resident datasets (``dataset.resident=true``): every clip of a dataset in one flat f32
tensor in HBM, batches cut out of it by ``mia_crop_gather`` (include/miaudio_data.h) -- the reference's zero
padding, short-clip right-padding and crop (src/datasets/preprocessing.py:825, :842-845, :855, :881) as one rule
on the device -- and a loader whose batches never touch the host.

* ``ResidentStore``: the flat store, per-clip offsets and labels (device and host), keyed by the bundle's path.
  Built in one pass over the bundles (``build_resident_store``) or from a ``resample.ResampledStore``.
  ``gather`` cuts pad-and-crop windows out of it, ``fit`` (``mia_fit_gather``) makes whole clips
  one length for the spectrogram path.
* ``max_starts`` / ``center_starts`` / ``multi_crop_starts`` / ``draw_starts``: the reference's crop-start rules
  on tensors (CPU or device).
* ``epoch_indices``: the order of an epoch for this rank.
* ``_ResidentLoader``: ``(x, y)`` batches on the device over an index subset of the store.
"""
from __future__ import annotations

import math

import torch

GIB = float(2 ** 30)


# ------------------------------------------------------------------------------------------------ crop starts
def max_starts(lengths: torch.Tensor, pad: int, window: int) -> torch.Tensor:
    """Largest crop start per clip, ``total - window`` with ``total = len + 2 * pad``; 0 for a short clip
    (``total <= window``: the reference right-pads it and takes it from 0, preprocessing.py:842-845)."""
    return (lengths.long() + (2 * int(pad) - int(window))).clamp_min(0)


def center_starts(lengths: torch.Tensor, pad: int, window: int) -> torch.Tensor:
    """Evaluation crop: ``(total - window) // 2`` (preprocessing.py:853)."""
    return max_starts(lengths, pad, window) // 2


def draw_starts(max_start: torch.Tensor, gen: torch.Generator | None = None) -> torch.Tensor:
    """Training crop: uniform over {0 .. max_start} per clip, ``floor(u * (max_start + 1))`` clamped to
    ``max_start`` with u float64 from ``gen`` on ``max_start``'s device (no host sync).  ``random.randint`` of the
    reference (preprocessing.py:851) in distribution, like every other draw in augment.py."""
    u = torch.rand(max_start.shape, dtype=torch.float64, device=max_start.device, generator=gen)
    return torch.minimum(torch.floor(u * (max_start + 1).double()).long(), max_start.long())


def multi_crop_starts(lengths, pad: int, window: int, test_crops: int):
    """Multi-crop test starts, ``torch.linspace(0, total - window, test_crops).long()`` (preprocessing.py:877)
    called exactly so on the host once per distinct clip length -> ``(starts int32 (N, test_crops), counts int64
    (N,))``; a short clip has one crop at 0 (its row is zeros, its count 1)."""
    lengths = [int(n) for n in torch.as_tensor(lengths).tolist()]
    rows = {}
    for n in set(lengths):
        total = n + 2 * int(pad)
        rows[n] = None if total <= window else torch.linspace(0, total - window, int(test_crops)).long()
    starts = torch.zeros(len(lengths), int(test_crops), dtype=torch.int32)
    counts = torch.ones(len(lengths), dtype=torch.int64)
    for i, n in enumerate(lengths):
        if rows[n] is not None:
            starts[i] = rows[n].to(torch.int32)
            counts[i] = int(test_crops)
    return starts, counts


# ------------------------------------------------------------------------------------------------ epoch order
def epoch_indices(n: int, world: int, rank: int, epoch: int, shuffle: bool, seed: int = 42) -> torch.Tensor:
    """Positions 0..n-1 this rank visits in ``epoch`` (host int64).  World 1: ``torch.randperm`` seeded
    ``seed + epoch`` (as _DeviceLoader) or 0..n-1; world > 1: what ``DistributedSampler(seed=seed,
    drop_last=False)`` over ``range(n)`` yields for this rank and epoch (padded by wrap-around to equal shards)."""
    if world > 1:
        from torch.utils.data.distributed import DistributedSampler
        sampler = DistributedSampler(range(n), num_replicas=world, rank=rank, shuffle=shuffle, seed=seed,
                                     drop_last=False)
        sampler.set_epoch(epoch)
        return torch.tensor(list(sampler), dtype=torch.int64)
    if shuffle:
        return torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch))
    return torch.arange(n)


# ------------------------------------------------------------------------------------------------ the store
class ResidentStore:
    """Every clip of a dataset in HBM: ``data`` flat f32, ``offsets`` int64 [N + 1] and ``labels`` int64 [N] on the
    device, their host copies ``offsets_host`` / ``labels_host`` (lists), and the bundle paths."""

    def __init__(self, paths, data: torch.Tensor, offsets, labels, sample_rate: int):
        self.paths = [str(p) for p in paths]
        self.index = {p: i for i, p in enumerate(self.paths)}
        self.offsets_host = [int(o) for o in offsets]
        self.labels_host = [int(v) for v in labels]
        if len(self.offsets_host) != len(self.paths) + 1 or len(self.labels_host) != len(self.paths) \
                or self.offsets_host[-1] != data.numel():
            raise ValueError("ResidentStore: paths, offsets, labels and data disagree")
        self.data = data
        self.offsets = torch.tensor(self.offsets_host, dtype=torch.int64, device=data.device)
        self.labels = torch.tensor(self.labels_host, dtype=torch.int64, device=data.device)
        self.lengths_host = [b - a for a, b in zip(self.offsets_host[:-1], self.offsets_host[1:])]
        self.lengths = self.offsets[1:] - self.offsets[:-1]
        self.sample_rate = int(sample_rate)

    def __len__(self):
        return len(self.paths)

    @property
    def nbytes(self) -> int:
        return self.data.numel() * 4

    def subset(self, files) -> torch.Tensor:
        """Clip numbers (host int64) of ``files``, in their order."""
        return torch.tensor([self.index[str(f)] for f in files], dtype=torch.int64)

    def gather(self, idx: torch.Tensor, start: torch.Tensor, pad: int, window: int) -> torch.Tensor:
        """``(ncrop, B, window)`` f32: ``K.crop_gather`` on this store (``idx`` int32 [B], ``start`` int32
        [B] or [B, ncrop], both on the device)."""
        from ..miaudio import kernels as K
        return K.crop_gather(self.data, self.offsets, idx, start, pad, window)

    def fit(self, idx: torch.Tensor, length: int, mode: str = "wrap") -> torch.Tensor:
        """``(B, length)`` f32: ``K.fit_gather`` on this store (``idx`` int32 [B] on the device) -- every clip
        trimmed about its centre, wrapped (``mode="wrap"``) or zero-padded (``"zero"``) to ``length`` samples."""
        from ..miaudio import kernels as K
        return K.fit_gather(self.data, self.offsets, idx, length, mode)


def _check_cap(nbytes: int, max_gib: float):
    if nbytes > float(max_gib) * GIB:
        raise ValueError(f"the resident store needs {nbytes / GIB:.2f} GiB, more than resident_max_gib={max_gib}: "
                         f"raise dataset.resident_max_gib or set dataset.resident=false")


def _require_cuda(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"dataset.resident=true keeps the clips in HBM and crops them with a HIP kernel (there is "
                         f"no CPU path), but the device is {device}: set dataset.resident=false")
    return device


def build_resident_store(files, sample_rate: int, device, max_gib: float = 8.0) -> ResidentStore:
    """One pass over the bundles: each file is read once, for both waveform and label."""
    device = _require_cuda(device)
    files = list(dict.fromkeys(str(f) for f in files))
    waves, labels, offsets = [], [], [0]
    for f in files:
        b = torch.load(f, map_location="cpu", weights_only=True)
        waves.append(b["waveform"].float().reshape(-1))
        labels.append(int(b["label"]))
        offsets.append(offsets[-1] + waves[-1].numel())
        _check_cap(offsets[-1] * 4, max_gib)
    data = torch.empty(offsets[-1], dtype=torch.float32, device=device)
    for i, w in enumerate(waves):
        data[offsets[i]:offsets[i + 1]].copy_(w)
    store = ResidentStore(files, data, offsets, labels, sample_rate)
    print(f"resident store: {len(store)} clips at {sample_rate} Hz, {store.nbytes / 2**20:.1f} MiB held in HBM")
    return store


def from_resampled(rs, device, max_gib: float = 8.0) -> ResidentStore:
    """Upload a ``resample.ResampledStore`` (flat tensor and offsets) as it is: nothing is resampled twice."""
    device = _require_cuda(device)
    _check_cap(rs.nbytes, max_gib)
    store = ResidentStore(rs.paths, rs.data.to(device), rs.offsets, rs.labels, rs.sample_rate)
    print(f"resident store: {len(store)} clips at {store.sample_rate} Hz, {store.nbytes / 2**20:.1f} MiB held in HBM")
    return store


# ------------------------------------------------------------------------------------------------ the loader
class _ResidentLoader:
    """Batches cut from a ``ResidentStore`` on the device: ``x`` (B, 1, window) f32 and ``y`` (B,) int64, or under
    ``mode="multi"`` ``x`` a list of ``ncrop`` (B, 1, window) views of one (ncrop, B, window) output.

    ``subset``: the clip numbers this loader serves (host int64).  ``mode``: ``"random"`` (training crop),
    ``"center"`` (evaluation crop), ``"multi"`` (multi-crop test, ``table`` = the store-wide (N, test_crops) int32
    device table and ``counts`` its host crop counts), ``"whole"`` (AST: whole clips of one length) or ``"fit"``
    (AST with ``preprocessing_config.clip_length``: every clip fitted to ``window`` samples by ``store.fit`` under
    ``fit_mode``; no starts).  The epoch's order, clip numbers, labels and starts are formed once in ``__iter__``; a
    batch is then slices of them and one kernel launch.  ``last_index`` / ``last_start`` hold the most recent
    batch's clip numbers (int32 [B]) and starts (int32 [B], or [B, ncrop] under "multi"; None under "fit")."""

    def __init__(self, store: ResidentStore, subset: torch.Tensor, batch_size: int, mode: str, pad: int,
                 window: int, shuffle: bool, seed: int = 42, world: int = 1, rank: int = 0,
                 gen: torch.Generator | None = None, table: torch.Tensor | None = None,
                 counts: torch.Tensor | None = None, fit_mode: str = "wrap"):
        if mode not in ("random", "center", "multi", "whole", "fit"):
            raise ValueError(f"_ResidentLoader: mode {mode!r}")
        self.store, self.bs, self.mode, self.shuffle, self.seed = store, int(batch_size), mode, shuffle, seed
        self.world, self.rank, self.epoch, self.gen = world, rank, 0, gen
        self.n = int(subset.numel())
        if self.n < 1:
            raise ValueError("_ResidentLoader: empty subset")
        self.pad, self.window, self.ncrop, self.fit_mode = int(pad), int(window), 1, fit_mode
        lens = torch.tensor([store.lengths_host[i] for i in subset.tolist()], dtype=torch.int64)
        if mode == "whole":
            if int(lens.min()) != int(lens.max()):
                raise ValueError(f"resident AST mode serves whole clips as one (B, 1, T) batch, but the clip lengths "
                                 f"range from {int(lens.min())} to {int(lens.max())} samples")
            self.pad, self.window = 0, int(lens[0])
        dev = store.data.device
        self.clip = subset.to(device=dev, dtype=torch.int32)
        self.labels = store.labels[subset.to(dev)]
        self.start = None
        if mode == "random":
            self.max_start = max_starts(lens, self.pad, self.window).to(dev)
        elif mode == "center":
            self.start = center_starts(lens, self.pad, self.window).to(device=dev, dtype=torch.int32)
        elif mode == "whole":
            self.start = torch.zeros(self.n, dtype=torch.int32, device=dev)
        elif mode == "multi":
            c = counts[subset]
            if int(c.min()) != int(c.max()):
                raise ValueError(f"multi-crop test: the set mixes clips with 1 crop (len + 2 * pad <= window = "
                                 f"{self.window}) and clips with {int(c.max())} crops; a batch cannot hold both")
            self.ncrop = int(c[0])
            self.start = table[subset.to(dev)][:, :self.ncrop].contiguous()
        self.last_index = self.last_start = None

    def set_epoch(self, e):
        self.epoch = e

    def _index(self) -> torch.Tensor:
        return epoch_indices(self.n, self.world, self.rank, self.epoch, self.shuffle, self.seed)

    def __len__(self):
        per_rank = math.ceil(self.n / self.world) if self.world > 1 else self.n
        return max(1, math.ceil(per_rank / self.bs))

    def __iter__(self):
        order = self._index().to(self.clip.device)
        clip, labels = self.clip[order], self.labels[order]
        if self.mode == "fit":
            for i in range(0, order.numel(), self.bs):
                idx = clip[i:i + self.bs]
                out = self.store.fit(idx, self.window, self.fit_mode)
                self.last_index, self.last_start = idx, None
                yield out.unsqueeze(1), labels[i:i + self.bs]
            return
        if self.mode == "random":
            start = draw_starts(self.max_start[order], self.gen).to(torch.int32)
        else:
            start = self.start[order]
        for i in range(0, order.numel(), self.bs):
            idx, st = clip[i:i + self.bs], start[i:i + self.bs]
            out = self.store.gather(idx, st, self.pad, self.window)
            self.last_index, self.last_start = idx, st
            if self.mode == "multi":
                yield [out[c].unsqueeze(1) for c in range(self.ncrop)], labels[i:i + self.bs]
            else:
                yield out[0].unsqueeze(1), labels[i:i + self.bs]
