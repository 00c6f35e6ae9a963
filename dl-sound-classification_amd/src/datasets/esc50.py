"""ESC-50 Dataset / DataModule — drop-in for the reference ``src.datasets.esc50``
(ESC50DataModule ctor kwargs, config-constraint validation, 5-fold split with a stratified
validation split, reference src/datasets/esc50.py:335-629) with the per-clip feature work moved
onto the GPU:

* The Dataset only reads the ``{"waveform": (1, T) f32, "label": int}`` bundles written by
  scripts/prepare_esc50.py (torch.load(weights_only=True)) and, for EnvNet without BC mixing, pads
  T/2 each side and crops (random for training, centre otherwise — preprocessing.py:814-855).
* ``gpu_transform`` runs inside the training step on the device: BC mixing against the resident
  training-set pool (EnvNet) or the batched HIP log-mel -> SpecAugment -> Mixup against the
  resident un-augmented spectrogram pool (AST).  Labels become the same soft (B, C) f32 targets the
  reference produces, so LitClassifier's soft-label loss branch runs as in the reference.
* When ``preprocessing_config.sample_rate`` differs from the data module's ``sample_rate`` the clips are
  resampled first, as the reference's preprocessors do (preprocessing.py:822, :1021): once, on the GPU, in
  ``setup()`` (``resample.build_store``); window, padding and the log-mel filter bank are then in target-rate
  terms.  With equal rates (the default: the target falls back to the data module's rate) nothing changes.
* ``resident=True`` (off by default) keeps every clip in HBM (``resident.ResidentStore``, one pass
  over the bundles) and serves the three loaders from it: the pad, the crops and the multi-crop test are one HIP
  gather per batch (``mia_crop_gather``) and no batch touches the host.  Labels and the augmentation pool then come
  from the store as well.
* ``preprocessing_config.clip_length`` (seconds; off by default) fits every clip of the spectrogram
  path to one length -- centred trim, wrap or zero padding (``clip_fit``), the reference's
  src/utils/audio.py::pad_or_trim -- so clips of different lengths batch: ``fit_clip`` in the Dataset on the host
  path, ``mia_fit_gather`` per batch on the resident store.  Without it the clips are served whole, as before.
``SyntheticDataModule`` serves device-resident synthetic clips (benchmarks, plumbing runs).
"""
from __future__ import annotations

import math
import random
from pathlib import Path
from typing import Dict, List, Sequence, Union

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

SR = 44_100
CLIP_FITS = ("wrap", "zero")
# the shortest waveform GpuLogMel takes: its reflect padding of n_fft / 2 = 512 samples each side needs T > 512
# (csrc/logmel.hip, mia_logmel_fwd)
MIN_LOGMEL_SAMPLES = 513


def fit_clip(w: torch.Tensor, length: int, mode: str = "wrap") -> torch.Tensor:
    """``w`` (..., n) made exactly ``length`` samples long, the rule of the reference's
    src/utils/audio.py::pad_or_trim (``mia_fit_gather`` is the same rule on the resident store):
    n > length keeps the ``length`` samples from ``(n - length) // 2``; a shorter clip is repeated
    (``mode="wrap"``: ``out[t] = w[t mod n]``) or followed by +0.0 (``mode="zero"``); an empty clip gives +0.0
    (the reference would divide by zero).  Samples are copied, never computed with: they keep their bits."""
    if mode not in CLIP_FITS:
        raise ValueError(f"fit_clip: mode {mode!r} is not one of {CLIP_FITS}")
    length, n = int(length), w.shape[-1]
    if length < 1:
        raise ValueError(f"fit_clip: length {length} < 1")
    if n == length:
        return w
    if n > length:
        start = (n - length) // 2
        return w[..., start:start + length]
    if n > 0 and mode == "wrap":
        return w[..., torch.arange(length, device=w.device) % n]
    out = torch.zeros(*w.shape[:-1], length, dtype=w.dtype, device=w.device)
    out[..., :n] = w
    return out


def _collate_whole_clips(batch):
    """The default collate for whole ``"ast"``-mode clips; clips of different lengths cannot be stacked, and the
    error says which key makes them one length."""
    lens = sorted({b[0].shape[-1] for b in batch})
    if len(lens) > 1:
        raise ValueError(f"the spectrogram path stacks whole clips, but this batch holds clips of {lens[0]} .. "
                         f"{lens[-1]} samples: set model.dataset_overrides.preprocessing_config.clip_length "
                         f"(seconds) to fit every clip to one length")
    return torch.utils.data.default_collate(batch)


def _one_hot(y: torch.Tensor, C: int) -> torch.Tensor:
    out = torch.zeros(y.numel(), C, dtype=torch.float32, device=y.device)
    out.scatter_(1, y.long().view(-1, 1), 1.0)
    return out


class ESC50Dataset(Dataset):
    def __init__(self, root, folds: Sequence[int] = (), files: List[Path] | None = None, mode: str = "envnet_v2",
                 pad_crop: bool = False, window_length: float = 5.0, padding_ratio: float = 0.5,
                 training: bool = True, multi_crop_test: bool = False, test_crops: int = 10,
                 sample_rate: int = SR, store=None, fit_length: int | None = None, clip_fit: str = "wrap"):
        """``sample_rate``: the rate the window and the padding are counted in.  ``store``: a
        ``resample.ResampledStore`` that already holds every clip at that rate; ``load`` then reads from it
        instead of the bundle.  ``fit_length``: in ``"ast"`` mode, the samples every clip is fitted to
        (``fit_clip`` under ``clip_fit``); None serves the clips whole."""
        self.root = Path(root)
        if files is not None:
            self.files = list(files)
        else:
            self.files = []
            for f in folds:
                self.files += sorted((self.root / f"fold_{f}").glob("*.pt"))
        if not self.files:
            raise FileNotFoundError(f"No .pt files found in {self.root}; did you run scripts/prepare_esc50.py?")
        self.mode, self.pad_crop, self.training = mode, pad_crop, training
        self.window = int(window_length * sample_rate)
        self.store = store
        self.pad = int(self.window * padding_ratio)
        self.multi_crop_test, self.test_crops = multi_crop_test, test_crops
        self.fit_length = int(fit_length) if fit_length is not None and mode == "ast" else None
        self.clip_fit = clip_fit

    def __len__(self):
        return len(self.files)

    def load(self, idx):
        if self.store is not None:
            return self.store.get(self.files[idx])
        b = torch.load(self.files[idx], map_location="cpu", weights_only=True)
        return b["waveform"].float().reshape(1, -1), int(b["label"])

    def clip(self, idx):
        """``load``, with the clip fitted to ``fit_length`` when one was given (``"ast"`` mode): what
        ``__getitem__`` serves and the Mixup pool holds."""
        w, label = self.load(idx)
        if self.fit_length is not None:
            w = fit_clip(w, self.fit_length, self.clip_fit)
        return w, label

    def _crop(self, w, start):
        return w[..., start:start + self.window]

    def fit_window(self, w):
        """A raw clip as the BC-mixing partner pool holds it: its first ``window`` samples, zero-padded
        on the right when shorter (the reference mixes against the raw partner and truncates both to
        the shorter length, BCMixingUtils.mix_waveforms preprocessing.py:462-466; ESC-50 clips are
        exactly one window, so this is the identity there)."""
        w = w[..., :self.window]
        return torch.nn.functional.pad(w, (0, self.window - w.shape[-1])) if w.shape[-1] < self.window else w

    def __getitem__(self, idx):
        w, label = self.clip(idx)
        if self.mode == "envnet_v2" and not self.pad_crop:
            # BC-mixing path: no T/2 padding, but the reference's random_crop still runs
            # (esc50.py:233-234, preprocessing.py:841-855): a shorter clip (UrbanSound8K's <= 4 s) is
            # right-padded to the window, a longer one cropped (random when training, else centred)
            total = w.shape[-1]
            if total <= self.window:
                return torch.nn.functional.pad(w, (0, self.window - total)), label
            start = random.randint(0, total - self.window) if self.training else (total - self.window) // 2
            return self._crop(w, start), label
        if self.mode == "envnet_v2" and self.pad_crop:
            w = torch.nn.functional.pad(w, (self.pad, self.pad))
            total = w.shape[-1]
            if total <= self.window:
                return torch.nn.functional.pad(w, (0, self.window - total)), label
            if not self.training and self.multi_crop_test:
                starts = torch.linspace(0, total - self.window, self.test_crops).long()
                return [self._crop(w, int(s)) for s in starts], label
            start = random.randint(0, total - self.window) if self.training else (total - self.window) // 2
            w = self._crop(w, start)
        return w, label


class ESC50DataModule:
    NUM_FOLDS = 5

    def __init__(self, root: str, fold: int = 0, sample_rate: int = SR, n_mels: int = 128, val_split: float = 0.1,
                 batch_size: int = 32, num_workers: int = 4, is_spectrogram: bool = False,
                 enable_bc_mixing: bool = False, enable_mixup: bool = False, mixup_alpha: float = 0.5,
                 time_mask: Union[bool, int] = False, freq_mask: Union[bool, int] = False,
                 preprocessing_mode: str = "envnet_v2", preprocessing_config: Dict | None = None,
                 num_classes: int = 50, augment: Dict | None = None, resident: bool = False,
                 resident_max_gib: float = 8.0, **unused):
        if not (0 <= fold < self.NUM_FOLDS):
            raise ValueError(self._fold_error())
        self._validate_config_constraints(is_spectrogram, enable_bc_mixing, enable_mixup, time_mask, freq_mask)
        augment = dict(augment or {})
        if time_mask is not False:
            augment["time_mask"] = time_mask
        if freq_mask is not False:
            augment["freq_mask"] = freq_mask
        self.root, self.fold, self.sample_rate, self.n_mels = root, fold, sample_rate, n_mels
        self.val_split, self.batch_size, self.num_workers = val_split, batch_size, num_workers
        self.is_spectrogram = is_spectrogram
        self.enable_bc_mixing, self.enable_mixup, self.mixup_alpha = enable_bc_mixing, enable_mixup, mixup_alpha
        self.augment = augment
        self.preprocessing_mode = "ast" if is_spectrogram else "envnet_v2"
        self.preprocessing_config = dict(preprocessing_config or {})
        self.num_classes = num_classes
        self.fit_length, self.clip_fit = self._clip_fitting()
        self.device, self.world, self.rank = torch.device("cpu"), 1, 0
        self._train_set = self._val_set = self._test_set = None
        self._pool = self._pool_labels = None
        self._logmel = None
        self._gen = None
        self._store = None
        # resident=True: the clips live in HBM (resident.ResidentStore), the three loaders are
        # _ResidentLoader objects and batches never touch the host.  Off by default: nothing changes then.
        self.resident, self.resident_max_gib = bool(resident), float(resident_max_gib)
        self._rstore = self._crop_gen = self._crop_table = None
        self._loaders = {}

    @property
    def target_rate(self) -> int:
        """The rate the preprocessor works at (reference EnvNetPreprocessor / ASTPreprocessor ``sample_rate``).
        Defaults to the data module's own rate, not to the reference's 44100: every configuration that names no
        preprocessing_config.sample_rate stays on the path without resampling."""
        return int(self.preprocessing_config.get("sample_rate", self.sample_rate))

    def _clip_fitting(self):
        """``(fit_length, clip_fit)`` from ``preprocessing_config.clip_length`` (seconds; absent or null: off, the
        clips are served whole) and ``.clip_fit``: the spectrogram path's clips fitted to
        ``int(clip_length * target_rate)`` samples (``fit_clip`` / ``mia_fit_gather``)."""
        pc = self.preprocessing_config
        mode = pc.get("clip_fit", "wrap")
        if mode not in CLIP_FITS:
            raise ValueError(f"preprocessing_config.clip_fit must be one of {CLIP_FITS}, got {mode!r}")
        seconds = pc.get("clip_length")
        if seconds is None:
            return None, mode
        if not self.is_spectrogram:
            raise ValueError("preprocessing_config.clip_length fits the clips of the spectrogram path "
                             "(is_spectrogram=true); with is_spectrogram=false window_length pads and crops every "
                             "clip already")
        length = int(float(seconds) * self.target_rate)
        if length < MIN_LOGMEL_SAMPLES:
            raise ValueError(f"preprocessing_config.clip_length={seconds} s is {length} samples at "
                             f"{self.target_rate} Hz, but the log-mel kernel's reflect padding needs at least "
                             f"{MIN_LOGMEL_SAMPLES} (more than n_fft / 2 = 512)")
        return length, mode

    @classmethod
    def _fold_error(cls) -> str:
        return "fold must be 0…4 (ESC-50 uses five folds)."

    @staticmethod
    def _validate_config_constraints(is_spectrogram, enable_bc_mixing, enable_mixup, time_mask, freq_mask):
        """Same constraints and messages as the reference (esc50.py:437-476)."""
        errors = []
        if is_spectrogram and enable_bc_mixing:
            errors.append("enable_bc_mixing cannot be true when is_spectrogram=true (BC mixing is only for waveform mode)")
        if not is_spectrogram and enable_mixup:
            errors.append("enable_mixup can only be true when is_spectrogram=true (Mixup is only for spectrogram mode)")
        if not is_spectrogram:
            if time_mask is not False and time_mask != 0:
                errors.append("time_mask will be ignored when is_spectrogram=false (SpecAugment is only for spectrogram mode)")
            if freq_mask is not False and freq_mask != 0:
                errors.append("freq_mask will be ignored when is_spectrogram=false (SpecAugment is only for spectrogram mode)")
        if is_spectrogram:
            for name, v in (("time_mask", time_mask), ("freq_mask", freq_mask)):
                if v is not False and not isinstance(v, int):
                    errors.append(f"{name} must be False or a positive integer")
                if isinstance(v, int) and not isinstance(v, bool) and v < 0:
                    errors.append(f"{name} must be a positive integer")
        if errors:
            raise ValueError("Configuration validation failed:\n" + "\n".join(f"  • {e}" for e in errors))

    # -------------------------------------------------------------------- setup
    def attach(self, device, world: int = 1, rank: int = 0):
        self.device, self.world, self.rank = torch.device(device), world, rank

    def _ds(self, **kw):
        pc = self.preprocessing_config
        if self.target_rate != self.sample_rate:  # window and padding in target-rate samples, clips from the store
            kw = dict(kw, sample_rate=self.target_rate, store=self._store)
        return ESC50Dataset(self.root, mode=self.preprocessing_mode,
                            window_length=pc.get("window_length", 5.0), padding_ratio=pc.get("padding_ratio", 0.5),
                            multi_crop_test=pc.get("multi_crop_test", False), test_crops=pc.get("test_crops", 10),
                            fit_length=self.fit_length, clip_fit=self.clip_fit, **kw)

    def setup(self, stage: str | None = None) -> None:
        if self._train_set is not None:
            return
        if self.resident and self.device.type != "cuda":
            raise ValueError(f"dataset.resident=true keeps the clips in HBM and crops them with a HIP kernel (there "
                             f"is no CPU path), but the device is {self.device}: set dataset.resident=false")
        from sklearn.model_selection import StratifiedShuffleSplit
        train_folds = [f for f in range(self.NUM_FOLDS) if f != self.fold]
        if self.target_rate != self.sample_rate:
            # the reference's order (preprocessing.py:822, :1021): resample the whole clip first, then pad and crop
            # in target-rate samples.  One pass over every file; the three datasets read the result.
            from .resample import build_store
            every = ESC50Dataset(self.root, folds=list(range(self.NUM_FOLDS))).files
            self._store = build_store(every, self.sample_rate, self.target_rate, self.device)
        full = self._ds(folds=train_folds, training=True)
        if self.resident:
            # one pass over the files (or none after the resampler's): waveforms and labels both come from the store
            from . import resident as R
            if self._store is not None:
                self._rstore = R.from_resampled(self._store, self.device, self.resident_max_gib)
            else:
                every = ESC50Dataset(self.root, folds=list(range(self.NUM_FOLDS))).files
                self._rstore = R.build_resident_store(every, self.target_rate, self.device, self.resident_max_gib)
            labels = [self._rstore.labels_host[self._rstore.index[str(f)]] for f in full.files]
        else:
            labels = [full.load(i)[1] for i in range(len(full))]
        val_size = math.ceil(len(full) * self.val_split)
        splitter = StratifiedShuffleSplit(n_splits=1, test_size=val_size, random_state=42)
        tr, va = next(splitter.split(np.zeros(len(labels)), labels))
        tr_files = [full.files[i] for i in tr]
        va_files = [full.files[i] for i in va]
        if set(tr_files) & set(va_files):
            raise RuntimeError("Data leakage detected between train and val splits")
        pad_crop = not self.enable_bc_mixing  # reference: BC mixing path skips pad + crop
        self._train_set = self._ds(files=tr_files, training=True, pad_crop=pad_crop)
        self._val_set = self._ds(files=va_files, training=False, pad_crop=True)
        self._test_set = self._ds(folds=[self.fold], training=False, pad_crop=True)
        self._train_labels = [labels[i] for i in tr]
        ds = self._test_set
        if self.resident and not self.is_spectrogram and ds.multi_crop_test:
            # the multi-crop starts of every clip: torch.linspace on the host once per distinct length
            from .resident import multi_crop_starts
            starts, counts = multi_crop_starts(self._rstore.lengths_host, ds.pad, ds.window, ds.test_crops)
            self._crop_table = (starts.to(self.device), counts)

    def _pools(self):
        """Resident augmentation pool on the device (reference preloads it for BC/Mixup, esc50.py:167-187)."""
        if self._pool is not None or not (self.enable_bc_mixing or self.enable_mixup):
            return
        ds = self._train_set
        if self.resident:
            waves = self._resident_pool_waves(ds)
        elif self.is_spectrogram:
            waves = torch.stack([ds.clip(i)[0][0] for i in range(len(ds))]).to(self.device)
        else:
            waves = torch.stack([ds.fit_window(ds.load(i)[0])[0] for i in range(len(ds))]).to(self.device)
        self._pool_labels = torch.tensor(self._train_labels, dtype=torch.int64, device=self.device)
        if self.is_spectrogram:
            lm = self.logmel()
            self._pool = torch.cat([lm(waves[i:i + 64]) for i in range(0, waves.shape[0], 64)])
        else:
            self._pool = waves

    def logmel(self):
        if self._logmel is None:
            from .features import GpuLogMel
            pc = self.preprocessing_config
            self._logmel = GpuLogMel(self.target_rate, pc.get("n_mels", self.n_mels), pc.get("normalize", True),
                                     pc.get("target_mean", 0.0), pc.get("target_std", 0.5))
        return self._logmel

    def gpu_transform(self, x: torch.Tensor, y: torch.Tensor, training: bool):
        """Per-batch feature transform + augmentation on the device -> (model input, soft labels)."""
        if isinstance(y, torch.Tensor) and y.dtype != torch.float32:
            y = y.to(self.device)
        if self._gen is None and x.is_cuda:
            self._gen = torch.Generator(device=x.device).manual_seed(1234 + self.rank)
        C = self.num_classes
        if not self.is_spectrogram:
            wav_aug = self.preprocessing_config.get("augment") or {}
            if training and x.is_cuda and (wav_aug.get("time_stretch") or wav_aug.get("gain_shift")):
                # EnvNetPreprocessor.apply_augmentation after the crop, before BC mixing (esc50.py:235-245)
                from .augment import stretch_gain
                x = stretch_gain(x.reshape(x.shape[0], -1), wav_aug.get("time_stretch"), wav_aug.get("gain_shift"),
                                 gen=self._gen).view(x.shape[0], 1, -1)
            if training and self.enable_bc_mixing:
                from .augment import bc_mix, bc_mix_cpu
                self._pools()
                if x.is_cuda:
                    out, ys, _ = bc_mix(x.reshape(x.shape[0], -1), y, C, gen=self._gen, pool=self._pool,
                                        pool_labels=self._pool_labels)
                else:  # trainer.accelerator=cpu (config 1 plumbing) only
                    out, ys, _ = bc_mix_cpu(x, y, C, self._pool, self._pool_labels)
                return out.view(x.shape[0], 1, -1), ys
            return x, _one_hot(y, C)
        spec = self.logmel()(x.reshape(x.shape[0], -1))
        if training:
            from .augment import spec_augment_mixup
            self._pools()
            aug = bool(self.augment.get("time_mask") or self.augment.get("freq_mask"))
            # reference quirk (esc50.py:271-272): the mask sizes read back from torchaudio's
            # TimeMasking/FrequencyMasking fall back to 192 / 48 whatever was configured
            spec, ys = spec_augment_mixup(spec, y, C, 192, 48, self.mixup_alpha, 0.25, gen=self._gen, specaug=aug,
                                          mixup=self.enable_mixup, pool=self._pool, pool_labels=self._pool_labels)
            return spec, ys
        return spec, _one_hot(y, C)

    # -------------------------------------------------------------------- loaders
    def _loader(self, ds, shuffle):
        sampler = DistributedSampler(ds, self.world, self.rank, shuffle=shuffle, seed=42) if self.world > 1 else None
        # whole clips (spectrogram path, no clip_length): the default collate behind a check that names the key
        collate = _collate_whole_clips if self.is_spectrogram and self.fit_length is None else None
        return DataLoader(ds, batch_size=self.batch_size, shuffle=shuffle and sampler is None, sampler=sampler,
                          num_workers=self.num_workers, pin_memory=self.device.type == "cuda",
                          persistent_workers=self.num_workers > 0, collate_fn=collate)

    def _resident_pool_waves(self, ds):
        """The augmentation pool's waveforms cut from the resident store with the loader's kernel: start 0, no
        padding, one window -- ``fit_window`` (EnvNet) or the whole clip (AST; the clips must be one length, as
        ``torch.stack`` demands on the host path).  AST with a clip length: the fitted clips (``mia_fit_gather``),
        as ``ESC50Dataset.clip`` gives them on the host path."""
        st = self._rstore
        sub = st.subset(ds.files)
        window = ds.window
        if self.is_spectrogram and self.fit_length is not None:
            return st.fit(sub.to(device=self.device, dtype=torch.int32), self.fit_length, self.clip_fit)
        if self.is_spectrogram:
            lens = {st.lengths_host[i] for i in sub.tolist()}
            if len(lens) != 1:
                raise ValueError(f"the Mixup pool holds whole clips of one length, but the training clips have "
                                 f"{len(lens)} different lengths ({min(lens)} .. {max(lens)} samples)")
            window = lens.pop()
        idx = sub.to(device=self.device, dtype=torch.int32)
        return st.gather(idx, torch.zeros_like(idx), 0, window)[0]

    def _resident_loader(self, name, ds, training):
        """One _ResidentLoader per split, kept across epochs (the trainer asks for the train loader every epoch)."""
        if name in self._loaders:
            return self._loaders[name]
        from .resident import _ResidentLoader
        st = self._rstore
        kw = dict(batch_size=self.batch_size, window=ds.window, shuffle=training, seed=42, world=self.world,
                  rank=self.rank)
        if self.is_spectrogram and self.fit_length is not None:
            kw.update(mode="fit", pad=0, window=self.fit_length, fit_mode=self.clip_fit)
        elif self.is_spectrogram:
            kw.update(mode="whole", pad=0)
        elif training:
            if self._crop_gen is None:
                self._crop_gen = torch.Generator(device=self.device).manual_seed(4321 + self.rank)
            kw.update(mode="random", pad=ds.pad if ds.pad_crop else 0, gen=self._crop_gen)
        elif ds.multi_crop_test:
            kw.update(mode="multi", pad=ds.pad, table=self._crop_table[0], counts=self._crop_table[1])
        else:
            kw.update(mode="center", pad=ds.pad)
        self._loaders[name] = _ResidentLoader(st, st.subset(ds.files), **kw)
        return self._loaders[name]

    def train_dataloader(self):
        if self._train_set is None:
            raise RuntimeError("Dataset not set up. Call setup() first.")
        if self.resident:
            return self._resident_loader("train", self._train_set, True)
        return self._loader(self._train_set, True)

    def val_dataloader(self):
        if self._val_set is None:
            raise RuntimeError("Dataset not set up. Call setup() first.")
        if self.resident:
            return self._resident_loader("val", self._val_set, False)
        return self._loader(self._val_set, False)

    def test_dataloader(self):
        if self._test_set is None:
            raise RuntimeError("Dataset not set up. Call setup() first.")
        if self.resident:
            return self._resident_loader("test", self._test_set, False)
        return self._loader(self._test_set, False)


class _DeviceLoader:
    """Batches straight from device-resident tensors (no host round trip)."""

    def __init__(self, x, y, batch_size, shuffle, seed, world=1, rank=0):
        self.x, self.y, self.bs, self.shuffle, self.seed = x, y, batch_size, shuffle, seed
        self.world, self.rank, self.epoch = world, rank, 0

    def set_epoch(self, e):
        self.epoch = e

    def _index(self):
        n = self.x.shape[0]
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(n, generator=g)
        else:
            idx = torch.arange(n)
        return idx[self.rank::self.world]

    def __len__(self):
        return max(1, math.ceil(len(self._index()) / self.bs))

    def __iter__(self):
        idx = self._index().to(self.x.device)
        for i in range(0, idx.numel(), self.bs):
            j = idx[i:i + self.bs]
            yield self.x[j], self.y[j]


class SyntheticDataModule(ESC50DataModule):
    """Device-resident synthetic clips with the ESC-50 DataModule interface: 0.1*N(0,1), peak-normalised
    (prepare_esc50.py:98-101), uniform labels; split into train/val/test 80/10/10."""

    def __init__(self, root: str = "none", num_clips: int = 64, clip_samples: int = 220_500, seed: int = 0, **kw):
        kw.pop("fold", None)
        super().__init__(root=root, fold=0, **kw)
        self.num_clips, self.clip_samples, self.seed = num_clips, clip_samples, seed

    def setup(self, stage=None):
        if self._train_set is not None:
            return
        g = torch.Generator(device=self.device).manual_seed(self.seed)
        x = 0.1 * torch.randn(self.num_clips, 1, self.clip_samples, generator=g, device=self.device)
        x = x / x.abs().amax(dim=-1, keepdim=True)
        if self.target_rate != self.sample_rate:  # clips are generated at the data module's rate
            if self.device.type != "cuda":
                raise ValueError(f"sample_rate={self.sample_rate} differs from preprocessing_config.sample_rate="
                                 f"{self.target_rate}: resampling runs on the GPU (there is no CPU resampler), but "
                                 f"the device is {self.device}")
            from .resample import MAX_CLIPS_PER_LAUNCH, GpuResample
            rs = GpuResample(self.sample_rate, self.target_rate)
            x = torch.cat([rs(x[i:i + MAX_CLIPS_PER_LAUNCH]) for i in range(0, x.shape[0], MAX_CLIPS_PER_LAUNCH)])
        if self.fit_length is not None:  # once, in setup: the clips are one length already
            x = fit_clip(x, self.fit_length, self.clip_fit).contiguous()
        y =torch.randint(0, self.num_classes, (self.num_clips,), generator=g, device=self.device)
        n = self.num_clips
        nv = max(1, n // 10)
        self._train_set = (x[: n - 2 * nv], y[: n - 2 * nv])
        self._val_set = (x[n - 2 * nv: n - nv], y[n - 2 * nv: n - nv])
        self._test_set = (x[n - nv:], y[n - nv:])
        self._train_labels = self._train_set[1].tolist()

    def _pools(self):
        if self._pool is not None or not (self.enable_bc_mixing or self.enable_mixup):
            return
        waves, labels = self._train_set
        self._pool_labels = labels
        self._pool = self.logmel()(waves.reshape(waves.shape[0], -1)) if self.is_spectrogram \
            else waves.reshape(waves.shape[0], -1)

    def train_dataloader(self):
        return _DeviceLoader(*self._train_set, self.batch_size, True, 42, self.world, self.rank)

    def val_dataloader(self):
        return _DeviceLoader(*self._val_set, self.batch_size, False, 42, self.world, self.rank)

    def test_dataloader(self):
        return _DeviceLoader(*self._test_set, self.batch_size, False, 42, self.world, self.rank)
