"""GPU: mia_fit_gather (include/miaudio_data.h) against the numpy restatement of the rule in tests/_fit_ref.py,
at the smallest shapes where the kernel can go wrong.  Every comparison is on the int32 view of the floats.

The store sits behind a junk prefix of 3 words (clip bases are misaligned) and holds raw uint32 patterns, a
signalling-NaN payload, -0.0, +inf and a denormal among them: a read outside a clip brings in junk or a neighbour's
words where the rule demands the clip's own or +0.0.  ``out`` is taken from a tests/_arena.py GuardedArena at
element offsets 0..3 past a 256-B boundary (every head and tail path of the 16-B grouping; the rows of one launch
shift further with ``length % 4``), between poisoned guard bands that must come back unchanged, under both poisons
(0xFF: an element never written stays a NaN; 0x00: a write of the poison value itself shows).

Store offsets above 2^31 elements are not tested here (such a store needs more than 8 GB); the offset arithmetic is
the one of mia_crop_gather, whose test covers it."""
import numpy as np
import pytest
import torch

from tests._arena import POISONS, GuardedArena
from tests._fit_ref import MODES, fit_ref

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 5, 64, 1031)  # 1031 > 1024: more than one block along a row
SPECIALS = (0x7FA12345, 0x80000000, 0x7F800000, 0x00000001)  # signalling NaN + payload, -0.0, +inf, a denormal
JUNK, PREFIX = 0xDEADBEEF, 3
B = 5


def clip_lengths(L):
    return [0, 1, 2, 3, L - 1, L, L + 1, L + 2, 2 * L + 1, 3 * L]


class Store:
    def __init__(self, L, device):
        rng = np.random.default_rng(100 + L)
        self.lens = clip_lengths(L)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        total = int(self.offsets_host[-1])
        words = rng.integers(1, 2 ** 32, size=total, dtype=np.uint64).astype(np.uint32)
        for c, n in enumerate(self.lens):
            clip = words[self.offsets_host[c]:self.offsets_host[c + 1]]
            for q in range(min(n, 4)):
                clip[q] = SPECIALS[(c + q) % 4]
            if n > 4:
                clip[n - 1] = SPECIALS[c % 4]
        self.words = words
        buf = np.full(PREFIX + total + 5, JUNK, dtype=np.uint32)
        buf[PREFIX:PREFIX + total] = words
        self.buf = torch.from_numpy(buf.view(np.int32)).to(device).view(torch.float32)
        self.data = self.buf[PREFIX:PREFIX + total]
        assert self.data.data_ptr() % 16 == 12
        self.offsets = torch.from_numpy(self.offsets_host).to(device)
        self.n_clips = len(self.lens)

    def clip(self, i):
        if not 0 <= i < self.n_clips:
            return np.zeros(0, dtype=np.uint32)
        return self.words[self.offsets_host[i]:self.offsets_host[i + 1]]

    def expected(self, idx, L, mode):
        return np.stack([fit_ref(self.clip(i), L, mode) for i in idx]).view(np.int32)


@pytest.fixture(scope="module")
def stores(cuda):
    return {L: Store(L, cuda) for L in LENGTHS}


def _launches(n_clips):
    """Three launches of B = 5 rows: every clip, a clip number below and one past the store, three repeats."""
    rows = list(range(n_clips)) + [-1, n_clips, n_clips - 1, 4, 1]
    assert len(rows) == 3 * B
    return [rows[0:B], rows[B:2 * B], rows[2 * B:3 * B]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", LENGTHS)
def test_fit_gather_matches_the_rule(cuda, stores, L, mode):
    from src.miaudio import kernels as K
    st = stores[L]
    lens = st.lens
    assert {(n - L) % 2 for n in lens if n > L} == {0, 1}  # odd and even centre trims
    if L >= 64:
        assert all(-(-L // n) > 2 for n in (1, 2, 3))  # more than two repeats
    for poison in POISONS:
        arena = GuardedArena(cuda, poison)
        runs = []
        for off in range(4):
            for idx in _launches(st.n_clips):
                out = arena.take_as(f"out+{off}", (B, L), torch.float32, offset=4 * off)
                assert out.data_ptr() % 16 == (4 * off) % 16
                res = K.fit_gather(st.data, st.offsets, torch.tensor(idx, dtype=torch.int32, device=cuda), L, mode,
                                   out=out)
                assert res.data_ptr() == out.data_ptr()
                runs.append((idx, out))
        torch.cuda.synchronize()
        arena.check()
        for idx, out in runs:
            got = out.view(torch.int32).cpu().numpy()
            exp = st.expected(idx, L, mode)
            assert np.array_equal(got, exp), (poison, idx, np.argwhere(got != exp)[:4].tolist())
            for r, i in enumerate(idx):
                if not 0 <= i < st.n_clips or lens[i] == 0:
                    assert not got[r].any()  # +0.0: sign bit clear
        assert bool((st.buf[:PREFIX].view(torch.int32) == JUNK - 2 ** 32).all())
        arena.release()


@pytest.mark.parametrize("mode", MODES)
def test_one_row_and_default_output(cuda, stores, mode):
    from src.miaudio import kernels as K
    for L in (5, 1031):
        st = stores[L]
        for i in (2, 8, 9, st.n_clips):  # wrapped many times, trimmed odd and even, outside the store
            out = K.fit_gather(st.data, st.offsets, torch.tensor([i], dtype=torch.int32, device=cuda), L, mode)
            assert out.shape == (1, L) and out.dtype == torch.float32
            assert np.array_equal(out.view(torch.int32).cpu().numpy(), st.expected([i], L, mode))


def test_zero_mode_is_the_crop_gather_zero_padding(cuda, stores):
    """For clips no longer than L, mode zero is mia_crop_gather at pad 0, start 0 (tools/bench_data.py's yardstick)."""
    from src.miaudio import kernels as K
    L = 1031
    st = stores[L]
    idx = torch.tensor([0, 1, 2, 3, 4, 5], dtype=torch.int32, device=cuda)
    a = K.fit_gather(st.data, st.offsets, idx, L, "zero")
    b = K.crop_gather(st.data, st.offsets, idx, torch.zeros_like(idx), 0, L)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_wrapper_rejects_bad_tensors(cuda, stores):
    from src.miaudio import kernels as K
    st = stores[4]
    idx = torch.zeros(2, dtype=torch.int32, device=cuda)
    with pytest.raises(TypeError, match="idx must be a contiguous torch.int32"):
        K.fit_gather(st.data, st.offsets, idx.long(), 4)
    with pytest.raises(TypeError, match="offsets must be a contiguous torch.int64"):
        K.fit_gather(st.data, st.offsets.int(), idx, 4)
    with pytest.raises(TypeError, match="out must be contiguous f32"):
        K.fit_gather(st.data, st.offsets, idx, 4, out=torch.empty(2, 5, device=cuda))
    with pytest.raises(ValueError, match="mode"):
        K.fit_gather(st.data, st.offsets, idx, 4, "reflect")
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.fit_gather(st.data.cpu(), st.offsets.cpu(), idx.cpu(), 4)


def test_launcher_rejects_bad_arguments(cuda, stores):
    from src.miaudio import lib as L
    lib = L.load()
    st = stores[4]
    idx = torch.zeros(1, dtype=torch.int32, device=cuda)
    sentinel = 0x4B1D4B1D
    out = torch.full((16,), sentinel, dtype=torch.int32, device=cuda)

    def call(store_p=st.data.data_ptr(), off_p=st.offsets.data_ptr(), n_clips=st.n_clips, idx_p=idx.data_ptr(), B=1,
             length=4, mode=0, out_p=out.data_ptr()):
        return lib.mia_fit_gather(store_p, off_p, n_clips, idx_p, B, length, mode, out_p, L.stream_ptr())

    for bad in (dict(out_p=None), dict(length=0), dict(mode=2), dict(B=0), dict(mode=-1), dict(length=-4),
                dict(n_clips=0), dict(store_p=None), dict(off_p=None), dict(idx_p=None),
                dict(out_p=out.data_ptr() + 2), dict(store_p=st.data.data_ptr() + 1)):
        assert call(**bad) < 0, bad
        assert lib.mia_last_error_string(), bad
        torch.cuda.synchronize()
        assert bool((out == sentinel).all()), bad
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out[4:] == sentinel).all()) and not bool((out[:4] == sentinel).any())


def test_resident_store_fit_equals_fit_clip_of_each_file(cuda, tmp_path):
    from src.datasets.esc50 import fit_clip
    from src.datasets.resident import build_resident_store
    from tests.test_fit_cpu import L as LEN
    from tests.test_fit_cpu import RATE, ragged_tree
    files = ragged_tree(tmp_path)
    paths = sorted(files)
    store = build_resident_store(paths, RATE, cuda)
    assert min(store.lengths_host) < LEN < max(store.lengths_host)
    order = torch.randperm(len(paths), generator=torch.Generator().manual_seed(3)).tolist()
    order = order + order[:7] + [order[0]] * 3
    idx = torch.tensor([store.index[paths[i]] for i in order], dtype=torch.int32, device=cuda)
    for mode in MODES:
        got = store.fit(idx, LEN, mode).cpu()
        assert got.shape == (len(order), LEN)
        for r, i in enumerate(order):
            ref = fit_clip(files[paths[i]], LEN, mode)[0]
            assert torch.equal(got[r].view(torch.int32), ref.contiguous().view(torch.int32)), (mode, r)
