"""GPU: mia_crop_gather (include/miaudio_data.h) against the reference's pad + right-pad + crop restated here with
F.pad and slicing.  Every comparison is torch.equal on the int32 view, so NaN payloads and -0.0 count.

The store is a slice in the middle of a NaN-filled buffer (a read outside a clip would bring in a NaN or a
neighbour's nonzero sample where the rule demands +0.0); ``out`` is a NaN-prefilled slice between sentinel bands."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

LENGTHS = [1000, 1001, 4410, 4413, 9000, 13230]
LEAD = 37  # elements of the buffer before the store: clip bases are odd and even, none 16-B aligned by design
SENTINEL = 12345.0
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def store(cuda):
    g = torch.Generator().manual_seed(11)
    total = sum(LENGTHS)
    data = torch.rand(total, generator=g) + 0.5  # nonzero everywhere
    offsets = [0]
    for n in LENGTHS:
        offsets.append(offsets[-1] + n)
    for i, n in enumerate(LENGTHS):  # a NaN with a payload and a -0.0 in every clip, at its ends and inside
        bits = data[offsets[i]:offsets[i + 1]].view(torch.int32)
        bits[0] = 0x7FC12345
        bits[n // 2] = -2 ** 31  # -0.0
        bits[n - 1] = 0xFFA00001 - 2 ** 32  # a negative NaN with a payload
        bits[1] = -2 ** 31
    buf = torch.full((LEAD + total + 91,), float("nan"))
    buf[LEAD:LEAD + total] = data
    assert torch.equal(buf[LEAD:LEAD + total].view(torch.int32), data.view(torch.int32))
    dev_buf = buf.to(cuda)
    return {"buf": dev_buf, "data": dev_buf[LEAD:LEAD + total], "host": data, "offsets_host": offsets,
            "offsets": torch.tensor(offsets, dtype=torch.int64, device=cuda)}


def _reference(host, offsets, idx, start, pad, window):
    """(ncrop, B, window): F.pad + slicing, with a margin of one window each side so any overlapping start is a
    plain slice; a start whose window misses the padded clip altogether is all zeros."""
    B, ncrop = len(start), len(start[0])
    out = torch.zeros(ncrop, B, window)
    for b in range(B):
        clip = host[offsets[idx[b]]:offsets[idx[b] + 1]]
        total = clip.numel() + 2 * pad
        ext = F.pad(clip, (pad + window, pad + window))
        for c in range(ncrop):
            s = start[b][c]
            if s < -window or s > total:
                continue
            out[c, b] = ext[s + window:s + 2 * window]
    return out


def _starts(n, pad, window, count):
    """Starts for one clip: 0, max_start, every alignment mod 4, a partly negative one, one partly beyond the end,
    then those that miss the clip altogether (negative, beyond the end, the int32 extremes)."""
    total = n + 2 * pad
    mx = max(0, total - window)
    inside = [0, mx, 1, 2, 3, mx // 2, -5, total - 3, max(0, mx - 1)]
    zeros = [-window - 1, total + 5, I32_MIN, I32_MAX]
    pool = inside + zeros
    return [pool[k % len(pool)] for k in range(count)], zeros


@pytest.mark.parametrize("lead", [64, 65])
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("ncrop", [1, 5])
@pytest.mark.parametrize("pad,window", [(2205, 4410), (0, 4410), (0, 4413), (7, 1)])
def test_crop_gather_matches_pad_and_slice(cuda, store, pad, window, ncrop, B, lead):
    from src.miaudio import kernels as K
    idx = [5, 0, 3, 3, 1, 4, 2][:B] if B > 1 else [3]
    start, rot = [], 0
    for b in range(B):
        s, _ = _starts(LENGTHS[idx[b]], pad, window, 13)
        start.append([s[(rot + c) % 13] for c in range(ncrop)])
        rot += ncrop  # B * ncrop = 35 > 13: the whole list is used at ncrop = 5, B = 7
    ref = _reference(store["host"], store["offsets_host"], idx, start, pad, window)
    n = ncrop * B * window
    big = torch.full((lead + n + 64,), SENTINEL, device=cuda)
    big[lead:lead + n] = float("nan")
    out = big[lead:lead + n]
    res = K.crop_gather(store["data"], store["offsets"], torch.tensor(idx, dtype=torch.int32, device=cuda),
                        torch.tensor(start, dtype=torch.int32, device=cuda), pad, window, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    got = out.view(ncrop, B, window).cpu()
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    assert bool((big[:lead] == SENTINEL).all()) and bool((big[lead + n:] == SENTINEL).all())


def test_starts_that_miss_the_clip_give_positive_zero(cuda, store):
    from src.miaudio import kernels as K
    pad, window = 2205, 4410
    idx = [0, 2, 5, 1]
    zeros = [_starts(LENGTHS[i], pad, window, 1)[1] for i in idx]  # [B][4]: negative, beyond, int32 min and max
    out = K.crop_gather(store["data"], store["offsets"], torch.tensor(idx, dtype=torch.int32, device=cuda),
                        torch.tensor(zeros, dtype=torch.int32, device=cuda), pad, window)
    torch.cuda.synchronize()
    assert out.shape == (4, 4, window)
    assert not out.view(torch.int32).any()  # +0.0 bits: no NaN from outside the clip, no -0.0


def test_default_output_and_1d_start(cuda, store):
    from src.miaudio import kernels as K
    idx = [4, 4, 0]
    start = [100, 101, 0]
    out = K.crop_gather(store["data"], store["offsets"], torch.tensor(idx, dtype=torch.int32, device=cuda),
                        torch.tensor(start, dtype=torch.int32, device=cuda), 0, 4413)
    ref = _reference(store["host"], store["offsets_host"], idx, [[s] for s in start], 0, 4413)
    assert out.shape == (1, 3, 4413)
    assert torch.equal(out.cpu().view(torch.int32), ref.view(torch.int32))


def test_clip_past_two_to_the_31_elements(cuda):
    """64-bit index math: a clip whose base lies past 2^31 elements of the store (a 48 kHz UrbanSound8K store is
    that large).  Only the clip itself is written; the 8.6 GB before it are never touched."""
    from src.miaudio import kernels as K
    base, n, window = 2 ** 31 + 5, 3001, 1000
    data = torch.empty(base + n, dtype=torch.float32, device=cuda)
    clip = torch.rand(n, generator=torch.Generator().manual_seed(3)) + 0.5
    data[base:] = clip.to(cuda)
    offsets = torch.tensor([0, base, base + n], dtype=torch.int64, device=cuda)
    out = K.crop_gather(data, offsets, torch.tensor([1, 1], dtype=torch.int32, device=cuda),
                        torch.tensor([[0, 7], [2001, 2500]], dtype=torch.int32, device=cuda), 0, window)
    got = out.cpu()
    assert torch.equal(got[0, 0], clip[:1000]) and torch.equal(got[1, 0], clip[7:1007])
    assert torch.equal(got[0, 1], clip[2001:3001])
    assert torch.equal(got[1, 1], F.pad(clip[2500:], (0, 499)))


def test_launcher_rejects_bad_arguments(cuda, store):
    from src.miaudio import lib as L
    lib = L.load()
    d, o = store["data"], store["offsets"]
    idx = torch.zeros(1, dtype=torch.int32, device=cuda)
    out = torch.full((16,), SENTINEL, device=cuda)

    def call(store_p=d.data_ptr(), off_p=o.data_ptr(), idx_p=idx.data_ptr(), start_p=idx.data_ptr(), B=1, ncrop=1,
             pad=0, window=4, out_p=out.data_ptr()):
        return lib.mia_crop_gather(store_p, off_p, len(LENGTHS), idx_p, start_p, B, ncrop, pad, window, out_p,
                                   L.stream_ptr())

    assert call() == 0
    for bad in (dict(B=0), dict(ncrop=0), dict(window=0), dict(pad=-1), dict(store_p=None), dict(off_p=None),
                dict(idx_p=None), dict(start_p=None), dict(out_p=None)):
        assert call(**bad) < 0, bad
        assert lib.mia_last_error_string()
    torch.cuda.synchronize()
    assert bool((out[4:] == SENTINEL).all())
