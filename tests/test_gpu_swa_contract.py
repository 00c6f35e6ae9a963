"""GPU: the memory contract of include/miaudio_swa.h, with the harness of tests/test_gpu_memory_contract.py as
tests/test_gpu_optim_family_contract.py uses it.

Averages, parameters, bf16 shadows and the pointer / size tables are taken from the guarded arena at exactly their
stated sizes; each call runs three times (poison 0xFF, poison 0x00, plain buffers); the guards stay clean and every
buffer is bit-identical across the runs.  mia_swa_update writes avg only (at n_averaged == 0 without reading it: it
is left poisoned before the call) and leaves params as they were; mia_swa_transfer writes params and the non-NULL
shadows only (both left poisoned before the call) and leaves avg as it was.
"""
import functools

import pytest
import torch

from tests.test_gpu_memory_contract import BF16, F32, I64, p, rnd, run_three

CASES = {}


def _table(ctx, name, values):
    t = ctx.out(name, len(values), I64, compare=False)  # device addresses differ between the runs
    t.copy_(torch.tensor(values, dtype=I64))
    return t


def _ptrs(ts):
    return [0 if t is None else t.data_ptr() for t in ts]


def _update_case(dev, sizes, offset, n_averaged):
    P0 = [rnd(dev, s, F32, 310 + i) for i, s in enumerate(sizes)]
    A0 = [rnd(dev, s, F32, 320 + i, 0.5) for i, s in enumerate(sizes)]

    def run(ctx):
        avg = [ctx.out(f"avg{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        par = [ctx.out(f"param{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        for dst, src in zip(par, P0):
            dst.copy_(src)
        if n_averaged:  # at n_averaged == 0 avg is an output only
            for dst, src in zip(avg, A0):
                dst.copy_(src)
        ta, tp, tn = _table(ctx, "avgs", _ptrs(avg)), _table(ctx, "params", _ptrs(par)), _table(ctx, "sizes", list(sizes))
        ctx.call("mia_swa_update", p(ta), p(tp), p(tn), len(sizes), max(sizes), n_averaged)
        torch.cuda.synchronize()
        for got, src in zip(par, P0):
            assert torch.equal(got, src), "mia_swa_update wrote a parameter"
    return run


def _transfer_case(dev, sizes, offset, shadows):
    """shadows: None (NULL table) or a tuple of flags (a False entry is a NULL pointer in the table)."""
    A0 = [rnd(dev, s, F32, 330 + i) for i, s in enumerate(sizes)]

    def run(ctx):
        par = [ctx.out(f"param{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        avg = [ctx.out(f"avg{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        for dst, src in zip(avg, A0):
            dst.copy_(src)
        sh = [ctx.out(f"shadow{i}", s, BF16, offset=offset // 2) if shadows and shadows[i] else None
              for i, s in enumerate(sizes)]
        tp, ta, tn = _table(ctx, "params", _ptrs(par)), _table(ctx, "avgs", _ptrs(avg)), _table(ctx, "sizes", list(sizes))
        ts = _table(ctx, "shadows", _ptrs(sh)) if shadows else None
        ctx.call("mia_swa_transfer", p(tp), p(ta), p(ts), p(tn), len(sizes), max(sizes))
        torch.cuda.synchronize()
        for got, src in zip(avg, A0):
            assert torch.equal(got, src), "mia_swa_transfer wrote an average"
    return run


def _case(name, fn, **kw):
    CASES[name] = functools.partial(fn, **kw)


# 70 001 elements: 9 blocks of 256 threads -- the unrolled loop, the one-group loop and a one-element tail
_case("swa_update[first-70001-1003-7]", _update_case, sizes=(70_001, 1003, 7), offset=0, n_averaged=0)
_case("swa_update[n3-70001-1003-7]", _update_case, sizes=(70_001, 1003, 7), offset=0, n_averaged=3)
_case("swa_update[n3-4-byte-offset]", _update_case, sizes=(70_001, 1003, 7), offset=4, n_averaged=3)
_case("swa_update[first-4-byte-offset]", _update_case, sizes=(1003, 7), offset=4, n_averaged=0)
_case("swa_transfer[shadows-one-null]", _transfer_case, sizes=(70_001, 1003, 7), offset=0, shadows=(True, False, True))
_case("swa_transfer[null-shadow-table]", _transfer_case, sizes=(70_001, 1003, 7), offset=0, shadows=None)
_case("swa_transfer[4-byte-offset]", _transfer_case, sizes=(70_001, 1003, 7), offset=4, shadows=(True, True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_swa_memory_contract(cuda, monkeypatch, name):
    run_three(cuda, CASES[name](cuda), monkeypatch)
