"""GPU: the memory contract of include/miaudio_optim.h, with the harness of tests/test_gpu_memory_contract.py.

Parameters, moments, bf16 shadows, the pointer / size / first-use / step tables and the norm workspace are taken from
the guarded arena at exactly their stated sizes; each call runs three times (poison 0xFF, poison 0x00, plain
buffers); the guards stay clean and every output is bit-identical across the runs.  A momentum buffer at its first
use is an output only: it is left poisoned before the call.

COVERS maps every case to the entry points it calls; tests/test_optim_family_cpu.py checks it against the header.
"""
import functools

import pytest
import torch

from src.miaudio import kernels as K
from src.miaudio import lib as L
from tests.test_gpu_memory_contract import BF16, F32, F64, I32, I64, Ctx, p, rnd, run_three, uni  # noqa: F401

CASES = {}


def _table(ctx, name, values, dtype=I64):
    t = ctx.out(name, len(values), dtype, compare=False)  # device addresses differ between the runs
    t.copy_(torch.tensor(values, dtype=dtype))
    return t


def _clip_case(dev, what, sizes, offset, momentum=0.9, first=None, steps=None):
    n = len(sizes)
    adamw = what == "mia_clip_adamw"
    P0 = [rnd(dev, s, F32, 250 + i) for i, s in enumerate(sizes)]
    G0 = [rnd(dev, s, F32, 260 + i, 3.0) for i, s in enumerate(sizes)]
    M0 = [rnd(dev, s, F32, 270 + i, 0.01) for i, s in enumerate(sizes)]
    V0 = [uni(dev, s, 0.0, 1e-3, 280 + i) for i, s in enumerate(sizes)]
    if offset:  # gradients are inputs: the same 4-byte offset by hand
        G0 = [torch.cat([g.new_zeros(1), g])[1:] for g in G0]

    def run(ctx):
        pp = [ctx.out(f"param{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        sh = [ctx.out(f"shadow{i}", s, BF16, offset=offset // 2) if i == 0 else None for i, s in enumerate(sizes)]
        for dst, src in zip(pp, P0):
            dst.copy_(src)
        mm = vv = None
        if adamw or momentum:
            mm = [ctx.out(f"moment{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
            for i, (dst, src) in enumerate(zip(mm, M0)):
                if adamw or not (first and first[i]):  # a buffer at first use is written, never read
                    dst.copy_(src)
        if adamw:
            vv = [ctx.out(f"exp_avg_sq{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
            for dst, src in zip(vv, V0):
                dst.copy_(src)
        ptrs = lambda ts: [0 if t is None else t.data_ptr() for t in ts]  # noqa: E731
        tp, tg = _table(ctx, "params", ptrs(pp)), _table(ctx, "grads", ptrs(G0))
        tm = _table(ctx, "moments", ptrs(mm)) if mm else None
        tv = _table(ctx, "exp_avg_sq", ptrs(vv)) if vv else None
        ts, tn = _table(ctx, "shadows", ptrs(sh)), _table(ctx, "sizes", list(sizes))
        tot = ctx.out("total_norm", 1, F32)
        ws = ctx.ws("sqnorm_ws", ctx.lib.mia_adam_workspace_bytes(n))
        if adamw:
            st = _table(ctx, "steps", list(steps), I32) if steps else None
            ctx.call("mia_clip_adamw", p(tp), p(tg), p(tm), p(tv), p(ts), p(tn), n, max(sizes), max(sizes), 1e-3, 0.9,
                     0.999, 1e-8, 1e-2, 3, 1.0, p(tot), p(ws), None, None, p(st))
        else:
            fu = _table(ctx, "first_use", list(first), I32) if first else None
            ctx.call("mia_clip_sgd", p(tp), p(tg), p(tm), p(ts), p(tn), n, max(sizes), max(sizes), 1e-2, momentum, 0.0,
                     1e-4, 1 if momentum else 0, 1.0, p(tot), p(ws), None, None, p(fu))
    return run


def _gemm_case(dev, what, momentum=0.9, first=0):
    M, N, Kd = 256, 384, 128
    adamw = what == "mia_gemm_adamw"
    dy, x = rnd(dev, (Kd, M), BF16, 207), rnd(dev, (Kd, N), BF16, 208)
    p0, m0, v0 = rnd(dev, (M, N), F32, 209), rnd(dev, (M, N), F32, 210, 0.01), uni(dev, (M, N), 0.0, 1e-3, 211)
    coef = torch.tensor([0.37], device=dev)

    def run(ctx):
        A, Bo = K.dense(dy, L.RC, Kd, M), K.dense(x, L.RC, Kd, N)
        pp, sh = ctx.out("param", (M, N), F32), ctx.out("shadow_bf16", (M, N), BF16)
        pp.copy_(p0)
        if adamw:
            mm, vv = ctx.out("exp_avg", (M, N), F32), ctx.out("exp_avg_sq", (M, N), F32)
            mm.copy_(m0), vv.copy_(v0)
            ctx.call("mia_gemm_adamw", A, Bo, M, N, Kd, p(pp), p(mm), p(vv), p(sh), N, p(coef), 1e-3, 0.0316, 0.9, 0.999,
                     1e-8, 1e-3, 1e-2)
            return
        buf = None
        if momentum:
            buf = ctx.out("momentum_buffer", (M, N), F32)
            if not first:
                buf.copy_(m0)
        ctx.call("mia_gemm_sgd", A, Bo, M, N, Kd, p(pp), p(buf), p(sh), N, p(coef), 1e-2, momentum, 0.0, 1e-4,
                 1 if momentum else 0, first)
    return run


def _case(name, covers, fn, **kw):
    CASES[name] = ((covers,), functools.partial(fn, what=covers, **kw))


_case("clip_sgd[1-tensor-300001]", "mia_clip_sgd", _clip_case, sizes=(300_001,), offset=0)
_case("clip_sgd[3-tensors-first-use]", "mia_clip_sgd", _clip_case, sizes=(1003, 4096, 7), offset=0, first=(1, 0, 1))
_case("clip_sgd[3-tensors-4-byte-offset]", "mia_clip_sgd", _clip_case, sizes=(1003, 4096, 7), offset=4)
_case("clip_sgd[no-momentum]", "mia_clip_sgd", _clip_case, sizes=(1003, 4096, 7), offset=0, momentum=0.0)
_case("clip_sgd[no-momentum-300001-4-byte-offset]", "mia_clip_sgd", _clip_case, sizes=(300_001, 7), offset=4,
      momentum=0.0)
_case("clip_adamw[1-tensor-300001]", "mia_clip_adamw", _clip_case, sizes=(300_001,), offset=0)
_case("clip_adamw[3-tensors-steps]", "mia_clip_adamw", _clip_case, sizes=(1003, 4096, 7), offset=0, steps=(3, 2, 3))
_case("clip_adamw[3-tensors-4-byte-offset]", "mia_clip_adamw", _clip_case, sizes=(1003, 4096, 7), offset=4)
_case("gemm_sgd[256x384x128]", "mia_gemm_sgd", _gemm_case)
_case("gemm_sgd[256x384x128-first-use]", "mia_gemm_sgd", _gemm_case, first=1)
_case("gemm_sgd[256x384x128-no-momentum]", "mia_gemm_sgd", _gemm_case, momentum=0.0)
_case("gemm_adamw[256x384x128]", "mia_gemm_adamw", _gemm_case)

COVERS = {name: covers for name, (covers, _) in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_optim_family_memory_contract(cuda, monkeypatch, name):
    run_three(cuda, CASES[name][1](cuda), monkeypatch)
