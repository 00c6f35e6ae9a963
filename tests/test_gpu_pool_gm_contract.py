"""GPU: the memory contract of include/miaudio_pool.h, with the harness of tests/test_gpu_memory_contract.py.

gm (f32 and bf16), dgamma, dbeta, dx, dbias and the partial workspaces are taken from the guarded arena at exactly
their stated sizes; each call runs three times (poison 0xFF, poison 0x00, plain buffers); the guards stay clean and
every output is bit-identical across the runs.  The gather runs in each of its forms: the 16-B-load kernel (NHWC with
the winners saved), the staged kernel (channel-major from 16 cells a block iteration) and the per-element kernel (no
winners; channel-major at C = 256).  The cell counts are no multiple of a block iteration, so the ragged last
iteration is in play.

COVERS maps every case to the entry points it calls; tests/test_pool_gm_cpu.py checks it against the header.
"""
import functools

import pytest
import torch

from src.miaudio import lib as L  # noqa: F401
from tests.test_gpu_memory_contract import BF16, F32, U8, bn_state, code, p, rnd, run_three, uni

CASES = {}


def _pool_gm_case(dev, n, h, w, c, kh, kw_, dt, gdt):
    oh, ow = h // kh, w // kw_
    cells, P = n * oh * ow, n * h * w
    x = rnd(dev, (n, h, w, c), dt, 31)
    gamma, beta = uni(dev, c, 0.5, 1.5, 32), rnd(dev, c, F32, 33, 0.1)
    gamma[1] = -gamma[1]
    mean, invstd, scale, shift = bn_state(x.view(P, c), gamma, beta)
    g = torch.Generator(device=dev).manual_seed(34)
    argmax = torch.randint(0, kh * kw_, (cells, c), generator=g, device=dev).to(U8)
    win = rnd(dev, (cells, c), dt, 35)
    dout = rnd(dev, (cells, c), dt, 36)
    gm_in = rnd(dev, (cells, c), gdt, 37)
    dgamma, dbeta = rnd(dev, c, F32, 38), rnd(dev, c, F32, 39)

    def run(ctx):
        nb = ctx.lib.mia_bn_partial_bytes(P, c)
        for layout in (0, 1, 2):
            if layout == 1 and oh != 1:
                continue
            for tag, wptr in ((f"gather{layout}", None), (f"gather{layout}_win", p(win))):
                gm = ctx.out(f"{tag}.gm", (cells, c), gdt)
                dg, db = ctx.out(f"{tag}.dgamma", c, F32), ctx.out(f"{tag}.dbeta", c, F32)
                ctx.call("mia_pool_bwd_gather_ex", p(dout), layout, p(argmax), p(x), wptr, code(dt), n, h, w, c, kh, kw_,
                         p(scale), p(shift), p(mean), p(invstd), p(gm), code(gdt), p(dg), p(db),
                         p(ctx.ws(f"{tag}.partial", nb)))
        dx, dbias = ctx.out("apply.dx", (n, h, w, c), dt), ctx.out("apply.dbias", c, F32)
        ctx.call("mia_pool_bn_relu_bwd_apply_ex", p(gm_in), code(gdt), p(argmax), p(x), code(dt), n, h, w, c, kh, kw_,
                 p(gamma), p(mean), p(invstd), p(dgamma), p(dbeta), p(dx), p(dbias), p(ctx.ws("apply.partial", nb)))
    return run


for _geo, _dt, _gdt in [((2, 1, 200, 64, 1, 64), BF16, BF16),    # frontend pool: staged gather, row-octet apply
                        ((3, 11, 68, 32, 5, 3), BF16, BF16),      # 132 cells: runs of 3
                        ((3, 2, 75, 256, 1, 2), BF16, BF16),      # 222 cells, 8 a block iteration: runs of 2
                        ((3, 2, 75, 256, 1, 2), BF16, F32),
                        ((2, 10, 35, 32, 5, 3), F32, F32),        # f32 activations: per-pixel apply
                        ((2, 5, 23, 64, 2, 5), BF16, BF16)]:      # kw = 5: per-pixel apply reading a bf16 gm
    CASES[f"pool_gm[{_geo}-{_dt}-gm-{_gdt}]"] = (
        ("mia_pool_bwd_gather_ex", "mia_pool_bn_relu_bwd_apply_ex"),
        functools.partial(lambda dev, g, d, gd: _pool_gm_case(dev, *g, d, gd), g=_geo, d=_dt, gd=_gdt))

COVERS = {name: covers for name, (covers, _) in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_pool_gm_memory_contract(cuda, monkeypatch, name):
    for v in ("MIA_POOL_V1", "MIA_POOL_GRID"):
        monkeypatch.delenv(v, raising=False)
    run_three(cuda, CASES[name][1](cuda), monkeypatch)
