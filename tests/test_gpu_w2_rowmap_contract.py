"""GPU: the memory contract of include/miaudio_rowmap.h, with the harness of tests/test_gpu_memory_contract.py.

The row-mapped dx ((lead + rows * row_pixels) * c elements), the zero pixel, dbias and the partial workspaces are taken
from the guarded arena at exactly their stated sizes; each call runs three times (poison 0xFF, poison 0x00, plain
buffers); the guards stay clean and every output is bit-identical across the runs -- so every element of dx, the
lead pixels and the zero columns included, is written.  The maps: the (1, 2)-conv layout (lead 1, one zero column), a
wider one (lead 2, three zero columns) and the dense one.

COVERS maps every case to the entry points it calls; test_header_functions_are_bound_and_covered checks it against
the header."""
import functools
import re
from pathlib import Path

import pytest
import torch

from src.miaudio import lib as L
from tests.test_gpu_memory_contract import BF16, F32, U8, bn_state, code, p, rnd, run_three, uni

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio_rowmap.h"
MAPS = ((1, 1), (2, 3), (0, 0))  # (lead, zero columns per row)
CASES = {}


def _pool_case(dev, n, h, w, c, kh, kw_, gdt):
    oh, ow = h // kh, w // kw_
    cells, P = n * oh * ow, n * h * w
    x = rnd(dev, (n, h, w, c), BF16, 41)
    gamma, beta = uni(dev, c, 0.5, 1.5, 42), rnd(dev, c, F32, 43, 0.1)
    gamma[1] = -gamma[1]
    mean, invstd, _, _ = bn_state(x.view(P, c), gamma, beta)
    g = torch.Generator(device=dev).manual_seed(44)
    argmax = torch.randint(0, kh * kw_, (cells, c), generator=g, device=dev).to(U8)
    gm_in = rnd(dev, (cells, c), gdt, 45)
    dgamma, dbeta = rnd(dev, c, F32, 46), rnd(dev, c, F32, 47)

    def run(ctx):
        nb = ctx.lib.mia_bn_partial_bytes(P, c)
        for lead, extra in MAPS:
            tag = f"pool.l{lead}e{extra}"
            dx = ctx.out(f"{tag}.dx", (lead + n * h * (w + extra), c), BF16)
            zp = ctx.out(f"{tag}.zero_pixel", 64, BF16) if lead else None
            dbias = ctx.out(f"{tag}.dbias", c, F32)
            ctx.call("mia_pool_bn_relu_bwd_apply_rows", p(gm_in), code(gdt), p(argmax), p(x), code(BF16), n, h, w, c,
                     kh, kw_, p(gamma), p(mean), p(invstd), p(dgamma), p(dbeta), p(dx), lead, w + extra, p(zp),
                     64 if lead else 0, p(dbias), p(ctx.ws(f"{tag}.partial", nb)))
    return run


def _bn_case(dev, rows, w, c, dt):
    P = rows * w
    x, dact = rnd(dev, (P, c), dt, 51), rnd(dev, (P, c), dt, 52)
    gamma, beta = uni(dev, c, 0.5, 1.5, 53), rnd(dev, c, F32, 54, 0.1)
    mean, invstd, scale, shift = bn_state(x, gamma, beta)
    dgamma, dbeta = rnd(dev, c, F32, 55), rnd(dev, c, F32, 56)

    def run(ctx):
        nb = ctx.lib.mia_bn_partial_bytes(P, c)
        for lead, extra in MAPS:
            tag = f"bn.l{lead}e{extra}"
            dx = ctx.out(f"{tag}.dx", (lead + rows * (w + extra), c), dt)
            zp = ctx.out(f"{tag}.zero_pixel", 32, dt) if lead else None
            dbias = ctx.out(f"{tag}.dbias", c, F32)
            ctx.call("mia_bn_relu_bwd_apply_rows", p(dact), p(x), p(dx), code(dt), P, c, w, lead, w + extra, p(zp),
                     32 if lead else 0, p(gamma), p(scale), p(shift), p(mean), p(invstd), p(dgamma), p(dbeta),
                     p(dbias), p(ctx.ws(f"{tag}.partial", nb)))
    return run


for _geo, _gdt in [((3, 2, 75, 256, 1, 2), BF16),   # runs of 2, 8 a block iteration, a column past the last cell
                   ((3, 2, 75, 256, 1, 2), F32),
                   ((3, 11, 68, 32, 5, 3), BF16)]:   # runs of 3, kh = 5
    CASES[f"pool_rows[{_geo}-gm-{_gdt}]"] = (("mia_pool_bn_relu_bwd_apply_rows",),
                                             functools.partial(lambda dev, g, gd: _pool_case(dev, *g, gd), g=_geo, gd=_gdt))
for _rows, _w, _c, _dt in [(7, 37, 64, BF16), (5, 9, 256, BF16), (7, 37, 32, F32)]:
    CASES[f"bn_rows[{_rows}x{_w}-C{_c}-{_dt}]"] = (("mia_bn_relu_bwd_apply_rows",),
                                                    functools.partial(_bn_case, rows=_rows, w=_w, c=_c, dt=_dt))

COVERS = {name: covers for name, (covers, _) in CASES.items()}


def test_header_functions_are_bound_and_covered():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(mia_\w+)\s*\(([^)]*)\)\s*;", text))
    assert set(decls) == {"mia_pool_bn_relu_bwd_apply_rows", "mia_bn_relu_bwd_apply_rows"}
    assert set(decls) <= set(L.SIGNATURES) and set(decls) <= L.exported_symbols()
    for name, params in decls.items():
        assert len(L.SIGNATURES[name][1]) == len(params.split(",")), name
    assert {n for covers in COVERS.values() for n in covers} == set(decls)
    # the row-mapped forms take the dense entry points' arguments plus lead, row_pixels, zero_pixel, zc (and w)
    assert len(L.SIGNATURES["mia_pool_bn_relu_bwd_apply_rows"][1]) == len(L.SIGNATURES["mia_pool_bn_relu_bwd_apply_ex"][1]) + 4
    assert len(L.SIGNATURES["mia_bn_relu_bwd_apply_rows"][1]) == len(L.SIGNATURES["mia_bn_relu_bwd_apply"][1]) + 5


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_w2_rowmap_memory_contract(cuda, monkeypatch, name):
    for v in ("MIA_POOL_V1", "MIA_POOL_GRID", "MIA_POOL_BWD_PIXEL"):
        monkeypatch.delenv(v, raising=False)
    run_three(cuda, CASES[name][1](cuda), monkeypatch)
