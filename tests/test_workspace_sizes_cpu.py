"""CPU: the size functions of include/miaudio.h (``*_bytes`` / ``*_slots`` / ``*_blocks`` / ``*_offset``).

They are pure host functions, so the library is loaded without a GPU (as tests/test_gemm_dispatch.py does).  Over a
small grid of arguments: results are non-negative and non-decreasing in each size argument, rejected geometry gives
the documented sentinel, and the relations between the functions that the header states hold.  Where the header
states a size in prose next to a function (conv3_wgrad), both are computed here and must agree.

tests/test_gpu_memory_contract.py checks on the GPU that the kernels stay inside these sizes.
"""
import itertools
import re
from pathlib import Path

import pytest

from src.miaudio import lib as L
from tests import test_gemm_dispatch as D

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio.h"
F32, BF16 = L.F32, L.BF16

# name -> (grid per argument, indices of the size arguments the result must not decrease in, valid(args))
# Every combination of the grid is evaluated; monotonicity compares neighbours along one argument between two
# argument tuples that are both valid geometry.
ALWAYS = lambda *a: True  # noqa: E731
GRIDS = {
    "mia_gemm_workspace_bytes": ([[1, 37, 256, 4096], [1, 50, 384, 4096], [1, 2, 3, 16]], (0, 1, 2), ALWAYS),
    "mia_gemm_sqsum_slots": ([[1, 127, 128, 129, 300, 4096], [1, 128, 200, 84480]], (0, 1), ALWAYS),
    "mia_gemm_mxfp8_workspace_bytes": ([[1, 255, 256, 300, 4096], [32, 768, 3072], [0, 1]], (0, 1, 2), ALWAYS),
    "mia_logmel_workspace_bytes": ([[1, 3, 64], [1, 12, 13, 216, 1379]], (0, 1), ALWAYS),
    "mia_bn_partial_bytes": ([[1, 5000, 70_000, 10_000_000], [8, 32, 64, 256]], (0, 1), ALWAYS),
    "mia_conv3_wgrad_workspace_bytes": ([[4, 8, 1024, 4096]], (0,), ALWAYS),
    "mia_adam_workspace_bytes": ([[1, 2, 3, 100, 65535]], (0,), ALWAYS),
    "mia_adam_coef_offset": ([[1, 2, 3, 100, 65535]], (0,), ALWAYS),
    "mia_layernorm_partial_bytes": ([[1, 5, 300, 4113, 65536], [6, 384, 768, 1000, 1024]], (0, 1), ALWAYS),
    "mia_attn_bwd_workspace_bytes": ([[F32, BF16], [1, 2, 3, 64], [1, 37, 64, 65, 77, 257, 300, 1214], [1, 2, 3, 12]],
                                     (1, 2, 3), ALWAYS),
    "mia_attn_saved_q_bytes": ([[1, 2, 3, 64], [1, 37, 64, 65, 77, 257, 300, 1214], [1, 2, 3, 12]], (0, 1, 2), ALWAYS),
    "mia_attn_bwd_chain_bytes": ([[1, 2, 3, 64], [1, 37, 64, 65, 77, 257, 300, 1214], [1, 2, 3, 12]], (0, 1, 2), ALWAYS),
    "mia_attn_bwd_error_offset": ([[1, 2, 3, 64], [1, 37, 64, 65, 77, 257, 300, 1214], [1, 2, 3, 12]], (0, 1, 2), ALWAYS),
    # forward (the packed bank): non-decreasing in B, T, F and Kt.  The backward is a number of slabs times the
    # bank size, and the number of slabs is ceil(frames / ceil(frames / cap)): "for exactly this call", it is
    # not monotonic in the frame count (500 frames give 500 slabs, 6890 frames 493), nor in Kt (which also picks
    # the kernel).  test_leaf_backward_workspace_bounds states what does hold for it.
    "mia_leaf_workspace_bytes": ([[1, 2, 8], [1024, 5000, 16000, 220_500], [1, 5, 40, 64], [3, 17, 401, 1023],
                                  [32, 160, 1024], [0]], (0, 1, 2, 3),
                                 lambda B, T, F, Kt, pool, bwd: T >= pool),
    "mia_pcen_workspace_bytes": ([[1, 2, 8, 65535], [1, 5, 40, 1024]], (0, 1), ALWAYS),
    "mia_lt_stats_blocks": ([[1, 2, 8, 64], [5, 68, 1000, 5512], [8, 32, 384, 1024], [1, 2, 5]], (0, 1),
                            lambda n, t, c, k: t >= k),
    "mia_lt_workspace_bytes": ([[8, 32, 384, 1024]], (0,), ALWAYS),
}
# needs a device (the CU count); covered by the GPU memory-contract test
DEVICE_ONLY = {"mia_mfma_rate_sink_floats"}
# takes descriptors, not sizes: covered by tests/test_gemm_dispatch.py's table and test_ex_covers_split_k below
DESCRIPTOR = {"mia_gemm_workspace_bytes_ex"}


def size_functions_in_header():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(?:int64_t|int32_t)\s+(mia_\w+)\s*\(", text))


def test_every_size_function_of_the_header_is_covered():
    names = size_functions_in_header()
    assert names, "no size function found: the header's declarations changed shape"
    assert all(re.search(r"_(bytes|bytes_ex|slots|blocks|offset|floats)$", n) for n in names), sorted(names)
    assert names == set(GRIDS) | DEVICE_ONLY | DESCRIPTOR
    assert names <= set(L.SIGNATURES)


@pytest.mark.parametrize("name", list(GRIDS))
def test_non_negative_and_non_decreasing(name):
    fn = getattr(L.load(), name)
    grid, mono, valid = GRIDS[name]
    val = {a: int(fn(*a)) for a in itertools.product(*grid) if valid(*a)}
    assert val
    for a, v in val.items():
        assert v >= 0, f"{name}{a} = {v}"
    for a, v in val.items():
        for i in mono:
            k = grid[i].index(a[i])
            if k + 1 < len(grid[i]):
                b = a[:i] + (grid[i][k + 1],) + a[i + 1:]
                if b in val:
                    assert val[b] >= v, f"{name}{b} = {val[b]} < {name}{a} = {v}"


def test_sizes_that_must_be_positive():
    lib = L.load()
    assert lib.mia_gemm_workspace_bytes(37, 50, 1) == 0 and lib.mia_gemm_workspace_bytes(37, 50, 3) == 3 * 37 * 50 * 4
    assert lib.mia_gemm_sqsum_slots(256, 384) == 6 and lib.mia_gemm_sqsum_slots(300, 200) == 6
    assert lib.mia_gemm_mxfp8_workspace_bytes(300, 768, 0) == 0 < lib.mia_gemm_mxfp8_workspace_bytes(300, 768, 1)
    for name, args in [("mia_logmel_workspace_bytes", (3, 12)), ("mia_bn_partial_bytes", (5000, 32)),
                       ("mia_adam_workspace_bytes", (1,)), ("mia_layernorm_partial_bytes", (5, 768)),
                       ("mia_attn_bwd_workspace_bytes", (F32, 1, 77, 2)), ("mia_attn_bwd_workspace_bytes", (BF16, 1, 77, 2)),
                       ("mia_attn_saved_q_bytes", (1, 77, 2)), ("mia_attn_bwd_chain_bytes", (1, 77, 2)),
                       ("mia_leaf_workspace_bytes", (2, 5000, 5, 17, 160, 0)),
                       ("mia_leaf_workspace_bytes", (2, 5000, 5, 17, 160, 1)), ("mia_pcen_workspace_bytes", (2, 5)),
                       ("mia_lt_stats_blocks", (2, 68, 32, 5)), ("mia_lt_workspace_bytes", (384,))]:
        assert getattr(lib, name)(*args) > 0, (name, args)


@pytest.mark.parametrize("B,T,F,Kt,pool", [a for a in itertools.product([1, 2, 8], [1024, 5000, 16000, 220_500],
                                                                         [1, 5, 40, 64], [3, 17, 401, 1023],
                                                                         [32, 160, 1024]) if a[1] >= a[4]])
def test_leaf_backward_workspace_bounds(B, T, F, Kt, pool):
    """Between one and min(frames, 512) slabs of the bank's size [2][F][Kt] f32, plus at most the packed bf16
    bank of the MFMA form (8 KiB per 64 filters x 32 taps tile)."""
    ws = L.load().mia_leaf_workspace_bytes(B, T, F, Kt, pool, 1)
    bank = 2 * F * Kt * 4
    frames = B * (T // pool)
    assert bank <= ws <= min(frames, 512) * bank + 8192 * ((F + 63) // 64) * ((Kt + 31) // 32)


# ------------------------------------------------------------------------------------------- sentinels
@pytest.mark.parametrize("args", [(2, 5000, 5, 16, 160), (2, 5000, 5, 1, 160), (2, 5000, 5, 1025, 160),
                                  (2, 5000, 5, 17, 100), (2, 5000, 5, 17, 0), (2, 5000, 5, 17, 2048),
                                  (2, 100, 5, 17, 160), (0, 5000, 5, 17, 160), (2, 5000, 0, 17, 160),
                                  (-1, 5000, 5, 17, 160)])
@pytest.mark.parametrize("backward", [0, 1])
def test_leaf_workspace_rejects_with_minus_one(args, backward):
    assert L.load().mia_leaf_workspace_bytes(*args, backward) == -1


@pytest.mark.parametrize("args", [(0, 5), (2, 0), (-1, 5), (2, -3), (0, 0)])
def test_pcen_workspace_rejects_with_minus_one(args):
    assert L.load().mia_pcen_workspace_bytes(*args) == -1


@pytest.mark.parametrize("C", [0, 1, 4, 7, 12, 33, -8])
def test_bn_partial_rejects_with_zero(C):
    assert L.load().mia_bn_partial_bytes(5000, C) == 0


@pytest.mark.parametrize("c", [0, 4, 7, 12, 1032, 2048, -8])
def test_lt_functions_reject_with_zero(c):
    lib = L.load()
    assert lib.mia_lt_workspace_bytes(c) == 0
    assert lib.mia_lt_stats_blocks(2, 68, c, 5) == 0


@pytest.mark.parametrize("args", [(0, 68, 32, 5), (2, 68, 32, 0), (2, 4, 32, 5), (-1, 68, 32, 5)])
def test_lt_stats_blocks_rejects_with_zero(args):
    assert L.load().mia_lt_stats_blocks(*args) == 0


# ------------------------------------------------------------------------------------------- relations
def test_ex_covers_split_k():
    """mia_gemm_workspace_bytes_ex >= mia_gemm_workspace_bytes(M, N, split_k) for split-K on paths 0-5, over the
    dispatch table's rows."""
    lib = L.load()
    seen = set()
    for name, (A, B, E, M, N, Kd, cd, split) in D.CASES.items():
        path = lib.mia_gemm_path(A, B, M, N, Kd, cd, split)
        if split < 2 or path not in (0, 1, 2, 3, 4, 5):
            continue
        ex = lib.mia_gemm_workspace_bytes_ex(A, B, E, M, N, Kd, cd, split)
        assert ex >= lib.mia_gemm_workspace_bytes(M, N, split), name
        seen.add(path)
    assert {0, 2, 3, 5} <= seen, seen  # the paths that take split_k >= 2 all appear


@pytest.mark.parametrize("n", [1, 2, 3, 100, 65535])
def test_adam_coef_word_lies_inside_the_workspace(n):
    lib = L.load()
    off = lib.mia_adam_coef_offset(n)
    assert off >= 0 and off % 4 == 0
    assert off + 4 <= lib.mia_adam_workspace_bytes(n)


ATTN = list(itertools.product([1, 2, 3, 64], [1, 37, 64, 65, 77, 257, 300, 1214], [1, 2, 3, 12]))


@pytest.mark.parametrize("B,N,H", ATTN)
def test_attention_workspace_layout(B, N, H):
    lib = L.load()
    ws = lib.mia_attn_bwd_workspace_bytes(BF16, B, N, H)
    off = lib.mia_attn_bwd_error_offset(B, N, H)
    assert off % 4 == 0 and off + 4 <= ws
    saved = lib.mia_attn_saved_q_bytes(B, N, H)
    assert saved <= ws
    assert saved <= off  # the error word is not part of the state kept from the forward
    assert lib.mia_attn_bwd_workspace_bytes(F32, B, N, H) == B * N * H * 4


@pytest.mark.parametrize("nwaves", [4, 8, 1024, 4096])
def test_conv3_wgrad_prose_and_function_agree(nwaves):
    """The header gives mia_conv3_wgrad's workspace as `nwaves*2048 + 64*4096` floats and says that
    mia_conv3_wgrad_workspace_bytes(nwaves) is that plus mia_conv3_wgrad_bn's nwaves*32 floats."""
    text = HEADER.read_text()
    assert "nwaves*2048 + 64*4096 floats" in text and "nwaves*32 floats" in text
    prose = (nwaves * 2048 + 64 * 4096) * 4
    assert L.load().mia_conv3_wgrad_workspace_bytes(nwaves) == prose + nwaves * 32 * 4
