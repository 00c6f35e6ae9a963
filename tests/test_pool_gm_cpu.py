"""CPU: include/miaudio_pool.h against the ctypes table, the library's exports and the memory-contract cases of
tests/test_gpu_pool_gm_contract.py; host-side argument checks of the two entry points (no device needed: they
return before any launch)."""
import re
from pathlib import Path

from src.miaudio import lib as L
from tests import test_gpu_pool_gm_contract as T

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio_pool.h"


def _decls():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mia_\w+)\s*\(([^)]*)\)\s*;", text))


def test_header_functions_are_exported_bound_and_covered():
    decls = _decls()
    assert set(decls) == {"mia_pool_bwd_gather_ex", "mia_pool_bn_relu_bwd_apply_ex"}
    assert set(decls) <= set(L.SIGNATURES) and set(decls) <= L.exported_symbols()
    for name, params in decls.items():
        assert len(L.SIGNATURES[name][1]) == len(params.split(",")), name
    covered = {n for covers in T.COVERS.values() for n in covers}
    assert covered == set(decls)


def test_ex_signatures_extend_the_plain_ones():
    """The _ex forms take what the entry points of miaudio.h take plus gm's dtype."""
    for name in ("mia_pool_bwd_gather", "mia_pool_bn_relu_bwd_apply"):
        assert len(L.SIGNATURES[name + "_ex"][1]) == len(L.SIGNATURES[name][1]) + 1


def test_gm_dtype_is_checked_on_the_host():
    lib = L.load()
    one = 16  # any non-null, 16-byte aligned value: the calls are refused before a pointer is used
    args = [one, 0, one, one, one, L.F32, 1, 5, 3, 8, 5, 3, one, one, one, one, one]
    assert lib.mia_pool_bwd_gather_ex(*args, L.BF16, one, one, one, None) != 0  # bf16 gm beside f32 activations
    assert b"gm" in lib.mia_last_error_string()
    assert lib.mia_pool_bwd_gather_ex(*args, L.U8, one, one, one, None) != 0
    assert lib.mia_pool_bwd_gather_ex(*args[:16], one + 8, L.F32, one, one, one, None) != 0  # gm alignment
    tail = [one, one, L.BF16, 1, 5, 3, 8, 5, 3, None, one, one, one, one, one, None, None, None]
    assert lib.mia_pool_bn_relu_bwd_apply_ex(one, L.U8, *tail) != 0
    assert b"gm dtype" in lib.mia_last_error_string()
    assert lib.mia_pool_bn_relu_bwd_apply_ex(one + 8, L.BF16, *tail) != 0
    assert b"gm alignment" in lib.mia_last_error_string()
