"""CPU: every exported entry point of include/miaudio.h that takes caller-owned output or scratch memory has a
case in tests/test_gpu_memory_contract.py.  A new entry point without one fails here."""
import re
from pathlib import Path

from src.miaudio import lib as L
from tests import test_gpu_memory_contract as T

HEADER = Path(__file__).resolve().parents[1] / "include" / "miaudio.h"
# writes only into host memory of the caller (a C string buffer): nothing for a device arena to guard
HOST_ONLY = {"mia_device_arch"}


def _writes_caller_memory(params: str) -> bool:
    for prm in params.split(","):
        prm = " ".join(prm.split())
        if "*" not in prm:
            continue
        if prm.startswith(("const MiaEpilogue*", "const MiaPackJob*")):  # descriptors that carry output pointers
            return True
        if not prm.startswith("const "):  # void*, float*, uint8_t*, double*, uint32_t*, void* const* tables
            return True
    return False


def entry_points_with_caller_memory():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    decls = re.findall(r"\bint\s+(mia_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert len(decls) >= 80, "the header's declarations changed shape"
    return {name for name, params in decls if _writes_caller_memory(params)} - HOST_ONLY


def test_parser_sorts_the_known_ones():
    names = entry_points_with_caller_memory()
    assert {"mia_gemm", "mia_splitk_reduce", "mia_pack_weights", "mia_clip_adam", "mia_fe_conv2_wgrad", "mia_soft_ce",
            "mia_attn_bwd_onepass", "mia_lt_pcen_bwd", "mia_mfma_rate", "mia_dropout"} <= names
    assert "mia_gemm_path" not in names and "mia_device_arch" not in names and "mia_last_error_string" not in names


def test_every_entry_point_with_caller_memory_has_a_case():
    names = entry_points_with_caller_memory()
    covered = T.covered_entry_points()
    assert not names - covered, f"no memory-contract case for {sorted(names - covered)}"
    assert covered <= set(L.SIGNATURES), sorted(covered - set(L.SIGNATURES))
    assert not covered - names, f"cases name entry points the header does not declare as such: {sorted(covered - names)}"


def test_case_ids_are_unique_and_name_their_entry_points():
    assert len(T.CASES) == len(T.COVERS) and all(T.COVERS.values())
