"""GPU: the memory contract of include/miaudio_resample.h, with the harness of tests/test_gpu_memory_contract.py.

``out`` is taken from the guarded arena at exactly ``B * ldo`` floats; the call runs three times (poison 0xFF, poison
0x00, plain buffers); the guards stay clean and ``[0, Tout)`` of every row is bit-identical across the runs.  The
slack columns ``[Tout, ldo)`` are not written by contract and keep whatever the buffer held, so they are left out
of the comparison.  mia_resample takes no workspace.

COVERS maps every case to the entry points it calls; tests/test_resample_cpu.py checks it against the header.
"""
import pytest
import torch

from tests.test_gpu_memory_contract import F32, Ctx, p, rnd, run_three  # noqa: F401  (Ctx: the harness's run object)

CASES = {}


def _case(name, o, n, width, B, T, ldx, slack, lengths):
    def build(dev):
        K = 2 * width + o
        x = rnd(dev, (B, ldx), F32, 90)
        taps = rnd(dev, (n, K), F32, 91, scale=0.1)
        lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
        Tout = -(-n * T // o)

        def run(ctx):
            assert ctx.lib.mia_resample_out_len(T, o, n) == Tout
            out = ctx.out("out", (B, Tout + slack), F32, compare=False)
            ctx.outs["out[:, :Tout]"] = out[:, :Tout]
            ctx.call("mia_resample", p(x), ldx, B, T, p(lens), p(taps), o, n, width, p(out), Tout + slack, Tout)
        return run
    CASES[name] = (("mia_resample",), build)


# the last frame tile and the last phase tile are ragged in each; 1201 samples of 441 -> 160 end inside a tile's
# first frames, 5000 of 160 -> 441 cross a frame tile of 128
_case("resample[441-160]", 441, 160, 17, 3, 60_000, 60_007, 5, None)
_case("resample[441-160-lengths]", 441, 160, 17, 3, 60_000, 60_007, 5, [60_000, 0, 1201])
_case("resample[160-441]", 160, 441, 7, 3, 21_000, 21_001, 3, None)
_case("resample[160-441-lengths]", 160, 441, 7, 3, 21_000, 21_001, 3, [5000, 21_000, 1])
_case("resample[2-1-ldo=Tout]", 2, 1, 13, 2, 4097, 4097, 0, None)
_case("resample[1-2-lengths]", 1, 2, 7, 2, 3000, 3000, 1, [2999, 77])

COVERS = {name: covers for name, (covers, _) in CASES.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_resample_memory_contract(cuda, monkeypatch, name):
    run_three(cuda, CASES[name][1](cuda), monkeypatch)
