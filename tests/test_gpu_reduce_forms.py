"""GPU: the two forms of the slab reduces and of the soft-label loss compute the same bits.

mia_fe_conv2_wgrad and mia_conv3_wgrad end in a fixed-order sum of per-workgroup / per-wave slabs, mia_soft_ce in
a fixed-order sum of per-row losses.  The default forms keep that order and only overlap the load latency (groups
of 16 slabs in registers, rows spread over the chip); MIA_REDUCE_V1=1 selects the earlier kernels.  Both run on
the same inputs and every output must be `torch.equal`.  The default form is also checked against a float64 sum
of the very slabs it reduced (read back from the workspace), within the bound the existing tests of these kernels
use (tests/test_gpu_gemm.py::test_fe_conv2_wgrad 1e-3, tests/test_gpu_norm.py::test_conv3_wgrad 1e-4), and
soft_ce against the oracle as tests/test_gpu_loss.py does."""
import pytest
import torch

from oracle import train as otrain
from src.miaudio import kernels as K
from src.miaudio import lib as L

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("n", [1, 3, 17, 300])
def test_fe_conv2_wgrad_reduce_forms(cuda, monkeypatch, n):
    """One slab per workgroup, one workgroup per clip here (w2 = 100 pixels: one 128-pixel item a clip), so 1, 3 and
    17 slabs; n = 300 gives one slab per CU (256 on an MI355X)."""
    w1 = 214
    w2 = (w1 - 16) // 2 + 1
    g = torch.Generator().manual_seed(n)
    y1 = torch.randn(n * w1, 32, generator=g).to(torch.bfloat16).to(cuda)
    dy = (torch.randn(n * w2, 64, generator=g) * 0.1).to(torch.bfloat16).to(cuda)
    slabs_max = min(n, 512)
    lib = L.load()
    res = []
    for v1 in (False, True):
        if v1:
            monkeypatch.setenv("MIA_REDUCE_V1", "1")
        else:
            monkeypatch.delenv("MIA_REDUCE_V1", raising=False)
        ws = torch.zeros(slabs_max, 64 * 512, device=cuda)  # zero: slabs no workgroup owns add nothing below
        dw = torch.full((64, 512), float("nan"), device=cuda)
        L.check(lib.mia_fe_conv2_wgrad(dy.data_ptr(), y1.data_ptr(), None, None, dw.data_ptr(), n, w1, w2,
                                       ws.data_ptr(), ws.numel() * 4, L.stream_ptr()), "mia_fe_conv2_wgrad")
        torch.cuda.synchronize()
        res.append((dw, ws))
    monkeypatch.delenv("MIA_REDUCE_V1")
    (dw, ws), (dw1, ws1) = res
    assert torch.equal(ws, ws1)  # the same slabs went in
    assert torch.equal(dw, dw1)
    assert torch.isfinite(dw).all()
    assert rel(dw.view(-1), ws.double().sum(0)) < 1e-3


@pytest.mark.parametrize("nslab", [4, 12, 68, 100, 256, 1300, 4096])
def test_conv3_wgrad_reduce_forms(cuda, monkeypatch, nslab):
    """nslab = the caller's wave count (a multiple of 4).  Stage 1 gives each of its 64 groups ceil(nslab / 64)
    slabs: 4 and 12 leave most groups empty, 68 and 100 do not divide into the groups (a short or empty tail
    group), 1300 gives 21 a group (one register batch of 16 and a remainder of 5, the last group 19), 4096 is
    EnvNet's."""
    n, h, wd = 2, 12, 40
    g = torch.Generator(device=cuda).manual_seed(nslab)
    x = torch.randn(n, h, wd, generator=g, device=cuda).to(torch.bfloat16)
    dy = torch.randn(n * (h - 7) * (wd - 7), 32, generator=g, device=cuda).to(torch.bfloat16)
    lib = L.load()
    res = []
    for v1 in (False, True):
        if v1:
            monkeypatch.setenv("MIA_REDUCE_V1", "1")
        else:
            monkeypatch.delenv("MIA_REDUCE_V1", raising=False)
        part = torch.zeros(int(lib.mia_conv3_wgrad_workspace_bytes(nslab)) // 4, device=cuda)
        dw = torch.full((32, 64), float("nan"), device=cuda)
        L.check(lib.mia_conv3_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), part.data_ptr(), nslab, n, h, wd,
                                    L.stream_ptr()), "mia_conv3_wgrad")
        torch.cuda.synchronize()
        res.append((dw, part))
    monkeypatch.delenv("MIA_REDUCE_V1")
    (dw, part), (dw1, part1) = res
    # the slabs and the stage-1 sums, as raw words (half of an f64 read as f32 can be a NaN pattern)
    assert torch.equal(part.view(torch.int32), part1.view(torch.int32))
    assert torch.equal(dw, dw1)
    assert torch.isfinite(dw).all()
    assert rel(dw.view(-1), part[: nslab * 2048].view(nslab, 2048).double().sum(0)) < 1e-4


@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("M,N,Kd", [(2048, 1024, 4096), (256, 512, 16384), (264, 264, 20 * 1024 + 40)])
def test_mgemm_split_k_reduce_forms(cuda, monkeypatch, odt, M, N, Kd):
    """The split-K weight-gradient GEMM (both operands k-by-m; the split is a fixed function of the shape: 4, 16
    and 19 slabs here -- after slab 0 no register batch of 8, one and a remainder of 7, two and a remainder of 2)
    ends in a slab-order sum; 256 x 512 is an EnvNet shape, 264 x 264 ragged tiles; a strided output.  Against an
    fp32 matmul of the same bf16 operands within the bound of tests/test_gpu_gemm.py::test_mgemm_wgrad_split_k."""
    g = torch.Generator(device=cuda).manual_seed(M + N + Kd)
    a = torch.randn(M, Kd, generator=g, device=cuda).to(torch.bfloat16)
    b = torch.randn(N, Kd, generator=g, device=cuda).to(torch.bfloat16)
    A, Bo = K.dense(a.t().contiguous(), L.RC, Kd, M), K.dense(b.t().contiguous(), L.RC, Kd, N)
    assert L.load().mia_gemm_path(A, Bo, M, N, Kd, L.BF16, 1) == 7
    outs = []
    for v1 in (False, True):
        if v1:
            monkeypatch.setenv("MIA_REDUCE_V1", "1")
        else:
            monkeypatch.delenv("MIA_REDUCE_V1", raising=False)
        full = torch.full((M, N + 64), float("nan"), dtype=odt, device=cuda)
        K.gemm(A, Bo, K.epilogue(full[:, :N], N + 64), M, N, Kd, L.BF16)
        torch.cuda.synchronize()
        outs.append(full)
    monkeypatch.delenv("MIA_REDUCE_V1")
    assert torch.isnan(outs[0][:, N:].float()).all()  # nothing written past N
    assert torch.equal(outs[0][:, :N], outs[1][:, :N])
    assert rel(outs[0][:, :N].float(), a.float() @ b.float().t()) < (1e-5 if odt == torch.float32 else 1e-2)


def _labels(B, C, g):
    y = torch.zeros(B, C, dtype=torch.float64)
    lab = torch.randint(0, C, (B,), generator=g)
    y[torch.arange(B), lab] = 1.0
    r = torch.rand(B, generator=g, dtype=torch.float64)
    mix = torch.arange(B) % 3 == 1  # BC mixing: r / 1 - r on two different classes
    other = (lab + 1 + torch.randint(0, C - 1, (B,), generator=g)) % C
    y[mix, lab[mix]] = r[mix]
    y[mix, other[mix]] = 1 - r[mix]
    return y


@pytest.mark.parametrize("input_sigmoid", [False, True], ids=["logits", "sigmoid"])
@pytest.mark.parametrize("C", [10, 50])
@pytest.mark.parametrize("B", [1, 5, 256])
def test_soft_ce_forms(cuda, monkeypatch, B, C, input_sigmoid):
    g = torch.Generator().manual_seed(B * 100 + C)
    logits = (torch.randn(B, C, generator=g) * 4).float()
    y = _labels(B, C, g)
    res = []
    for v1 in (False, True):
        if v1:
            monkeypatch.setenv("MIA_REDUCE_V1", "1")
        else:
            monkeypatch.delenv("MIA_REDUCE_V1", raising=False)
        out = K.soft_ce(logits.to(cuda), y.float().to(cuda), input_sigmoid=input_sigmoid)
        torch.cuda.synchronize()
        res.append([t.clone() for t in out])
    monkeypatch.delenv("MIA_REDUCE_V1")
    for a, b, what in zip(res[0], res[1], ("loss", "dlogits", "correct")):
        assert torch.equal(a, b), f"{what} differs between the forms"
    loss, dlogits, correct = res[0]
    z = logits.double().requires_grad_(True)
    ref = otrain.soft_ce(torch.sigmoid(z) if input_sigmoid else z, y)
    ref.backward()
    ref = ref.detach()
    assert abs(float(loss) - float(ref)) <= 2e-6 * max(1.0, abs(float(ref)))
    torch.testing.assert_close(dlogits.cpu().double(), z.grad, rtol=1e-4, atol=1e-7)
    assert int(correct) == int((logits.argmax(1) == y.argmax(1)).sum())
