"""GPU: attention with dropout on the probabilities (mia_attn_fwd_dropout / mia_attn_bwd_dropout) and the
element-wise mia_dropout_apply, against the numpy mask functions and float64 formulas of tests/_ast_small_ref.py."""
import functools

import numpy as np
import pytest
import torch

from src.miaudio import lib as L
from tests import _ast_small_ref as R

pytestmark = pytest.mark.gpu

B, H = 2, 3
SCALE = 0.125
SEED = 0x5EED0000A57
NS = [37, 64, 133, 300]
PS = [0.1, 0.5]
DTS = [L.BF16, L.F32]


def _tdt(dt):
    return torch.bfloat16 if dt == L.BF16 else torch.float32


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def fwd(cuda, qkv, N, dt, p, seed, save_q=False):
    """(out (B, N, H, 64), lse (B, H, N), work or None) through mia_attn_fwd_dropout."""
    lib = L.load()
    tq = qkv.to(cuda, _tdt(dt)).contiguous()
    out = torch.empty(B, N, H, 64, dtype=_tdt(dt), device=cuda)
    lse = torch.empty(B, H, N, device=cuda)
    work = None
    if save_q:
        work = torch.empty(int(lib.mia_attn_saved_q_bytes(B, N, H)), dtype=torch.uint8, device=cuda)
    L.check(lib.mia_attn_fwd_dropout(tq.data_ptr(), out.data_ptr(), lse.data_ptr(), L.ptr(work), dt, B, N, H, SCALE, p,
                                     seed, L.stream_ptr()), "mia_attn_fwd_dropout")
    torch.cuda.synchronize()
    return tq, out, lse, work


def bwd(cuda, tq, out, lse, dout, N, dt, p, seed, work=None):
    """dqkv (3, B, H, N, 64) through mia_attn_bwd_dropout; work given = the forward-saved Q' (q_ready)."""
    lib = L.load()
    q_ready = int(work is not None)
    if work is None:
        work = torch.empty(int(lib.mia_attn_bwd_workspace_bytes(dt, B, N, H)), dtype=torch.uint8, device=cuda)
    dqkv = torch.empty_like(tq)
    do = dout.to(cuda, _tdt(dt)).contiguous()
    L.check(lib.mia_attn_bwd_dropout(tq.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                     work.data_ptr(), dt, B, N, H, SCALE, p, seed, q_ready, L.stream_ptr()),
            "mia_attn_bwd_dropout")
    torch.cuda.synchronize()
    return dqkv.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)


@functools.lru_cache(maxsize=None)
def keep_mask(N, p, seed=SEED):
    return R.attn_keep_mask(seed, B, H, N, p)


def _onehot_block(N, j):
    """(N, 64): row r = e_{r - 64 j} for 64 j <= r < 64 j + 64, else 0."""
    m = torch.zeros(N, 64)
    r = torch.arange(64 * j, min(N, 64 * j + 64))
    m[r, r - 64 * j] = 1.0
    return m


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", NS)
def test_mask_extraction(cuda, N, p, dt):
    """Every mask bit each of the three kernels applies, read out of its results with q = 0 (P uniform), equals
    the numpy function: forward through a one-hot V block, dK/dV through a one-hot dO block, dQ through a one-hot
    K block with constant V and dO rows (kept and dropped dS differ by c / N)."""
    M = keep_mask(N, p)
    c = R.attn_scale(p)
    nblk = (N + 63) // 64
    got_f = np.zeros_like(M)
    got_v = np.zeros_like(M)
    got_q = np.zeros_like(M)
    kf = torch.from_numpy(M.mean(-1))  # (B, H, N) kept fraction of each query row
    for j in range(nblk):
        n = min(N, 64 * j + 64) - 64 * j
        e = _onehot_block(N, j)
        # forward: out[b, q, h, d] = c / N * keep(q, 64 j + d)
        qkv = torch.zeros(B, N, 3, H, 64)
        qkv[:, :, 2] = e[None, :, None, :]
        tq, out, lse, _ = fwd(cuda, qkv, N, dt, p, SEED)
        got_f[:, :, :, 64 * j:64 * j + n] = (out.float().cpu().permute(0, 2, 1, 3) != 0).numpy()[..., :n]
        # dK/dV: dV[b, h, k, d] = c / N * keep(64 j + d, k)
        qkv = torch.zeros(B, N, 3, H, 64)
        tq, out, lse, _ = fwd(cuda, qkv, N, dt, p, SEED)
        dout = e[None, :, None, :].expand(B, N, H, 64)
        dv = bwd(cuda, tq, out, lse, dout, N, dt, p, SEED)[2].float().cpu()  # (B, H, k, d)
        got_v[:, :, 64 * j:64 * j + n, :] = (dv != 0).numpy()[..., :n].transpose(0, 1, 3, 2)
        # dQ: dQ[b, h, q, d] = scale / N * (c keep(q, 64 j + d) - c kf(q)): above / below the midpoint c (1/2 - kf)
        qkv = torch.zeros(B, N, 3, H, 64)
        qkv[:, :, 1] = e[None, :, None, :]
        qkv[:, :, 2] = 0.125
        tq, out, lse, _ = fwd(cuda, qkv, N, dt, p, SEED)
        dout = torch.full((B, N, H, 64), 0.125)
        dq = bwd(cuda, tq, out, lse, dout, N, dt, p, SEED)[0].float().cpu()  # (B, H, q, d)
        mid = (SCALE / N * c * (0.5 - kf)).unsqueeze(-1)
        got_q[:, :, :, 64 * j:64 * j + n] = (dq.double() > mid).numpy()[..., :n]
    for name, got in (("forward", got_f), ("dK/dV", got_v), ("dQ", got_q)):
        bad = int((got != M).sum())
        print(f"{name}: {bad} mismatches of {M.size}")
        assert bad == 0, f"{name}: {bad} mask bits differ from the numpy function"


@functools.lru_cache(maxsize=None)
def value_ref(N, p):
    """Random inputs (bf16-representable, shared by both dtypes) and the float64 results under the numpy mask."""
    g = torch.Generator().manual_seed(1000 + N)
    qkv = (torch.randn(B, N, 3, H, 64, generator=g) * 1.5).to(torch.bfloat16).float()
    dout = torch.randn(B, N, H, 64, generator=g).to(torch.bfloat16).float()
    q, k, v = (t.double().requires_grad_(True) for t in qkv.permute(2, 0, 3, 1, 4).unbind(0))
    s = q @ k.transpose(-1, -2) * SCALE
    mask = torch.from_numpy(keep_mask(N, p)).double() * R.attn_scale(p)
    o = (torch.softmax(s, -1) * mask) @ v
    o.backward(dout.double().permute(0, 2, 1, 3))
    return qkv, dout, o.detach(), torch.logsumexp(s.detach(), -1), q.grad, k.grad, v.grad


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("N", NS)
def test_values(cuda, N, p, dt):
    """Forward and backward against the float64 formula under the numpy mask; the tolerances of
    tests/test_gpu_ast.py::test_attention_fwd_bwd.  lse is that of the undropped softmax."""
    qkv, dout, o, lse_ref, dq_ref, dk_ref, dv_ref = value_ref(N, p)
    tq, out, lse, _ = fwd(cuda, qkv, N, dt, p, SEED)
    d = bwd(cuda, tq, out, lse, dout, N, dt, p, SEED)
    tol = 2e-2 if dt == L.BF16 else 1e-5
    errs = dict(out=rel(out.permute(0, 2, 1, 3), o), lse=float((lse.cpu().double() - lse_ref).abs().max()),
                dq=rel(d[0], dq_ref), dk=rel(d[1], dk_ref), dv=rel(d[2], dv_ref))
    print(f"N={N} p={p} dt={dt}: " + " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
    assert errs["out"] < tol and errs["lse"] < tol
    assert errs["dq"] < 3 * tol and errs["dk"] < 3 * tol and errs["dv"] < 3 * tol


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [133, 300])
def test_p0_is_the_existing_path(cuda, N, dt):
    """p = 0 through the new entry points equals the existing entry points bit for bit."""
    lib = L.load()
    qkv, dout = value_ref(N, 0.1)[:2]
    for save_q in ((False, True) if dt == L.BF16 else (False,)):
        tq, out, lse, work = fwd(cuda, qkv, N, dt, 0.0, SEED, save_q=save_q)
        out0 = torch.empty_like(out)
        lse0 = torch.empty_like(lse)
        if save_q:
            work0 = torch.empty_like(work)
            L.check(lib.mia_attn_fwd_save_q(tq.data_ptr(), out0.data_ptr(), lse0.data_ptr(), None, None,
                                            work0.data_ptr(), B, N, H, SCALE, L.stream_ptr()), "fwd_save_q")
        else:
            L.check(lib.mia_attn_fwd(tq.data_ptr(), out0.data_ptr(), lse0.data_ptr(), dt, B, N, H, SCALE,
                                     L.stream_ptr()), "fwd")
        assert torch.equal(out, out0) and torch.equal(lse, lse0)
        d = bwd(cuda, tq, out, lse, dout, N, dt, 0.0, SEED, work=work)
        dq0 = torch.empty_like(tq)
        do = dout.to(cuda, _tdt(dt)).contiguous()
        if save_q:
            L.check(lib.mia_attn_bwd_saved_q(tq.data_ptr(), out0.data_ptr(), do.data_ptr(), lse0.data_ptr(),
                                             dq0.data_ptr(), work0.data_ptr(), B, N, H, SCALE, L.stream_ptr()), "bwd")
        else:
            w = torch.empty(int(lib.mia_attn_bwd_workspace_bytes(dt, B, N, H)), dtype=torch.uint8, device=cuda)
            L.check(lib.mia_attn_bwd(tq.data_ptr(), out0.data_ptr(), do.data_ptr(), lse0.data_ptr(), dq0.data_ptr(),
                                     w.data_ptr(), dt, B, N, H, SCALE, L.stream_ptr()), "bwd")
        torch.cuda.synchronize()
        assert torch.equal(d, dq0.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4))


@pytest.mark.parametrize("dt", DTS)
def test_same_seed_same_bits_other_seed_other_output(cuda, dt):
    N, p = 133, 0.1
    qkv, dout = value_ref(N, p)[:2]
    runs = []
    for seed in (SEED, SEED, SEED + 1):
        tq, out, lse, _ = fwd(cuda, qkv, N, dt, p, seed)
        runs.append((out.clone(), lse.clone(), bwd(cuda, tq, out, lse, dout, N, dt, p, seed).clone()))
    assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[1]))
    assert torch.equal(runs[0][1], runs[2][1])  # lse does not see the mask
    assert not torch.equal(runs[0][0], runs[2][0]) and not torch.equal(runs[0][2], runs[2][2])


@pytest.mark.parametrize("N", [133, 300])
def test_saved_q_equals_prep_path(cuda, N):
    """bf16: the backward on the forward-saved Q' (q_ready) equals the backward that prepares Q' itself."""
    p = 0.1
    qkv, dout = value_ref(N, p)[:2]
    tq, out, lse, work = fwd(cuda, qkv, N, L.BF16, p, SEED, save_q=True)
    tq2, out2, lse2, _ = fwd(cuda, qkv, N, L.BF16, p, SEED)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    a = bwd(cuda, tq, out, lse, dout, N, L.BF16, p, SEED, work=work)
    b = bwd(cuda, tq, out, lse, dout, N, L.BF16, p, SEED)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ mia_dropout_apply
def _apply(cuda, src, res, ddt, p, seed, inplace=False):
    lib = L.load()
    dst = src if inplace else torch.empty(src.shape, dtype=ddt, device=cuda)
    L.check(lib.mia_dropout_apply(src.data_ptr(), L.dtype_code(src), L.ptr(res), dst.data_ptr(), L.dtype_code(dst),
                                  src.numel(), p, seed, L.stream_ptr()), "mia_dropout_apply")
    torch.cuda.synchronize()
    return dst


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
def test_dropout_apply_equals_mia_dropout(cuda, tdt):
    """Same dtype, no residual: the bits of mia_dropout (out of place and in place)."""
    n, p, seed = 3 * 133 * 192 + 5, 0.1, 77
    x = torch.from_numpy(R.hash_uniform(5, (n,))).to(cuda, tdt)
    ref = x.clone()
    L.check(L.load().mia_dropout(ref.data_ptr(), L.dtype_code(ref), n, p, seed, L.stream_ptr()), "mia_dropout")
    assert torch.equal(_apply(cuda, x, None, tdt, p, seed), ref)
    assert torch.equal(_apply(cuda, x.clone(), None, tdt, p, seed, inplace=True), ref)
    keep = torch.from_numpy(R.elem_keep(seed, (n,), p)).to(cuda)
    assert torch.equal(ref != 0, keep & (x != 0))


@pytest.mark.parametrize("sdt,ddt", [(torch.float32, torch.float32), (torch.bfloat16, torch.float32),
                                     (torch.bfloat16, torch.bfloat16)])
def test_dropout_apply_residual_and_cast(cuda, sdt, ddt):
    """With a residual and across dtypes: float64 formula to one rounding of the output type."""
    shape, p, seed = (3, 61, 192), 0.1, 123456789012345
    x = torch.from_numpy(R.hash_uniform(6, shape)).to(cuda, sdt)
    res = torch.from_numpy(R.hash_uniform(7, shape)).to(cuda)
    got = _apply(cuda, x, res, ddt, p, seed)
    keep = torch.from_numpy(R.elem_keep(seed, shape, p)).double()
    want = res.double().cpu() + x.double().cpu() * keep * R.elem_scale(p)
    eps = 2.0 ** -8 if ddt == torch.bfloat16 else 2.0 ** -23  # one rounding of the product + one of the sum
    err = (got.double().cpu() - want).abs()
    assert bool((err <= eps * want.abs().clamp_min(1.0)).all()), float(err.max())
    if sdt == ddt == torch.float32:  # in place on the source
        y = x.clone()
        assert torch.equal(_apply(cuda, y, res, ddt, p, seed, inplace=True), got)
