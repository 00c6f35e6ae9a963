"""GPU: FusedSGD (mia_clip_sgd / mia_gemm_sgd) and FusedAdamW (mia_clip_adamw / mia_gemm_adamw) against the installed
torch's clip_grad_norm_ + torch.optim.SGD / torch.optim.AdamW on the same device -- rtol 1e-5 / atol 1e-6 on the
parameters and 1e-5 relative on the norm, what tests/test_gpu_optim.py holds FusedAdam to -- and the deferred
weight-gradient forms against the materialised gradient, bit for bit.  FusedAdam (mia_clip_adam / mia_gemm_adam) runs
the same walker and the same GEMM epilogue, so it takes the misaligned, shadow, precomputed-sum, deferred and
position-independence cases beside them."""
import pytest
import torch

from oracle.synth import synth_waveform
from src.miaudio import kernels as K
from src.miaudio import lib as L
from src.training.optim import FusedAdam, FusedAdamW, FusedSGD
from tests._util import envnet_with_hash_params

pytestmark = pytest.mark.gpu

SIZES = (1003, 4096, 7, 300_001)  # scalar tail, aligned body, a tiny tensor, more than one block per tensor


def _make(cuda, seed, sizes=SIZES, misaligned=False):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(n, generator=g) for n in sizes]
    if misaligned:  # views at a 4-byte offset: the kernels' element-by-element path
        ps = [torch.nn.Parameter(torch.cat([v.new_zeros(1), v]).to(cuda)[1:]) for v in vals]
        assert all(p.data_ptr() % 16 == 4 for p in ps)
    else:
        ps = [torch.nn.Parameter(v.to(cuda)) for v in vals]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    return g, ps, ref


def _run_against_torch(cuda, g, ps, ref, opt, ropt, clip, steps=3, skip=None):
    for it in range(steps):
        for i, (p, r) in enumerate(zip(ps, ref)):
            if skip == (it, i):
                p.grad = r.grad = None
                continue
            gr = torch.randn(p.shape, generator=g).to(cuda)
            p.grad, r.grad = gr.clone(), gr.clone()
        opt.step()
        live = [r for r in ref if r.grad is not None]
        total = torch.nn.utils.clip_grad_norm_(live, clip if clip else float("inf"))
        ropt.step()
        torch.cuda.synchronize()
        assert abs(float(opt.last_total_norm) - float(total)) <= 1e-5 * float(total), it
        for p, r in zip(ps, ref):
            assert torch.allclose(p, r, rtol=1e-5, atol=1e-6), (it, p.numel())


SGD_CASES = [dict(momentum=m, nesterov=n, weight_decay=wd)
             for m, n in ((0.0, False), (0.9, False), (0.9, True)) for wd in (0.0, 1e-4)]
SGD_CASES.append(dict(momentum=0.9, dampening=0.1, weight_decay=1e-4))


@pytest.mark.parametrize("clip", [0.0, 0.5])
@pytest.mark.parametrize("kw", SGD_CASES, ids=lambda kw: "-".join(f"{k[0]}{v}" for k, v in kw.items()))
def test_sgd_matches_torch(cuda, kw, clip):
    g, ps, ref = _make(cuda, 0)
    opt = FusedSGD(ps, lr=0.05, clip=clip, **kw)
    _run_against_torch(cuda, g, ps, ref, opt, torch.optim.SGD(ref, lr=0.05, **kw), clip)
    for p in ps:
        assert set(opt.state[p]) == ({"momentum_buffer"} if kw["momentum"] else set())


@pytest.mark.parametrize("clip", [0.0, 0.5])
def test_adamw_matches_torch(cuda, clip):
    g, ps, ref = _make(cuda, 1)
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=1e-2, clip=clip)
    _run_against_torch(cuda, g, ps, ref, opt, torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2), clip)


@pytest.mark.parametrize("which", ["sgd", "sgd-plain", "adamw", "adam"])
def test_misaligned_views_take_the_scalar_path(cuda, which):
    g, ps, ref = _make(cuda, 2, misaligned=True)
    if which == "adamw":
        opt, ropt = FusedAdamW(ps, lr=1e-2, clip=0.5), torch.optim.AdamW(ref, lr=1e-2)
    elif which == "adam":
        opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-2, clip=0.5)
        ropt = torch.optim.Adam(ref, lr=1e-2, weight_decay=1e-2)
    else:
        kw = dict(momentum=0.9, nesterov=True, weight_decay=1e-4) if which == "sgd" else {}
        opt, ropt = FusedSGD(ps, lr=0.05, clip=0.5, **kw), torch.optim.SGD(ref, lr=0.05, **kw)
    _run_against_torch(cuda, g, ps, ref, opt, ropt, 0.5)


def _family(which, ps):
    if which == "adam":
        return FusedAdam(ps, lr=1e-2, weight_decay=1e-2, clip=0.5), ("exp_avg", "exp_avg_sq")
    if which == "adamw":
        return FusedAdamW(ps, lr=1e-2, weight_decay=1e-2, clip=0.5), ("exp_avg", "exp_avg_sq")
    if which == "sgd":
        return FusedSGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4, clip=0.5), ("momentum_buffer",)
    return FusedSGD(ps, lr=0.05, weight_decay=1e-4, clip=0.5), ()


@pytest.mark.parametrize("which", ["adam", "adamw", "sgd", "sgd-plain"])
def test_update_does_not_depend_on_position_or_alignment(cuda, which):
    """The same values once in 16-B aligned tensors and once in views at a 4-byte offset, the same (aligned)
    gradients, 3 steps: parameters, state and norm agree bit for bit.  At 300 001 elements the grid is 37 blocks of
    256 threads, so the aligned tensor runs the unrolled loop, the one-group remainder loop and a one-element tail;
    1003 takes the remainder loop and a 3-element tail, 7 one group and a 3-element tail; every element of an offset
    view goes through the element-by-element loop.  Every multiply-add of a rule is an explicit fmaf
    (csrc/optim_update.h), so no loop can be contracted differently from another."""
    _, pa, _ = _make(cuda, 11)
    _, pm, _ = _make(cuda, 11, misaligned=True)
    (oa, names), (om, _) = _family(which, pa), _family(which, pm)
    g = torch.Generator().manual_seed(12)
    for it in range(3):
        for a, m in zip(pa, pm):
            a.grad = torch.randn(a.shape, generator=g).to(cuda)
            m.grad = a.grad.clone()
        oa.step()
        om.step()
        torch.cuda.synchronize()
        assert torch.equal(oa.last_total_norm, om.last_total_norm), it
        for a, m in zip(pa, pm):
            assert torch.equal(a, m), (it, a.numel())
            for k in names:
                assert torch.equal(oa.state[a][k], om.state[m][k]), (it, a.numel(), k)


def test_sgd_buffer_of_a_parameter_that_missed_step_one_starts_at_step_two(cuda):
    """torch creates a momentum buffer at the parameter's first gradient (buf = g, no dampening); the fused step
    carries that as mia_clip_sgd's first_use table.  Dampening makes a wrong first use visible."""
    kw = dict(momentum=0.9, dampening=0.1, weight_decay=1e-4)
    g, ps, ref = _make(cuda, 3, sizes=(515, 64, 3))
    opt, ropt = FusedSGD(ps, lr=0.05, **kw), torch.optim.SGD(ref, lr=0.05, **kw)
    _run_against_torch(cuda, g, ps, ref, opt, ropt, 0.0, steps=4, skip=(0, 1))
    for p, r in zip(ps, ref):
        assert torch.allclose(opt.state[p]["momentum_buffer"], ropt.state[r]["momentum_buffer"], rtol=1e-5, atol=1e-6)


def test_adamw_per_parameter_steps_and_table_reuse(cuda):
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in (515, 64, 3)]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = FusedAdamW(ps, lr=1e-2, weight_decay=1e-2)
    ropt = torch.optim.AdamW(ref, lr=1e-2, weight_decay=1e-2)
    grads = [torch.empty_like(p) for p in ps]  # fixed storage: the table key stays the same
    for it in range(5):
        for i, (p, r) in enumerate(zip(ps, ref)):
            if it == 1 and i == 1:  # parameter 1 misses step 1
                p.grad = r.grad = None
                continue
            grads[i].copy_(torch.randn(p.shape, generator=g).to(cuda))
            p.grad, r.grad = grads[i], grads[i].clone()
        opt.step()
        ropt.step()
        torch.cuda.synchronize()
        for p, r in zip(ps, ref):
            assert torch.allclose(p, r, rtol=1e-5, atol=1e-6), it
    assert [int(opt.state[p]["step"]) for p in ps] == [5, 4, 5]
    # builds: step 0 (3 tensors), step 1 (2 tensors), steps 2-4 (per-tensor counts, same pointers)
    assert opt.table_builds == 3


def test_sgd_table_reuse(cuda):
    g = torch.Generator().manual_seed(6)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in (515, 64)]
    opt = FusedSGD(ps, lr=0.05, momentum=0.9)
    grads = [torch.randn(p.shape, generator=g).to(cuda) for p in ps]
    for it in range(4):
        for p, gr in zip(ps, grads):
            p.grad = gr
        opt.step()
    # the buffers exist from step 0 on and keep their storage: one table for all four steps
    assert opt.table_builds == 1


@pytest.mark.parametrize("which", ["sgd", "sgd-plain", "adamw", "adam"])
def test_step_refreshes_bf16_shadow(cuda, which):
    g, ps, ref = _make(cuda, 7, sizes=(1003, 4096, 7))
    sh0 = K.bf16_shadow(ps[1])  # live copy on one tensor only
    sh2 = K.bf16_shadow(ps[0])  # and one on the tensor with a scalar tail
    if which == "adamw":
        opt = FusedAdamW(ps, lr=1e-2, clip=1.0)
    elif which == "adam":
        opt = FusedAdam(ps, lr=1e-2, weight_decay=1e-2, clip=1.0)
    else:
        opt = FusedSGD(ps, lr=0.05, clip=1.0, **(dict(momentum=0.9, nesterov=True) if which == "sgd" else {}))
    for it in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g).to(cuda)
        opt.step()
        torch.cuda.synchronize()
        for p, s0 in ((ps[1], sh0), (ps[0], sh2)):
            sh = K.bf16_shadow(p)
            assert sh.data_ptr() == s0.data_ptr()  # no recast: the update pass wrote it
            assert torch.equal(sh, p.detach().to(torch.bfloat16))
    with torch.no_grad():
        ps[1].mul_(2.0)  # any other in-place change invalidates the copy
    assert torch.equal(K.bf16_shadow(ps[1]), ps[1].detach().to(torch.bfloat16))


M, N, KD = 256, 384, 128  # the smallest legal deferred GEMM with two row tiles and three column tiles


def _operands(cuda, g):
    a = torch.randn(KD, M, generator=g).to(torch.bfloat16).to(cuda)
    b = torch.randn(KD, N, generator=g).to(torch.bfloat16).to(cuda)
    return a, b


def _materialise(w, a, b):
    dW = torch.empty(M, N, dtype=torch.float32, device=w.device)
    sq = K.sqsum_slots(dW, M, N)
    K.gemm(K.dense(a, L.RC, KD, M), K.dense(b, L.RC, KD, N), K.epilogue(dW, N, sqsum=sq), M, N, KD, L.BF16, split_k=1)
    K.tag_sqsum(w, dW, sq)
    return dW, sq


OPTIMIZERS = {
    "sgd": (lambda ps: FusedSGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4, clip=0.5),
            lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4),
            ("momentum_buffer",)),
    "adamw": (lambda ps: FusedAdamW(ps, lr=1e-2, weight_decay=1e-2, clip=0.5),
              lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=1e-2), ("exp_avg", "exp_avg_sq")),
    "adam": (lambda ps: FusedAdam(ps, lr=1e-2, weight_decay=1e-2, clip=0.5),
             lambda ps: torch.optim.Adam(ps, lr=1e-2, weight_decay=1e-2), ("exp_avg", "exp_avg_sq")),
}


@pytest.mark.parametrize("which", list(OPTIMIZERS))
def test_precomputed_sqsum(cuda, which):
    """A gradient tagged with its GEMM's per-tile sums of squares is not re-read by the norm pass; the step matches
    torch's clip + optimizer."""
    fused, torch_opt, _ = OPTIMIZERS[which]
    g = torch.Generator().manual_seed(8)
    ps = [torch.nn.Parameter((0.05 * torch.randn(M, N, generator=g)).to(cuda)),
          torch.nn.Parameter(torch.randn(77, generator=g).to(cuda))]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt, ropt = fused(ps), torch_opt(ref)
    for it in range(3):
        a, b = _operands(cuda, g)
        dW, sq = _materialise(ps[0], a, b)
        assert K.valid_sqsum(ps[0], dW) is sq
        gb = torch.randn(77, generator=g).to(cuda)
        ps[0].grad, ps[1].grad = dW, gb.clone()
        ref[0].grad, ref[1].grad = dW.clone(), gb.clone()
        opt.step()
        assert opt.last_precomputed == 1 and opt.last_deferred == 0
        total = torch.nn.utils.clip_grad_norm_(ref, 0.5)
        ropt.step()
        torch.cuda.synchronize()
        assert abs(float(opt.last_total_norm) - float(total)) <= 1e-5 * float(total)
        for p, r in zip(ps, ref):
            assert torch.allclose(p, r, rtol=1e-5, atol=1e-6)
        assert ps[0]._mia_sqsum is None  # consumed


def _three_steps(cuda, which, defer):
    fused, _, names = OPTIMIZERS[which]
    g = torch.Generator().manual_seed(9)
    w = torch.nn.Parameter((0.05 * torch.randn(M, N, generator=g)).to(cuda))
    bias = torch.nn.Parameter(torch.randn(77, generator=g).to(cuda))
    sh = K.bf16_shadow(w)
    opt = fused([w, bias])
    norms = []
    for it in range(3):
        a, b = _operands(cuda, g)
        if defer:  # as a model's backward hands it over
            K.defer_weight_grad(w, K.dense(a, L.RC, KD, M), K.dense(b, L.RC, KD, N), M, N, KD, keep=(a, b))
        else:
            w.grad, _ = _materialise(w, a, b)
        bias.grad = torch.randn(77, generator=g).to(cuda)
        opt.step()
        assert (opt.last_deferred, opt.last_precomputed) == ((1, 1) if defer else (0, 1))
        assert w._mia_deferred is None
        w.grad = None
        norms.append(float(opt.last_total_norm))
        assert K.bf16_shadow(w).data_ptr() == sh.data_ptr()
    torch.cuda.synchronize()
    return norms, [t.detach().clone() for t in (w, bias, sh, *(opt.state[w][k] for k in names))]


@pytest.mark.parametrize("which", list(OPTIMIZERS))
def test_deferred_form_is_bit_identical_to_the_materialised_gradient(cuda, which):
    """The guarantee tests/test_gpu_deferred_wgrad.py gives for Adam: the same GEMM main loop and the same update
    arithmetic run in both forms, so parameter, moments, shadow and norm agree bit for bit after 3 steps."""
    n1, s1 = _three_steps(cuda, which, True)
    n0, s0 = _three_steps(cuda, which, False)
    assert n1 == n0, (n1, n0)
    for a, b in zip(s1, s0):
        assert torch.equal(a, b)
    assert torch.equal(s1[2], s1[0].to(torch.bfloat16))


class _Shard:  # stands in for GradAllReducer: records what the optimizer reports
    def __init__(self):
        self.calls = []

    def after_shard_update(self, param, shadow, d):
        self.calls.append((param, shadow, d))


@pytest.mark.parametrize("which", list(OPTIMIZERS))
def test_row_slice_of_a_deferred_gradient_updates_only_its_rows(cuda, which):
    """A deferred gradient that covers rows [row0, row0 + M/2) of the parameter (GradAllReducer fc1_exchange="shard"):
    those rows end as in the whole-tensor deferred step on the same operands, bit for bit, every other row of
    parameter, moments and shadow keeps its value, and the shard object is told."""
    fused, _, names = OPTIMIZERS[which]
    r0, Ms = 128, 128
    out = []
    for sliced in (True, False):
        g = torch.Generator().manual_seed(10)
        w = torch.nn.Parameter((0.05 * torch.randn(M, N, generator=g)).to(cuda))
        bias = torch.nn.Parameter(torch.randn(77, generator=g).to(cuda))
        before = w.detach().clone()
        sh = K.bf16_shadow(w)
        opt = fused([w, bias])
        a, b = _operands(cuda, g)
        shard = _Shard()
        if sliced:
            sq = torch.empty(int(L.load().mia_gemm_sqsum_slots(M, N)), dtype=torch.float64, device=cuda)
            per = sq.numel() // 2  # slots are row-block-major: a slice's slots are contiguous
            B = K.dense(b, L.RC, KD, N)
            for r in (0, 1):  # the other slice's sums arrive by all-gather in a real run
                K.gemm_sqsum_only(K.dense(a[:, r * Ms:], L.RC, KD, Ms, ld=M), B, Ms, N, KD, sq[r * per:(r + 1) * per])
            w._mia_deferred = dict(A=K.dense(a[:, r0:], L.RC, KD, Ms, ld=M), B=B, M=Ms, N=N, K=KD, sq=sq,
                                   keep=(a, b), row0=r0, rows_total=M, shard=shard)
        else:
            K.defer_weight_grad(w, K.dense(a, L.RC, KD, M), K.dense(b, L.RC, KD, N), M, N, KD, keep=(a, b))
        bias.grad = torch.randn(77, generator=g).to(cuda)
        opt.step()
        torch.cuda.synchronize()
        assert opt.last_deferred == 1
        if sliced:
            assert len(shard.calls) == 1 and shard.calls[0][0] is w and shard.calls[0][1].data_ptr() == sh.data_ptr()
            assert shard.calls[0][2]["row0"] == r0
            assert torch.equal(w[:r0], before[:r0]) and not torch.equal(w[r0:], before[r0:])
            assert torch.equal(sh[:r0], before[:r0].to(torch.bfloat16))
            for k in names:
                assert not opt.state[w][k][:r0].any()  # rows of another rank: untouched zeros
        out.append((float(opt.last_total_norm), [t.detach().clone() for t in
                                                 (w, sh, bias, *(opt.state[w][k] for k in names))]))
    assert out[0][0] == out[1][0]
    for t_s, t_f in zip(out[0][1], out[1][1]):
        if t_s.dim() == 2:
            assert torch.equal(t_s[r0:], t_f[r0:])
        else:
            assert torch.equal(t_s, t_f)


def test_envnet_fc1_stays_deferred_under_fused_sgd(cuda):
    B = 64
    x = torch.from_numpy(synth_waveform(33, B, 220_500)[:, None, :]).to(cuda)
    y = torch.zeros(B, 50, device=cuda)
    y[torch.arange(B), torch.arange(B) % 50] = 1.0
    m = envnet_with_hash_params(cuda, compute_dtype="bf16").train()
    opt = FusedSGD(m.parameters(), lr=0.01, momentum=0.9, nesterov=True, weight_decay=5e-4, clip=1.0)
    fc1 = dict(m.named_parameters())["classifier.1.weight"]
    before = fc1.detach().clone()
    for _ in range(2):
        z = m(x)
        loss, dz, _ = K.soft_ce(z.detach().float().contiguous(), y, input_sigmoid=False)
        z.backward(dz)
        assert fc1.grad is None and fc1._mia_deferred is not None
        opt.step()
        opt.zero_grad(set_to_none=True)
        assert opt.last_deferred == 1
        assert torch.isfinite(loss).all() and torch.isfinite(opt.last_total_norm).all()
    assert torch.isfinite(fc1).all() and not torch.equal(fc1.detach(), before)
    assert set(opt.state[fc1]) == {"momentum_buffer"}
