"""GPU: the stochastic-weight-averaging kernels (include/miaudio_swa.h through K.swa_update / K.swa_transfer) and
BatchNorm's cumulative moving average (momentum=None) in LeafModel and EnvNet-v2.

Update kernel: one table of 1, 3, 4, 7, 1024, 70 001 and 70 000 elements, the last a view one element into its
storage (misaligned: the element-by-element path).  max_numel = 70 001 gives 9 blocks of 256 threads: 17 500 float4
groups over 2304 threads, so every thread runs the 4-way unrolled loop once (1372 of them twice), the one-group loop
takes the remaining groups and one thread the n % 4 tail.  The result must be the bits of avg + (p - avg) / (n + 1)
evaluated in f32 by torch on the CPU.
"""
import numpy as np
import pytest
import torch

from tests import _leaf_model_ref as M
from tests._swa_ref import average_expr
from tests._util import envnet_with_hash_params, rel_err

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 7, 1024, 70_001, 70_000)


def _values(seed, n, other=None):
    """Normal draws with exact zeros, denormals and (given ``other``) elements equal to it."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g)
    idx = torch.arange(n)
    v[idx % 11 == 3] = 0.0
    v[idx % 13 == 5] = 1e-40   # denormal
    v[idx % 17 == 7] = -3e-42
    if other is not None:
        same = idx % 5 == 1
        v[same] = other[same]
    return v


def _place(cuda, vals, misaligned_last=True):
    """Device tensors holding ``vals``; the last one a view one element into its storage."""
    out = []
    for i, v in enumerate(vals):
        if misaligned_last and i == len(vals) - 1:
            store = torch.empty(v.numel() + 1, device=cuda)
            t = store[1:]
            t.copy_(v)
            assert t.data_ptr() % 16 == 4
        else:
            t = v.to(cuda)
            assert t.data_ptr() % 16 == 0
        out.append(t)
    return out


@pytest.fixture(scope="module")
def host_values():
    avg = [_values(100 + i, n) for i, n in enumerate(SIZES)]
    par = [_values(200 + i, n, other=a) for i, (n, a) in enumerate(zip(SIZES, avg))]
    return avg, par


@pytest.mark.parametrize("n_averaged", [0, 1, 2, 9])
def test_update_is_bit_equal_to_the_f32_expression(cuda, host_values, n_averaged):
    from src.miaudio import kernels as K
    avg_h, par_h = host_values
    avg, par = _place(cuda, avg_h), _place(cuda, par_h)
    K.swa_update(avg, par, n_averaged)
    torch.cuda.synchronize()
    for a, p, a0, p0 in zip(avg, par, avg_h, par_h):
        want = average_expr(a0, p0, n_averaged)
        got = a.cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (
            n_averaged, a0.numel(), int((got.view(torch.int32) != want.view(torch.int32)).sum()))
        assert torch.equal(p.cpu().view(torch.int32), p0.view(torch.int32)), "the parameter changed"


def test_update_does_not_depend_on_position_or_alignment(cuda):
    """The same element values in an aligned tensor, in a view at a 4-byte offset, and as the tail of a larger
    tensor (other threads, other loops of the walker): the same bits."""
    from src.miaudio import kernels as K
    n = 70_001
    a0, p0 = _values(1, n), _values(2, n)
    p0[::5] = a0[::5]
    pad = 1027  # the values start at element 1027 of a larger tensor: every element moves to another loop slot
    big_a, big_p = torch.cat([_values(3, pad), a0]), torch.cat([_values(4, pad), p0])
    res = {}
    for name, (av, pv, mis) in {"aligned": ([a0], [p0], False), "offset": ([a0], [p0], True),
                                "moved": ([big_a, _values(5, 7)], [big_p, _values(6, 7)], False)}.items():
        avg, par = _place(cuda, av, mis), _place(cuda, pv, mis)
        K.swa_update(avg, par, 3)
        torch.cuda.synchronize()
        res[name] = avg[0].cpu()[-n:]
    assert torch.equal(res["aligned"].view(torch.int32), res["offset"].view(torch.int32))
    assert torch.equal(res["aligned"].view(torch.int32), res["moved"].view(torch.int32))


@pytest.mark.parametrize("shadowed", ["some", "none"])
def test_transfer_copies_and_rewrites_live_shadows(cuda, host_values, shadowed):
    from src.miaudio import kernels as K
    avg_h, par_h = host_values
    avg = _place(cuda, avg_h)
    par = [torch.nn.Parameter(t) for t in _place(cuda, par_h)]
    live = set()
    if shadowed == "some":  # every second parameter has a live bf16 copy; one more has a stale one
        for i in (0, 2, 4, 5):
            K.bf16_shadow(par[i])
            live.add(i)
        K.bf16_shadow(par[3])
        par[3]._mia_bf16_ver = par[3]._version - 1
    K.swa_transfer(par, avg)
    torch.cuda.synchronize()
    for i, (p, a0) in enumerate(zip(par, avg_h)):
        assert torch.equal(p.detach().cpu().view(torch.int32), a0.view(torch.int32)), i
        assert torch.equal(avg[i].cpu().view(torch.int32), a0.view(torch.int32)), "the average changed"
        if i in live:
            assert p._mia_bf16_ver == p._version
            assert torch.equal(p._mia_bf16.cpu().view(torch.int16), a0.to(torch.bfloat16).view(torch.int16)), i
        # whatever the state before, the copy the next forward takes is the transferred parameter's
        assert torch.equal(K.bf16_shadow(p).cpu().view(torch.int16), a0.to(torch.bfloat16).view(torch.int16)), i


def test_entry_points_reject_bad_tables(cuda):
    from src.miaudio import lib as L
    lib = L.load()
    t = torch.zeros(4, dtype=torch.int64, device=cuda)
    assert lib.mia_swa_update(None, t.data_ptr(), t.data_ptr(), 1, 4, 0, L.stream_ptr()) < 0
    assert b"swa_update" in lib.mia_last_error_string()
    assert lib.mia_swa_update(t.data_ptr(), t.data_ptr(), t.data_ptr(), 1, 4, -1, L.stream_ptr()) < 0
    assert lib.mia_swa_transfer(t.data_ptr(), None, None, t.data_ptr(), 1, 4, L.stream_ptr()) < 0
    assert lib.mia_swa_transfer(t.data_ptr(), t.data_ptr(), None, t.data_ptr(), 0, 4, L.stream_ptr()) < 0


# ------------------------------------------------------------------ BatchNorm cumulative moving average
def _bns(m):
    return [mod for mod in m.modules() if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm)]


@pytest.fixture(scope="module")
def leaf_case():
    """LeafModel (fixture case M1's filters and initial state) at the golden clip length, B = 4: three inputs, and
    the restatement's running statistics after three cumulative updates in float64 and (the floor) in float32."""
    gm = dict(np.load(M.__file__.replace("_leaf_model_ref.py", "golden/golden_leaf_model.npz"), allow_pickle=False))
    d, _, _, state = M.case(gm, "M1")
    assert d["T"] == 160 * 94 + 37
    xs = [torch.from_numpy(M.case_waveform(7100 + i, 4, d["T"])) for i in range(3)]

    def restate(dtype):
        sd = M.tensors(state, dtype, grad=False)
        keep = M.MOMENTUM
        try:
            with torch.no_grad():
                for k, x in enumerate(xs, 1):
                    M.MOMENTUM = 1.0 / k  # the restatement's update factor: cumulative average
                    _, _, running = M.model_step(sd, x, None, d["Kt"], d["pool"])
                    sd.update(running)
        finally:
            M.MOMENTUM = keep
        return {k: v for k, v in sd.items() if "running_" in k}

    ref = restate(torch.float64)
    floor = {}
    before = torch.get_num_threads()
    try:
        for th in M.FLOOR_THREADS:
            torch.set_num_threads(th)
            r32 = restate(torch.float32)
            for k in ref:
                floor[k] = max(floor.get(k, 0.0), rel_err(r32[k], ref[k]))
    finally:
        torch.set_num_threads(before)
    return d, state, xs, ref, floor


def test_leaf_cumulative_average(cuda, leaf_case):
    """The bound on the running statistics is test_gpu_leaf_model.py's for the f32 mode: 10 x the float32 floor of
    the restatement against its float64 evaluation."""
    from src.models.leaf import LeafModel
    d, state, xs, ref, floor = leaf_case
    m = LeafModel(n_filters=d["F"], kernel_size=d["Kt"], num_classes=d["C"], compute_dtype="f32")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in state.items()}, strict=True)
    m = m.to(cuda).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0  # the restatement has no dropout (as test_gpu_leaf_model.py's build())
    for bn in _bns(m):
        bn.momentum = None
    with torch.no_grad():
        for x in xs:
            m(x[:, None, :].to(cuda))
    assert [int(bn.num_batches_tracked) for bn in _bns(m)] == [3] * 6
    sd = m.state_dict()
    over = {}
    for k, want in ref.items():
        err = rel_err(sd[k].cpu().numpy(), want.numpy())
        print(f"leaf cma {k:34s} err {err:.3e} floor {floor[k]:.3e} bound {10 * floor[k]:.3e}")
        assert floor[k] <= 1e-3
        if err > 10 * floor[k]:
            over[k] = (err, 10 * floor[k])
    assert not over, over
    # counter and statistics zeroed: the next forward's factor is 1, the running statistics ARE its batch statistics
    # -- whatever was there before (0 * old + 1 * batch), so a second start from other contents gives the same bits
    got = []
    for fill in (0.0, 3.0):
        for bn in _bns(m):
            bn.num_batches_tracked.zero_()
            bn.running_mean.fill_(fill)
            bn.running_var.fill_(fill)
        with torch.no_grad():
            m(xs[0][:, None, :].to(cuda))
        assert [int(bn.num_batches_tracked) for bn in _bns(m)] == [1] * 6
        got.append({k: v.clone() for k, v in m.state_dict().items() if "running_" in k})
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k
    conv1 = M.tensors(state, torch.float64, grad=False)
    keep = M.MOMENTUM
    try:
        M.MOMENTUM = 1.0
        with torch.no_grad():
            _, _, one = M.model_step(conv1, xs[0], None, d["Kt"], d["pool"])
    finally:
        M.MOMENTUM = keep
    for k, want in one.items():
        assert rel_err(got[0][k].cpu().numpy(), want.numpy()) <= max(10 * floor[k], 1e-6), k


def _oracle_params():
    """The oracle's parameter dict on the shared hash weights, with running buffers of its own (its forward updates
    them in place)."""
    from tests._util import hash_params
    return {k: torch.from_numpy(v.copy() if "running_" in k else v) for k, v in hash_params().items()}


def test_envnet_cumulative_average(cuda):
    """EnvNet-v2 at B = 2 against the oracle's forward with the update factor 1 / k, at the tolerance
    test_gpu_envnet.py uses for the running statistics (rtol 1e-3, atol 1e-4)."""
    from oracle import envnet as oenv
    from oracle.synth import synth_waveform
    m = envnet_with_hash_params(cuda).train()
    for bn in _bns(m):
        bn.momentum = None
    xs = [torch.from_numpy(synth_waveform(40 + i, 2, 220_500)[:, None, :]) for i in range(3)]
    conv_only = _oracle_params()
    with torch.no_grad():
        for k, x in enumerate(xs, 1):
            m(x.to(cuda))
            oenv.forward(conv_only, x, training=True, dropout_p=0.0, momentum=1.0 / k)
            if k == 1:  # factor 1: the oracle's batch statistics of xs[0]
                one = {n: v.clone() for n, v in conv_only.items() if "running_" in n}
    assert [int(bn.num_batches_tracked) for bn in _bns(m)] == [3] * 10
    sd = m.state_dict()
    for k, v in conv_only.items():
        if "running_" in k:
            np.testing.assert_allclose(sd[k].cpu().numpy(), v.numpy(), rtol=1e-3, atol=1e-4, err_msg=k)
    got = []
    for fill in (0.0, 3.0):
        for bn in _bns(m):
            bn.num_batches_tracked.zero_()
            bn.running_mean.fill_(fill)
            bn.running_var.fill_(fill)
        with torch.no_grad():
            m(xs[0].to(cuda))
        got.append({k: v.clone() for k, v in m.state_dict().items() if "running_" in k})
    assert [int(bn.num_batches_tracked) for bn in _bns(m)] == [1] * 10
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k
    for k, v in one.items():
        np.testing.assert_allclose(got[0][k].cpu().numpy(), v.numpy(), rtol=1e-3, atol=1e-4, err_msg=k)


def test_float_momentum_is_unchanged_and_envnet_does_not_count(cuda):
    from oracle.synth import synth_waveform
    m = envnet_with_hash_params(cuda).train()
    with torch.no_grad():
        m(torch.from_numpy(synth_waveform(21, 2, 220_500)[:, None, :]).to(cuda))
    assert [int(bn.num_batches_tracked) for bn in _bns(m)] == [0] * 10
    assert all(not hasattr(bn, "_mia_cma") for bn in _bns(m))
