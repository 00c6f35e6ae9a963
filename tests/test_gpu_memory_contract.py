"""GPU: the memory contract of include/miaudio.h, one case per entry point.

The header promises that the caller owns all memory and that a size function (or a prose formula) gives the bytes
exactly one call needs.  The value tests cannot see a broken promise: ``kernels.workspace`` over-allocates and
reuses its buffers, torch's allocator pads and packs, and most outputs have nothing behind them that anyone looks
at.  Here every caller-owned buffer of a call -- outputs, side outputs, workspaces, partial slabs, saved state --
comes from ``tests/_arena.py`` at exactly its documented size, between two poisoned 1 MiB guards.

Each case runs three times on the same inputs:
  1. arena, poison 0xFF (every float word a NaN);
  2. arena, poison 0x00;
  3. plain ``torch.empty`` buffers with workspaces of four times the documented size, or (GEMM, model steps) the
     unpatched ``kernels`` wrapper.
and asserts: return code 0, both arenas' guards untouched, every output and side output bit-identical across the
three runs.  Bit identity says that the result depends neither on what a workspace held before nor on placement or
slack, and that every element the header calls written is written (an unwritten byte differs between the two
poisons).  The header claims fixed-order sums throughout, so equality of bits is the contract, not a tolerance.
Values are not checked against float64 here; the other GPU tests do that.

Entry points reached through a ``kernels`` wrapper that calls ``kernels.workspace`` (mia_gemm, the model steps) run
with ``kernels.workspace`` replaced by ``arena.take(nbytes)``: exact, fresh per call, no 256-byte floor, no slack.
Everything else is called through ctypes with arena pointers.  The error words that the header requires to be
zero before the first call (mia_logmel_fwd, mia_attn_bwd_onepass) are zeroed by the test.

No kernel is ever handed a buffer smaller than documented.  The one undersized call, mia_fe_conv2_wgrad a slab
short, is rejected by the host before any launch.  An overrun longer than a guard (1 MiB; 64 KiB in the model
steps) is outside this file's reach.

COVERS maps every case to the entry points it calls; tests/test_memory_contract_table_cpu.py checks it against the
header.
"""
import ctypes
import functools
import math

import pytest
import torch

from src.miaudio import kernels as K
from src.miaudio import lib as L
from tests._arena import GuardDamage, GuardedArena

F32, BF16, F64, U8, I32, I64 = torch.float32, torch.bfloat16, torch.float64, torch.uint8, torch.int32, torch.int64

CASES = {}  # id -> (entry points, build(dev) -> run(ctx))


def case(name, *covers):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = (covers, fn)
        return fn
    return deco


def covered_entry_points():
    return {n for covers, _ in CASES.values() for n in covers}


class Ctx:
    """One run of a case: hands out the caller-owned buffers (arena, or plain torch in run 3)."""

    def __init__(self, dev, poison):
        self.dev = dev
        self.arena = GuardedArena(dev, poison) if poison is not None else None
        self.outs = {}
        self.lib = L.load()

    def out(self, name, shape, dtype, align=256, offset=0, compare=True):
        """An output / side output / in-out buffer of exactly its documented shape (compared across the runs)."""
        if self.arena is not None:
            t = self.arena.take_as(name, shape, dtype, align, offset)
        else:
            shape = (shape,) if isinstance(shape, int) else tuple(shape)
            item = torch.empty((), dtype=dtype).element_size()
            assert offset % item == 0
            flat = torch.empty(math.prod(shape) + offset // item, dtype=dtype, device=self.dev)
            t = flat[offset // item:].view(shape)
        if compare:
            assert name not in self.outs, name
            self.outs[name] = t
        return t

    def ws(self, name, nbytes, align=256):
        """A workspace / partial slab / saved state of exactly ``nbytes`` (four times that in the plain run)."""
        nbytes = int(nbytes)
        assert nbytes >= 0, (name, nbytes)
        if self.arena is not None:
            return self.arena.take(name, nbytes, align)
        return torch.empty(4 * nbytes + 256, dtype=U8, device=self.dev)

    def workspace(self, nbytes, device, slot="main"):  # stands in for kernels.workspace
        return self.ws(f"kernels.workspace[{slot}]", nbytes)

    def call(self, fn, *args):
        rc = getattr(self.lib, fn)(*args, L.stream_ptr())
        assert rc == 0, f"{fn} returned {rc}: {(self.lib.mia_last_error_string() or b'').decode()}"


def _bytes(t):
    return t.reshape(-1).view(U8)


def _diff(a, b):
    bad = (a != b).nonzero().flatten()
    return f"{bad.numel()} of {a.numel()} bytes differ, first at byte {int(bad[0])}, last at byte {int(bad[-1])}"


def run_three(dev, run, monkeypatch, chunk=None):
    res = []
    for poison in (0xFF, 0x00, None):
        ctx = Ctx(dev, poison)
        if chunk is not None and ctx.arena is not None:
            ctx.arena = GuardedArena(dev, poison, chunk_bytes=chunk)
        with monkeypatch.context() as mp:
            if poison is not None:
                mp.setattr(K, "workspace", ctx.workspace)
            run(ctx)
        torch.cuda.synchronize()
        if ctx.arena is not None:
            ctx.arena.check()
        res.append({k: _bytes(v).clone() for k, v in ctx.outs.items()})
        del ctx
    ff, zz, plain = res
    assert ff.keys() == zz.keys() == plain.keys() and ff
    for k in ff:
        assert torch.equal(ff[k], zz[k]), (f"'{k}' differs between poison 0xFF and 0x00 ({_diff(ff[k], zz[k])}): the "
                                           "call read memory it never wrote, or left part of the output unwritten")
        assert torch.equal(ff[k], plain[k]), f"'{k}' differs between the arena and the plain run ({_diff(ff[k], plain[k])})"


def rnd(dev, shape, dtype=F32, seed=0, scale=1.0, shift=0.0):
    g = torch.Generator(device=dev).manual_seed(1000 + seed)
    return (torch.randn(shape, generator=g, device=dev) * scale + shift).to(dtype)


def uni(dev, shape, lo, hi, seed=0):
    g = torch.Generator(device=dev).manual_seed(2000 + seed)
    return torch.rand(shape, generator=g, device=dev) * (hi - lo) + lo


def code(dt):
    return {F32: L.F32, BF16: L.BF16, U8: L.U8}[dt]


def p(t):
    return None if t is None else t.data_ptr()


def bn_state(x, gamma, beta, eps=1e-5):
    """(mean, invstd, scale, shift) of a (P, C) map, f32, formed with torch (inputs of the backward cases)."""
    xf = x.float()
    mean = xf.mean(0)
    invstd = (xf.var(0, unbiased=False) + eps).rsqrt()
    scale = gamma * invstd
    return mean.contiguous(), invstd.contiguous(), scale.contiguous(), (beta - mean * scale).contiguous()


# ================================================================================================ GEMM
def _gemm_case(dev, M, N, Kd, la=L.KC, lb=L.KC, cd=L.BF16, split=None, odt=F32, path=None, seed=0, **epi):
    """A dense GEMM through K.gemm.  epi: colsum / a_colsum / sqsum (bool), act + aux dtype."""
    dt = BF16 if cd == L.BF16 else F32
    a = rnd(dev, (M, Kd) if la == L.KC else (Kd, M), dt, seed)
    b = rnd(dev, (N, Kd) if lb == L.KC else (Kd, N), dt, seed + 1)
    aux = rnd(dev, (M, N), BF16, seed + 2) if epi.get("act") else None

    def operands():
        ra, ca = (M, Kd) if la == L.KC else (Kd, M)
        rb, cb = (N, Kd) if lb == L.KC else (Kd, N)
        return K.dense(a, la, ra, ca), K.dense(b, lb, rb, cb)

    if path is not None:
        A, Bo = operands()
        assert L.load().mia_gemm_path(A, Bo, M, N, Kd, cd, split or 1) == path

    def run(ctx):
        A, Bo = operands()
        out = ctx.out("C", (M, N), odt)
        kw = {}
        if epi.get("colsum"):
            kw["colsum"] = ctx.out("colsum", N, F32)
        if epi.get("a_colsum"):
            kw["a_colsum"] = ctx.out("a_colsum", M, F32)
        if epi.get("sqsum"):
            kw["sqsum"] = ctx.out("sqsum", int(ctx.lib.mia_gemm_sqsum_slots(M, N)), F64)
        if aux is not None:
            kw.update(act=epi["act"], aux=aux, ldaux=N)
        K.gemm(A, Bo, K.epilogue(out, N, **kw), M, N, Kd, cd, split_k=split)
    return run


def _g(name, *args, **kw):
    case(name, "mia_gemm")(lambda dev: _gemm_case(dev, *args, **kw))


_g("gemm[p0-splitk3-f32]", 37, 50, 200, cd=L.F32, split=3, path=0)
_g("gemm[p0-splitk3-bf16]", 37, 50, 200, cd=L.BF16, split=3, path=0)
_g("gemm[p0-splitk3-bf16-rc]", 37, 50, 200, la=L.RC, lb=L.RC, split=3, path=0, odt=BF16)
_g("gemm[p5-splitk4]", 256, 384, 4096, split=4, path=5)
# (1024, 256, 512) has 4 tiles of 256 x 256: under the 256x256 kernel's 32-tile floor it runs on the 128x128 kernel
# with a column-sum pass; (2085, 1024, 128) is 9 x 4 ragged tiles of the 256x256 kernel and its fused column sums
_g("gemm[dact_mul-colsum-1024x256x512]", 1024, 256, 512, odt=BF16, path=5, act=L.DACT_MUL, colsum=True)
_g("gemm[p7-dact_mul-colsum]", 2085, 1024, 128, odt=BF16, path=7, act=L.DACT_MUL, colsum=True)
_g("gemm[p7-rcrc-wgrad-a_colsum-own-splitk]", 1024, 256, 16384 + 40, la=L.RC, lb=L.RC, path=7, a_colsum=True)
_g("gemm[a_colsum-outside-p7]", 520, 264, 300, la=L.RC, lb=L.RC, a_colsum=True)
_g("gemm[colsum-outside-p7]", 900, 640, 256, odt=BF16, path=5, colsum=True)
_g("gemm[sqsum-256x384]", 256, 384, 128, sqsum=True)
_g("gemm[sqsum-ragged-300x200]", 300, 200, 64, sqsum=True)
_g("gemm[sqsum-ragged-splitk]", 300, 200, 2048, sqsum=True, split=2)
# a bf16 output with N % 8 == 4 and ldc == N: the last row ends at the buffer end
_g("gemm[bf16-out-n%8=4-p0]", 37, 52, 64, odt=BF16, path=0)
_g("gemm[bf16-out-n%8=4-p5]", 296, 204, 192, odt=BF16)
_g("gemm[bf16-out-n%8=4-36-tiles]", 2085, 1028, 128, odt=BF16, path=5)  # the 256x256 kernel takes N % 8 == 0 only


def _conv_wgrad_case(dev, n, cin, cout, h, w, kh, kw_, sw, pre, path):
    """Row-window / tap weight gradients (paths 2 and 3): split-K slabs in the workspace."""
    oh, ow = h - kh + 1, (w - kw_) // sw + 1
    x = rnd(dev, (n, h, w, cin), F32 if cin == 1 and kh == 1 else BF16, 3)  # conv1 reads the f32 waveform
    dy = rnd(dev, (n, oh, ow, cout), BF16, 4)
    sc, sh = uni(dev, cin, 0.5, 1.5, 5), rnd(dev, cin, F32, 6, 0.1)
    P, Kc = n * oh * ow, kh * kw_ * cin

    def operands():
        A = K.dense(dy, L.RC, P, cout)
        if cin == 1 and kh == 1:  # conv1 pair view of the waveform
            Bo = K.conv(x.view(n, w), L.RC, n, 1, w // 2, 2, 1, ow, 1, 32, row_kind=True)
        elif cin == 1:
            Bo = K.conv(x.view(n, h, w), L.RC, n, h, w, 1, oh, ow, kh, kw_, row_kind=True)
        else:
            Bo = K.conv(x, L.RC, n, h, w, cin, oh, ow, kh, kw_, sw=sw, pre=L.PRE_AFFINE_RELU if pre else L.PRE_NONE,
                        scale=sc if pre else None, shift=sh if pre else None)
        return A, Bo

    A, Bo = operands()
    assert L.load().mia_gemm_path(A, Bo, cout, Kc, P, L.BF16, 2) == path

    def run(ctx):
        A, Bo = operands()
        dW = ctx.out("dW", (cout, Kc), F32)
        K.gemm(A, Bo, K.epilogue(dW, Kc), cout, Kc, P, L.BF16)
    return run


for _name, _args in [("gemm[p2-rowwgrad-1x4]", (3, 32, 64, 4, 300, 1, 4, 1, True, 2)),
                     ("gemm[p2-rowwgrad-1x16-s2]", (2, 32, 32, 1, 901, 1, 16, 2, False, 2)),
                     ("gemm[p2-wgrad8]", (2, 32, 32, 12, 300, 8, 8, 1, True, 2)),
                     ("gemm[p3-tapwgrad-conv1]", (3, 1, 32, 1, 2 * 701 + 64, 1, 64, 2, False, 3)),
                     ("gemm[p3-tapwgrad-conv3]", (2, 1, 32, 12, 300, 8, 8, 1, False, 3))]:
    case(_name, "mia_gemm")(functools.partial(lambda dev, a: _conv_wgrad_case(dev, *a), a=_args))


@case("gemm_sqsum_only+gemm_adam[256x384x128]", "mia_gemm_sqsum_only", "mia_gemm_adam")
def _sqsum_adam(dev):
    M, N, Kd = 256, 384, 128
    dy, x = rnd(dev, (Kd, M), BF16, 7), rnd(dev, (Kd, N), BF16, 8)
    p0, m0, v0 = rnd(dev, (M, N), F32, 9), rnd(dev, (M, N), F32, 10, 0.01), uni(dev, (M, N), 0.0, 1e-3, 11)
    coef = torch.tensor([0.37], device=dev)

    def run(ctx):
        A, Bo = K.dense(dy, L.RC, Kd, M), K.dense(x, L.RC, Kd, N)
        sq = ctx.out("sqsum", int(ctx.lib.mia_gemm_sqsum_slots(M, N)), F64)
        ctx.call("mia_gemm_sqsum_only", A, Bo, M, N, Kd, p(sq))
        pp, mm, vv = ctx.out("param", (M, N), F32), ctx.out("exp_avg", (M, N), F32), ctx.out("exp_avg_sq", (M, N), F32)
        sh = ctx.out("shadow_bf16", (M, N), BF16)
        pp.copy_(p0), mm.copy_(m0), vv.copy_(v0)
        ctx.call("mia_gemm_adam", A, Bo, M, N, Kd, p(pp), p(mm), p(vv), p(sh), N, p(coef), 1e-3, 0.0316, 0.9, 0.999, 1e-8,
                 1e-4)
    return run


def _mx_case(dev, M, N, Kd, what):
    a = K.mx_quantize(rnd(dev, (M, Kd), BF16, 12))
    b = K.mx_quantize(rnd(dev, (N, Kd), BF16, 13))
    aux = uni(dev, (M, N), -0.1, 1.1, 14).to(BF16)

    def run(ctx):
        out = ctx.out("C", (M, N), BF16)
        if what == "colsum":
            cs = ctx.out("colsum", N, F32)
            E = K.epilogue(out, N, act=L.DACT_MUL, aux=aux, ldaux=N, colsum=cs)
            ws = ctx.ws("workspace", ctx.lib.mia_gemm_mxfp8_workspace_bytes(M, N, 1))
            ctx.call("mia_gemm_mxfp8_ex", p(a.q), p(a.scales), Kd, p(b.q), p(b.scales), Kd, E, M, N, Kd, p(ws))
        else:
            mx = K.MXTensor(ctx.out("mx_q", (M, N), U8), ctx.out("mx_scales", (M, N // 32), U8))
            E = K.epilogue(out, N, act=L.ACT_GELU, mx=mx)
            ctx.call("mia_gemm_mxfp8", p(a.q), p(a.scales), Kd, p(b.q), p(b.scales), Kd, E, M, N, Kd)
    return run


case("gemm_mxfp8_ex[colsum-300x768x768]", "mia_gemm_mxfp8_ex")(lambda dev: _mx_case(dev, 300, 768, 768, "colsum"))
case("gemm_mxfp8[mx-epilogue-copy-300x768x768]", "mia_gemm_mxfp8")(lambda dev: _mx_case(dev, 300, 768, 768, "mx"))


@case("gemm[p7-mx-epilogue-copy]", "mia_gemm")
def _p7_mx(dev):
    M, N, Kd = 2085, 1024, 128
    a, b = rnd(dev, (M, Kd), BF16, 15), rnd(dev, (N, Kd), BF16, 16)
    assert L.load().mia_gemm_path(K.dense(a, L.KC, M, Kd), K.dense(b, L.KC, N, Kd), M, N, Kd, L.BF16, 1) == 7

    def run(ctx):
        out = ctx.out("C", (M, N), BF16)
        u = ctx.out("aux(gelu_save)", (M, N), BF16)
        mx = K.MXTensor(ctx.out("mx_q", (M, N), U8), ctx.out("mx_scales", (M, N // 32), U8))
        K.gemm(K.dense(a, L.KC, M, Kd), K.dense(b, L.KC, N, Kd), K.epilogue(out, N, act=L.ACT_GELU_SAVE, aux=u, ldaux=N, mx=mx),
               M, N, Kd, L.BF16)
    return run


@case("splitk_reduce[37x50-s3]", "mia_splitk_reduce")
def _splitk(dev):
    M, N, S = 37, 50, 3
    slabs, bias = rnd(dev, (S, M, N), F32, 17), rnd(dev, N, F32, 18)

    def run(ctx):
        for odt in (F32, BF16):
            out = ctx.out(f"out[{odt}]", (M, N), odt)
            ctx.call("mia_splitk_reduce", p(slabs), S, M, N, K.epilogue(out, N, act=L.ACT_RELU, bias=bias, alpha=0.5))
    return run


@case("mx_quantize+mx_quantize_t", "mia_mx_quantize", "mia_mx_quantize_t")
def _mxq(dev):
    x, xt = rnd(dev, (37, 96), BF16, 19, 3.0), rnd(dev, (64, 48), F32, 20, 3.0)

    def run(ctx):
        q, s = ctx.out("q", (37, 96), U8), ctx.out("scales", (37, 3), U8)
        ctx.call("mia_mx_quantize", p(x), L.BF16, 37, 96, 96, p(q), 96, p(s))
        qt, st = ctx.out("q_t", (48, 64), U8), ctx.out("scales_t", (48, 2), U8)
        ctx.call("mia_mx_quantize_t", p(xt), L.F32, 64, 48, 48, p(qt), 64, p(st))
    return run


# ================================================================================================ BN / pool / colsum
def _bn_case(dev, C, P, dt):
    x, dact = rnd(dev, (P, C), dt, 21), rnd(dev, (P, C), dt, 22)
    gamma, beta = uni(dev, C, 0.5, 1.5, 23), rnd(dev, C, F32, 24, 0.1)
    mean, invstd, scale, shift = bn_state(x, gamma, beta)
    dgamma, dbeta = rnd(dev, C, F32, 25), rnd(dev, C, F32, 26)
    rm0, rv0 = rnd(dev, C, F32, 27), uni(dev, C, 0.5, 1.5, 28)

    def run(ctx):
        nb = ctx.lib.mia_bn_partial_bytes(P, C)
        o = {k: ctx.out(f"fwd_stats.{k}", C, F32) for k in ("running_mean", "running_var", "mean", "invstd", "scale", "shift")}
        o["running_mean"].copy_(rm0), o["running_var"].copy_(rv0)
        ctx.call("mia_bn_fwd_stats", p(x), code(dt), P, C, p(gamma), p(beta), p(o["running_mean"]), p(o["running_var"]),
                 0.1, 1e-5, 1, p(o["mean"]), p(o["invstd"]), p(o["scale"]), p(o["shift"]), p(ctx.ws("fwd_stats.partial", nb)))
        dz = ctx.out("reduce.dz", (P, C), dt)
        dg, db = ctx.out("reduce.dgamma", C, F32), ctx.out("reduce.dbeta", C, F32)
        ctx.call("mia_bn_relu_bwd_reduce", p(dact), p(dz), p(x), code(dt), P, C, p(scale), p(shift), p(mean), p(invstd),
                 p(dg), p(db), p(ctx.ws("reduce.partial", nb)))
        dx, dbias = ctx.out("apply.dx", (P, C), dt), ctx.out("apply.dbias", C, F32)
        ctx.call("mia_bn_bwd_apply", p(dact), p(x), p(dx), code(dt), P, C, p(gamma), p(mean), p(invstd), p(dgamma),
                 p(dbeta), p(dbias), p(ctx.ws("apply.partial", nb)))
        dx2, dbias2 = ctx.out("relu_apply.dx", (P, C), dt), ctx.out("relu_apply.dbias", C, F32)
        ctx.call("mia_bn_relu_bwd_apply", p(dact), p(x), p(dx2), code(dt), P, C, p(gamma), p(scale), p(shift), p(mean),
                 p(invstd), p(dgamma), p(dbeta), p(dbias2), p(ctx.ws("relu_apply.partial", nb)))
    return run


for _C, _P, _dt in [(32, 5000, F32), (32, 5000, BF16), (256, 5000, BF16), (256, 70_000, BF16)]:
    case(f"bn[C{_C}-P{_P}-{_dt}]", "mia_bn_fwd_stats", "mia_bn_relu_bwd_reduce", "mia_bn_bwd_apply",
         "mia_bn_relu_bwd_apply")(functools.partial(_bn_case, C=_C, P=_P, dt=_dt))


def _pool_case(dev, n, h, w, c, kh, kw_, dt):
    oh, ow = h // kh, w // kw_
    cells, P = n * oh * ow, n * h * w
    x = rnd(dev, (n, h, w, c), dt, 31)
    gamma, beta = uni(dev, c, 0.5, 1.5, 32), rnd(dev, c, F32, 33, 0.1)
    gamma[1] = -gamma[1]  # a channel whose winner is the raw minimum
    mean, invstd, scale, shift = bn_state(x.view(P, c), gamma, beta)
    g = torch.Generator(device=dev).manual_seed(34)
    argmax = torch.randint(0, kh * kw_, (cells, c), generator=g, device=dev).to(U8)
    win = rnd(dev, (cells, c), dt, 35)
    dout = rnd(dev, (cells, c), dt, 36)
    gm_in = rnd(dev, (cells, c), F32, 37)
    dgamma, dbeta = rnd(dev, c, F32, 38), rnd(dev, c, F32, 39)

    def run(ctx):
        nb = ctx.lib.mia_bn_partial_bytes(P, c)
        for layout in (0, 1, 2):
            if layout == 1 and oh != 1:
                continue
            o, am = ctx.out(f"fwd{layout}.out", (cells, c), dt), ctx.out(f"fwd{layout}.argmax", (cells, c), U8)
            wn = ctx.out(f"fwd{layout}.win", (cells, c), dt)
            ctx.call("mia_pool_fwd", p(x), code(dt), n, h, w, c, kh, kw_, p(scale), p(shift), p(o), layout, p(am), p(wn))
        if dt == BF16 and h % kh == 0:
            for nblk in (16, 2048):
                wn, am = ctx.out(f"raw{nblk}.win", (cells, c), BF16), ctx.out(f"raw{nblk}.argmax", (cells, c), U8)
                part = ctx.out(f"raw{nblk}.partial", (nblk, c, 2), F32, compare=False)
                ctx.call("mia_pool_raw_stats", p(x), n, h, w, c, kh, kw_, p(gamma), p(beta), p(wn), p(am), p(part), nblk)
                st = [ctx.out(f"raw{nblk}.{k}", c, F32) for k in ("mean", "invstd", "scale", "shift")]
                ctx.call("mia_bn_finalize_shifted", p(part), nblk, P, c, p(beta), p(gamma), p(beta), None, None, 0.1, 1e-5,
                         1, *[p(t) for t in st])
            for layout in (0, 1, 2):
                if layout == 1 and oh != 1:
                    continue
                o = ctx.out(f"pool_apply{layout}.out", (cells, c), BF16)
                ctx.call("mia_pool_apply", p(win), n, oh, ow, c, p(scale), p(shift), p(o), L.BF16, layout)
        dz = ctx.out("bwd_reduce.dz", (n, h, w, c), dt)
        dg, db = ctx.out("bwd_reduce.dgamma", c, F32), ctx.out("bwd_reduce.dbeta", c, F32)
        ctx.call("mia_pool_bwd_bn_relu_reduce", p(dout), 0, p(argmax), p(x), code(dt), n, h, w, c, kh, kw_, p(scale),
                 p(shift), p(mean), p(invstd), p(dz), p(dg), p(db), p(ctx.ws("bwd_reduce.partial", nb)))
        for tag, wptr in (("gather", None), ("gather_win", p(win))):
            gm = ctx.out(f"{tag}.gm", (cells, c), F32)
            dg, db = ctx.out(f"{tag}.dgamma", c, F32), ctx.out(f"{tag}.dbeta", c, F32)
            ctx.call("mia_pool_bwd_gather", p(dout), 0, p(argmax), p(x), wptr, code(dt), n, h, w, c, kh, kw_, p(scale),
                     p(shift), p(mean), p(invstd), p(gm), p(dg), p(db), p(ctx.ws(f"{tag}.partial", nb)))
        dx, dbias = ctx.out("apply.dx", (n, h, w, c), dt), ctx.out("apply.dbias", c, F32)
        ctx.call("mia_pool_bn_relu_bwd_apply", p(gm_in), p(argmax), p(x), code(dt), n, h, w, c, kh, kw_, p(gamma), p(mean),
                 p(invstd), p(dgamma), p(dbeta), p(dx), p(dbias), p(ctx.ws("apply.partial", nb)))
    return run


for _geo, _dt in [((2, 1, 200, 64, 1, 64), BF16), ((3, 11, 68, 32, 5, 3), BF16), ((2, 10, 35, 32, 5, 3), F32),
                  ((2, 10, 35, 32, 5, 3), BF16)]:
    case(f"pool[{_geo}-{_dt}]", "mia_pool_fwd", "mia_pool_raw_stats", "mia_pool_apply", "mia_bn_finalize_shifted",
         "mia_pool_bwd_bn_relu_reduce", "mia_pool_bwd_gather",
         "mia_pool_bn_relu_bwd_apply")(functools.partial(lambda dev, g, d: _pool_case(dev, *g, d), g=_geo, d=_dt))


def _colsum_case(dev, P, C, ld, dt):
    x = rnd(dev, (P, ld), dt, 41)

    def run(ctx):
        out = ctx.out("out", C, F32)
        part = ctx.ws("partial", 1024 * C * 4)  # MIA_COLSUM_MAXBLK * C floats
        ctx.call("mia_colsum", p(x), code(dt), P, C, ld, p(out), p(part))
    return run


for _C in (50, 768, 4096):
    for _P in (7, 5000, 70_000):
        _dt = BF16 if _C == 4096 else F32
        case(f"colsum[P{_P}-C{_C}]", "mia_colsum")(functools.partial(_colsum_case, P=_P, C=_C, ld=_C, dt=_dt))
case("colsum[P5000-C50-ld72]", "mia_colsum")(functools.partial(_colsum_case, P=5000, C=50, ld=72, dt=BF16))


# ================================================================================================ EnvNet convs
def _packed(dev, shape, mode, seed, dtype=L.BF16):
    return K.pack_weight(rnd(dev, shape, F32, seed, 0.1).contiguous(), dtype, mode)


def _fe_conv1_fwd(dev, nwaves):
    n, t = 2, 9000
    w1 = (t - 64) // 2 + 1
    x, w, bias = rnd(dev, (n, t), F32, 51), _packed(dev, (32, 1, 1, 64), 0, 52), rnd(dev, 32, F32, 53)

    def run(ctx):
        y1 = ctx.out("y1", (n * w1, 32), BF16)
        part = ctx.out("partial", (nwaves, 32, 2), F32)
        ctx.call("mia_fe_conv1_fwd", p(x), p(w), p(bias), p(y1), p(part), nwaves, n, t)
        y1b = ctx.out("y1(no partial)", (n * w1, 32), BF16)
        ctx.call("mia_fe_conv1_fwd", p(x), p(w), p(bias), p(y1b), None, nwaves, n, t)
    return run


def _fe_conv3_fwd(dev, nwaves):
    n, h, wd = 5, 12, 100
    x, w, bias = rnd(dev, (n, h, wd), BF16, 54), _packed(dev, (32, 1, 8, 8), 0, 55), rnd(dev, 32, F32, 56)

    def run(ctx):
        y = ctx.out("y", (n * (h - 7) * (wd - 7), 32), BF16)
        part = ctx.out("partial", (nwaves, 32, 2), F32)
        ctx.call("mia_fe_conv3_fwd", p(x), p(w), p(bias), p(y), p(part), nwaves, n, h, wd)
    return run


for _nw in (4, 4096):
    case(f"fe_conv1_fwd[nwaves{_nw}]", "mia_fe_conv1_fwd")(functools.partial(_fe_conv1_fwd, nwaves=_nw))
    case(f"fe_conv3_fwd[nwaves{_nw}]", "mia_fe_conv3_fwd")(functools.partial(_fe_conv3_fwd, nwaves=_nw))


def _trunk_conv8(dev, nblocks):
    n, h, wd = 3, 10, 40
    x, w, bias = rnd(dev, (n, h, wd, 32), BF16, 57), _packed(dev, (32, 32, 8, 8), 0, 58), rnd(dev, 32, F32, 59)
    sc, sh = uni(dev, 32, 0.5, 1.5, 60), rnd(dev, 32, F32, 61, 0.1)
    dy, wf = rnd(dev, (n, 3, 30, 32), BF16, 62), _packed(dev, (32, 32, 8, 8), 1, 63)

    def run(ctx):
        y = ctx.out("fwd.y", (n * (h - 7) * (wd - 7), 32), BF16)
        part = ctx.out("fwd.partial", (4 * nblocks, 32, 2), F32)
        ctx.call("mia_trunk_conv8", p(x), p(sc), p(sh), p(w), p(bias), p(y), p(part), nblocks, n, h, wd, 0, 0)
        dx = ctx.out("dgrad.dx", (n * 10 * 37, 32), BF16)
        ctx.call("mia_trunk_conv8", p(dy), None, None, p(wf), None, p(dx), None, nblocks, n, 3, 30, 7, 7)
    return run


def _trunk_conv8_dgrad_bn(dev, nblocks):
    n, h, wd = 3, 3, 30
    dy, wf = rnd(dev, (n, h, wd, 32), BF16, 64), _packed(dev, (32, 32, 8, 8), 1, 65)
    bx = rnd(dev, (n * (h + 7) * (wd + 7), 32), BF16, 66)
    gamma, beta = uni(dev, 32, 0.5, 1.5, 67), rnd(dev, 32, F32, 68, 0.1)
    mean, invstd, scale, shift = bn_state(bx, gamma, beta)

    def run(ctx):
        dx = ctx.out("dx", (n * (h + 7) * (wd + 7), 32), BF16)
        dg, db = ctx.out("dgamma", 32, F32), ctx.out("dbeta", 32, F32)
        part = ctx.ws("partial", 4 * nblocks * 32 * 2 * 4)  # f32 [4*nblocks][32][2]
        ctx.call("mia_trunk_conv8_dgrad_bn", p(dy), p(wf), p(dx), nblocks, n, h, wd, p(bx), p(scale), p(shift), p(mean),
                 p(invstd), p(dg), p(db), p(part))
    return run


for _nb in (1, 256):
    case(f"trunk_conv8[nblocks{_nb}]", "mia_trunk_conv8")(functools.partial(_trunk_conv8, nblocks=_nb))
    case(f"trunk_conv8_dgrad_bn[nblocks{_nb}]", "mia_trunk_conv8_dgrad_bn")(functools.partial(_trunk_conv8_dgrad_bn, nblocks=_nb))


def _conv3_wgrad(dev, nwaves):
    n, h, wd = 3, 9, 40
    cells = n * (h - 7) * (wd - 7)
    x, dy, ya = rnd(dev, (n, h, wd), BF16, 69), rnd(dev, (cells, 32), BF16, 70), rnd(dev, (cells, 32), BF16, 71)
    gamma, beta = uni(dev, 32, 0.5, 1.5, 72), rnd(dev, 32, F32, 73, 0.1)
    mean, invstd, scale, shift = bn_state(ya, gamma, beta)
    dgamma, dbeta = rnd(dev, 32, F32, 74), rnd(dev, 32, F32, 75)

    def run(ctx):
        dw = ctx.out("wgrad.dw", (32, 64), F32)
        part = ctx.ws("wgrad.part", (nwaves * 2048 + 64 * 4096) * 4, align=8)  # the header's prose
        ctx.call("mia_conv3_wgrad", p(x), p(dy), p(dw), p(part), nwaves, n, h, wd)
        dw2, dbias = ctx.out("wgrad_bn.dw", (32, 64), F32), ctx.out("wgrad_bn.dbias", 32, F32)
        dyo = ctx.out("wgrad_bn.dy", (cells, 32), BF16)
        part2 = ctx.ws("wgrad_bn.part", ctx.lib.mia_conv3_wgrad_workspace_bytes(nwaves), align=8)
        ctx.call("mia_conv3_wgrad_bn", p(x), p(dy), p(ya), p(dyo), p(dw2), p(dbias), p(part2), nwaves, n, h, wd, p(gamma),
                 p(scale), p(shift), p(mean), p(invstd), p(dgamma), p(dbeta))
    return run


for _nw in (4, 1024):
    case(f"conv3_wgrad[nwaves{_nw}]", "mia_conv3_wgrad", "mia_conv3_wgrad_bn")(functools.partial(_conv3_wgrad, nwaves=_nw))


def _fe_conv1_wgrad_bn(dev, n, split):
    t = 9000
    w1 = (t - 64) // 2 + 1
    x, dact, y1 = rnd(dev, (n, t), F32, 76), rnd(dev, (n * w1, 32), BF16, 77), rnd(dev, (n * w1, 32), BF16, 78)
    gamma, beta = uni(dev, 32, 0.5, 1.5, 79), rnd(dev, 32, F32, 80, 0.1)
    mean, invstd, scale, shift = bn_state(y1, gamma, beta)

    def run(ctx):
        o = {k: ctx.out(k, s, F32) for k, s in (("dgamma", 32), ("dbeta", 32), ("dw", (32, 64)), ("dbias", 32))}
        ws = ctx.ws("workspace", (split * (2 * 2048 + 96) + 2 * 2048 + n * 80 + 2 * 160 + 4) * 4)  # the header's prose
        ctx.call("mia_fe_conv1_wgrad_bn", p(x), p(dact), p(y1), n, t, p(scale), p(shift), p(gamma), p(mean), p(invstd),
                 p(o["dgamma"]), p(o["dbeta"]), p(o["dw"]), p(o["dbias"]), p(ws), split)
    return run


for _n in (2, 5):
    for _split in (2, 512):
        case(f"fe_conv1_wgrad_bn[n{_n}-split{_split}]",
             "mia_fe_conv1_wgrad_bn")(functools.partial(_fe_conv1_wgrad_bn, n=_n, split=_split))


def _fe_conv2_slabs(dev, n, w2):
    """One 128 KB f32 slab per workgroup: one workgroup per 128-pixel item, at most one per CU."""
    return min(n * -(-w2 // 128), torch.cuda.get_device_properties(dev).multi_processor_count)


def _fe_conv2(dev, n, w1, pre):
    w2 = (w1 - 16) // 2 + 1
    y1, dy2 = rnd(dev, (n * w1, 32), BF16, 81), rnd(dev, (n * w2, 64), BF16, 82)
    w, wpar, bias = _packed(dev, (64, 32, 1, 16), 0, 83), _packed(dev, (64, 32, 1, 16), 2, 83), rnd(dev, 64, F32, 84)
    sc, sh = (uni(dev, 32, 0.5, 1.5, 85), rnd(dev, 32, F32, 86, 0.1)) if pre else (None, None)

    def run(ctx):
        y2 = ctx.out("fwd.y2", (n * w2, 64), BF16)
        ctx.call("mia_fe_conv2_fwd", p(y1), p(sc), p(sh), p(w), p(bias), p(y2), n, w1, w2)
        da1 = ctx.out("dgrad.da1", (n * w1, 32), BF16)
        ctx.call("mia_fe_conv2_dgrad", p(dy2), p(wpar), p(da1), n, w1, w2)
        dw = ctx.out("wgrad.dw", (64, 512), F32)
        nbytes = _fe_conv2_slabs(dev, n, w2) * 64 * 512 * 4
        ws = ctx.ws("wgrad.workspace", nbytes)
        ctx.call("mia_fe_conv2_wgrad", p(dy2), p(y1), p(sc), p(sh), p(dw), n, w1, w2, p(ws), nbytes)
    return run


for _n, _w1, _pre in [(1, 300, False), (3, 4112, True), (20, 4112, True)]:
    case(f"fe_conv2[n{_n}-w{_w1}]", "mia_fe_conv2_fwd", "mia_fe_conv2_dgrad",
         "mia_fe_conv2_wgrad")(functools.partial(_fe_conv2, n=_n, w1=_w1, pre=_pre))


@pytest.mark.gpu
def test_fe_conv2_wgrad_a_slab_short_is_rejected_by_the_host(cuda):
    """The only undersized call of this file: the host validates ws_bytes before any launch, returns a negative
    code and leaves workspace and dw untouched."""
    n, w1 = 3, 4112
    w2 = (w1 - 16) // 2 + 1
    y1, dy2 = rnd(cuda, (n * w1, 32), BF16, 81), rnd(cuda, (n * w2, 64), BF16, 82)
    slab = 64 * 512 * 4
    short = (_fe_conv2_slabs(cuda, n, w2) - 1) * slab
    a = GuardedArena(cuda, 0xFF)
    ws, dw = a.take("workspace", short), a.f32("dw", (64, 512))
    lib = L.load()
    rc = lib.mia_fe_conv2_wgrad(p(dy2), p(y1), None, None, p(dw), n, w1, w2, p(ws), short, L.stream_ptr())
    torch.cuda.synchronize()
    assert rc < 0 and b"workspace too small" in lib.mia_last_error_string()
    a.check()
    assert bool((ws == 0xFF).all()) and bool((_bytes(dw) == 0xFF).all())


@case("envnet_small_kernels", "mia_conv1ch_dgrad", "mia_col2im_rows", "mia_pad_w2", "mia_shift_pad_w2",
      "mia_drop_last_col", "mia_bn_relu_apply")
def _envnet_small(dev):
    n, oh, ow = 3, 10, 121
    dy, w = rnd(dev, (n * oh * ow, 32), BF16, 87), rnd(dev, (32, 1, 8, 8), F32, 88)
    pc = rnd(dev, (2, 5, 37, 8), F32, 89)
    rows, W, c = 12, 37, 128
    dyw, src = rnd(dev, (rows, W - 1, c), BF16, 90), rnd(dev, (rows, W, c), BF16, 91)
    xa, sc, sh = rnd(dev, (999, 64), BF16, 92), uni(dev, 64, 0.5, 1.5, 93), rnd(dev, 64, F32, 94, 0.1)

    def run(ctx):
        dx = ctx.out("conv1ch_dgrad.dx", (n, oh + 7, ow + 7), BF16)
        ctx.call("mia_conv1ch_dgrad", p(dy), p(w), p(dx), n, oh, ow)
        for dt in (F32, BF16):
            o = ctx.out(f"col2im_rows.out[{dt}]", (2, 12, 37), dt)
            ctx.call("mia_col2im_rows", p(pc), 2, 5, 37, 8, p(o), code(dt))
        dst, zp = ctx.out("pad_w2.dst", (1 + rows * W, c), BF16), ctx.out("pad_w2.zero_pixel", 64, BF16)
        ctx.call("mia_pad_w2", p(dyw), rows, W, c, p(dst), p(zp), 64)
        ash = ctx.out("shift_pad_w2.out", (rows, W, 2 * c), BF16)
        ctx.call("mia_shift_pad_w2", p(dyw), rows, W, c, p(ash))
        dl = ctx.out("drop_last_col.dst", (rows, W - 1, c), BF16)
        ctx.call("mia_drop_last_col", p(src), rows, W, c, p(dl))
        o = ctx.out("bn_relu_apply.out", (999, 64), BF16)
        ctx.call("mia_bn_relu_apply", p(xa), 999, 64, p(sc), p(sh), p(o))
    return run


@case("pack_weight(s)", "mia_pack_weight", "mia_pack_weights")
def _pack(dev):
    W = {0: rnd(dev, (64, 32, 1, 16), F32, 95), 1: rnd(dev, (32, 32, 8, 8), F32, 96), 2: rnd(dev, (64, 32, 1, 16), F32, 97),
         3: rnd(dev, (32, 1, 8, 8), F32, 98), 4: rnd(dev, (33, 3, 5, 7), F32, 99)}

    def run(ctx):
        for mode, src in W.items():
            cout, cin, kh, kw_ = src.shape
            for dt in ((F32,) if mode == 4 else (BF16, F32)):
                o = ctx.out(f"pack_weight.m{mode}[{dt}]", src.numel(), dt)
                ctx.call("mia_pack_weight", p(src), p(o), code(dt), cout, cin, kh, kw_, mode)
        jobs = [(W[m], dt, m) for m in (0, 1, 2, 3) for dt in (BF16, F32)] + [(W[4], BF16, 0)]
        arr = (L.MiaPackJob * len(jobs))()
        for k, (src, dt, mode) in enumerate(jobs):
            o = ctx.out(f"pack_weights.job{k}", src.numel(), dt)
            arr[k] = L.MiaPackJob(p(src), p(o), code(dt), *src.shape, mode)
        ctx.call("mia_pack_weights", arr, len(jobs))
    return run


# ================================================================================================ LayerNorm
def _ln_case(dev, rows, D):
    x, dy = rnd(dev, (rows, D), F32, 101), rnd(dev, (rows, D), BF16, 102)
    xb = x.to(BF16)
    gamma, beta = uni(dev, D, 0.5, 1.5, 103), rnd(dev, D, F32, 104, 0.1)
    mean = x.mean(1).contiguous()
    rstd = (x.var(1, unbiased=False) + 1e-6).rsqrt().contiguous()
    dx0 = rnd(dev, (rows, D), F32, 105)

    def run(ctx):
        lib = ctx.lib
        for tag, xin, ydt in (("f32->bf16", x, BF16), ("bf16->bf16", xb, BF16), ("f32->f32", x, F32)):
            y = ctx.out(f"fwd[{tag}].y", (rows, D), ydt)
            mu, rs = ctx.out(f"fwd[{tag}].mean", rows, F32), ctx.out(f"fwd[{tag}].rstd", rows, F32)
            ctx.call("mia_layernorm_fwd", p(xin), code(xin.dtype), p(gamma), p(beta), p(y), code(ydt), p(mu), p(rs), rows, D, 1e-6)
        if D % 64 == 0 and D <= 768:
            y, q, s = ctx.out("fwd_mx.y", (rows, D), BF16), ctx.out("fwd_mx.q", (rows, D), U8), ctx.out("fwd_mx.scales", (rows, D // 32), U8)
            mu, rs = ctx.out("fwd_mx.mean", rows, F32), ctx.out("fwd_mx.rstd", rows, F32)
            ctx.call("mia_layernorm_fwd_mx", p(x), L.F32, p(gamma), p(beta), p(y), p(q), p(s), p(mu), p(rs), rows, D, 1e-6)
        nb = lib.mia_layernorm_partial_bytes(rows, D)
        for acc in (0, 1):
            dx = ctx.out(f"bwd[acc{acc}].dx", (rows, D), F32)
            dx.copy_(dx0)
            dg, db = ctx.out(f"bwd[acc{acc}].dgamma", D, F32), ctx.out(f"bwd[acc{acc}].dbeta", D, F32)
            dx2 = ctx.out(f"bwd[acc{acc}].dx2", (rows, D), BF16) if D == 768 else None
            ctx.call("mia_layernorm_bwd", p(dy), L.BF16, p(x), L.F32, p(gamma), p(mean), p(rstd), p(dx), L.F32, acc, p(dx2),
                     L.BF16, p(dg), p(db), p(ctx.ws(f"bwd[acc{acc}].partial", nb)), rows, D)
        dxb = ctx.out("bwd[bf16].dx", (rows, D), BF16)
        dg, db = ctx.out("bwd[bf16].dgamma", D, F32), ctx.out("bwd[bf16].dbeta", D, F32)
        ctx.call("mia_layernorm_bwd", p(dy), L.BF16, p(xb), L.BF16, p(gamma), p(mean), p(rstd), p(dxb), L.BF16, 0, None, 0,
                 p(dg), p(db), p(ctx.ws("bwd[bf16].partial", nb)), rows, D)
        if D == 768:
            o = {k: ctx.out(f"bwd_colsum.{k}", s, dt) for k, s, dt in (("dx", (rows, D), F32), ("dx2", (rows, D), BF16),
                                                                       ("dgamma", D, F32), ("dbeta", D, F32), ("colsum", D, F32))}
            ctx.call("mia_layernorm_bwd_colsum", p(dy), L.BF16, p(x), L.F32, p(gamma), p(mean), p(rstd), p(o["dx"]), L.F32, 0,
                     p(o["dx2"]), L.BF16, p(o["dgamma"]), p(o["dbeta"]), p(o["colsum"]), p(ctx.ws("bwd_colsum.partial", nb)),
                     rows, D)
            o = {k: ctx.out(f"bwd_colsum_mx.{k}", s, dt) for k, s, dt in (
                ("dx", (rows, D), F32), ("dx2", (rows, D), BF16), ("dgamma", D, F32), ("dbeta", D, F32), ("colsum", D, F32),
                ("q", (rows, D), U8), ("scales", (rows, D // 32), U8))}
            ctx.call("mia_layernorm_bwd_colsum_mx", p(dy), L.BF16, p(x), L.F32, p(gamma), p(mean), p(rstd), p(o["dx"]), L.F32,
                     0, p(o["dx2"]), p(o["dgamma"]), p(o["dbeta"]), p(o["colsum"]), p(o["q"]), p(o["scales"]),
                     p(ctx.ws("bwd_colsum_mx.partial", nb)), rows, D)
    return run


for _rows in (5, 300, 4113):
    for _D in (768, 384, 1000):
        case(f"layernorm[rows{_rows}-D{_D}]", "mia_layernorm_fwd", "mia_layernorm_fwd_mx", "mia_layernorm_bwd",
             "mia_layernorm_bwd_colsum", "mia_layernorm_bwd_colsum_mx")(functools.partial(_ln_case, rows=_rows, D=_D))


# ================================================================================================ attention
def _attn_inputs(dev, B, N, H, dt):
    qkv = rnd(dev, (B, N, 3 * H * 64), dt, 111, 1.5)
    dout = rnd(dev, (B, N, H * 64), dt, 112)
    lib = L.load()
    out, lse = torch.empty(B, N, H * 64, dtype=dt, device=dev), torch.empty(B, H, N, device=dev)
    L.check(lib.mia_attn_fwd(p(qkv), p(out), p(lse), code(dt), B, N, H, 0.125, L.stream_ptr()), "mia_attn_fwd")
    return qkv, dout, out, lse


def _attn_case(dev, B, N, H, dt):
    qkv, dout, out0, lse0 = _attn_inputs(dev, B, N, H, dt)
    cd = code(dt)

    def run(ctx):
        lib = ctx.lib
        out, lse = ctx.out("fwd.out", (B, N, H * 64), dt), ctx.out("fwd.lse", (B, H, N), F32)
        ctx.call("mia_attn_fwd", p(qkv), p(out), p(lse), cd, B, N, H, 0.125)
        dq = ctx.out("bwd.dqkv", (B, N, 3 * H * 64), dt)
        work = ctx.ws("bwd.work", lib.mia_attn_bwd_workspace_bytes(cd, B, N, H), align=256)
        ctx.call("mia_attn_bwd", p(qkv), p(out0), p(dout), p(lse0), p(dq), p(work), cd, B, N, H, 0.125)
        # dropout on the probabilities, p = 0.1
        od, ld = ctx.out("fwd_dropout.out", (B, N, H * 64), dt), ctx.out("fwd_dropout.lse", (B, H, N), F32)
        wd = ctx.ws("dropout.work", lib.mia_attn_saved_q_bytes(B, N, H) if dt == BF16 else
                    lib.mia_attn_bwd_workspace_bytes(cd, B, N, H), align=256)
        ctx.call("mia_attn_fwd_dropout", p(qkv), p(od), p(ld), p(wd) if dt == BF16 else None, cd, B, N, H, 0.125, 0.1, 1234)
        dqd = ctx.out("bwd_dropout.dqkv", (B, N, 3 * H * 64), dt)
        ctx.call("mia_attn_bwd_dropout", p(qkv), p(od), p(dout), p(ld), p(dqd), p(wd), cd, B, N, H, 0.125, 0.1, 1234,
                 int(dt == BF16))
        if dt == F32:
            return
        dq0 = ctx.out("bwd_dropout[q_ready0].dqkv", (B, N, 3 * H * 64), dt)
        w0 = ctx.ws("bwd_dropout[q_ready0].work", lib.mia_attn_bwd_workspace_bytes(cd, B, N, H), align=256)
        ctx.call("mia_attn_bwd_dropout", p(qkv), p(od), p(dout), p(ld), p(dq0), p(w0), cd, B, N, H, 0.125, 0.1, 1234, 0)
        # the fp8-mixed forward and the training forms that keep Q' from the forward
        o, l = ctx.out("fwd_mx.out", (B, N, H * 64), BF16), ctx.out("fwd_mx.lse", (B, H, N), F32)
        q8, s8 = ctx.out("fwd_mx.q8", (B * N, H * 64), U8), ctx.out("fwd_mx.s8", (B * N, H * 2), U8)
        ctx.call("mia_attn_fwd_mx", p(qkv), p(o), p(l), p(q8), p(s8), B, N, H, 0.125)
        for tag, mx in (("save_q", False), ("save_q_mx", True)):
            o, l = ctx.out(f"{tag}.out", (B, N, H * 64), BF16), ctx.out(f"{tag}.lse", (B, H, N), F32)
            q8 = ctx.out(f"{tag}.q8", (B * N, H * 64), U8) if mx else None
            s8 = ctx.out(f"{tag}.s8", (B * N, H * 2), U8) if mx else None
            saved = ctx.ws(f"{tag}.saved", lib.mia_attn_saved_q_bytes(B, N, H), align=256)
            ctx.call("mia_attn_fwd_save_q", p(qkv), p(o), p(l), p(q8), p(s8), p(saved), B, N, H, 0.125)
        dq = ctx.out("bwd_saved_q.dqkv", (B, N, 3 * H * 64), BF16)
        ctx.call("mia_attn_bwd_saved_q", p(qkv), p(out0), p(dout), p(lse0), p(dq), p(saved), B, N, H, 0.125)
        for q_ready in (0, 1):
            chain = ctx.ws(f"onepass[q_ready{q_ready}].chain", lib.mia_attn_bwd_chain_bytes(B, N, H), align=256)
            sv = saved if q_ready else ctx.ws("onepass[q_ready0].saved", lib.mia_attn_saved_q_bytes(B, N, H), align=256)
            err = ctx.out(f"onepass[q_ready{q_ready}].err", 1, I32)
            err.zero_()  # the header: zero before the first call
            dq = ctx.out(f"onepass[q_ready{q_ready}].dqkv", (B, N, 3 * H * 64), BF16)
            ctx.call("mia_attn_bwd_onepass", p(qkv), p(out0), p(dout), p(lse0), p(dq), p(sv), p(chain), p(err), B, N, H, 0.125,
                     q_ready)
        nws = lib.mia_attn_bwd_workspace_bytes(L.BF16, B, N, H)
        off = int(lib.mia_attn_bwd_error_offset(B, N, H))
        for fn in ("mia_attn_bwd_two_pass", "mia_attn_bwd_fused"):
            for q_ready in (0, 1):
                tag = f"{fn[13:]}[q_ready{q_ready}]"
                work = ctx.ws(f"{tag}.work", nws, align=256)
                if q_ready:
                    o, l = ctx.out(f"{tag}.fwd.out", (B, N, H * 64), BF16), ctx.out(f"{tag}.fwd.lse", (B, H, N), F32)
                    ctx.call("mia_attn_fwd_save_q", p(qkv), p(o), p(l), None, None, p(work), B, N, H, 0.125)
                dq = ctx.out(f"{tag}.dqkv", (B, N, 3 * H * 64), BF16)
                ctx.call(fn, p(qkv), p(out0), p(dout), p(lse0), p(dq), p(work), B, N, H, 0.125, q_ready)
                if fn.endswith("fused"):
                    ctx.outs[f"{tag}.error_word"] = work[off:off + 4]
    return run


for _B, _N, _H in [(1, 77, 2), (3, 37, 2), (1, 257, 3), (2, 300, 2)]:
    case(f"attention[{_B}-{_N}-{_H}-bf16]", "mia_attn_fwd", "mia_attn_bwd", "mia_attn_fwd_dropout", "mia_attn_bwd_dropout",
         "mia_attn_fwd_mx", "mia_attn_fwd_save_q", "mia_attn_bwd_saved_q", "mia_attn_bwd_onepass", "mia_attn_bwd_two_pass",
         "mia_attn_bwd_fused")(functools.partial(_attn_case, B=_B, N=_N, H=_H, dt=BF16))
    case(f"attention[{_B}-{_N}-{_H}-f32]", "mia_attn_fwd", "mia_attn_bwd", "mia_attn_fwd_dropout",
         "mia_attn_bwd_dropout")(functools.partial(_attn_case, B=_B, N=_N, H=_H, dt=F32))


# ================================================================================================ LEAF
def _leaf_case(dev, B, F, Kt, pool, T):
    x, w = rnd(dev, (B, T), F32, 121), rnd(dev, (2, F, Kt), F32, 122, 0.1)
    Tp = T // pool
    gP = rnd(dev, (B, F, Tp), F32, 123)

    def run(ctx):
        lib = ctx.lib
        for cd, tag in ((L.BF16, "bf16"), (L.F32, "f32")):
            P = ctx.out(f"fwd[{tag}].P", (B, F, Tp), F32)
            ws = ctx.ws(f"fwd[{tag}].workspace", lib.mia_leaf_workspace_bytes(B, T, F, Kt, pool, 0)) if cd == L.BF16 else None
            ctx.call("mia_leaf_energy_fwd", p(x), p(w), p(P), B, T, F, Kt, pool, cd, p(ws))
            dw = ctx.out(f"bwd[{tag}].dw", (2, F, Kt), F32)
            ws = ctx.ws(f"bwd[{tag}].workspace", lib.mia_leaf_workspace_bytes(B, T, F, Kt, pool, 1))
            ctx.call("mia_leaf_energy_bwd", p(x), p(w), p(gP), p(dw), B, T, F, Kt, pool, cd, p(ws))
    return run


for _edge, _geo in {"one_frame": (2, 5, 65, 160, 160), "short_of_a_frame": (2, 5, 65, 160, 160 * 3 - 1),
                    "wg_tile_plus_one_frame": (1, 5, 65, 160, 160 * 17), "three_taps": (2, 5, 3, 160, 160 * 2 + 7),
                    "pool_32": (2, 5, 65, 32, 32 * 81 + 5), "filters_33": (1, 33, 33, 160, 160 * 2),
                    "filters_65": (1, 65, 33, 160, 160 * 2), "taps_447": (1, 3, 447, 160, 160 * 9 + 3),
                    "taps_449": (1, 3, 449, 160, 160 * 2)}.items():
    case(f"leaf_energy[{_edge}]", "mia_leaf_energy_fwd",
         "mia_leaf_energy_bwd")(functools.partial(lambda dev, g: _leaf_case(dev, *g), g=_geo))


def _pcen_case(dev, B, F, Tp):
    P = uni(dev, (B, F, Tp), 0.01, 2.0, 124)
    r, delta = uni(dev, F, 0.2, 0.9, 125), uni(dev, F, 0.5, 2.5, 126)
    gy = rnd(dev, (B, F, Tp), F32, 127)
    Fp, halo = (F + 7) // 8 * 8, 2

    def run(ctx):
        lib = ctx.lib
        y = ctx.out("pcen_fwd.y", (B, F, Tp), F32)
        ctx.call("mia_pcen_fwd", p(P), p(r), p(delta), 1e-6, p(y), B, F, Tp)
        gP, dr, dd = ctx.out("pcen_bwd.gP", (B, F, Tp), F32), ctx.out("pcen_bwd.dr", F, F32), ctx.out("pcen_bwd.ddelta", F, F32)
        ctx.call("mia_pcen_bwd", p(P), p(r), p(delta), 1e-6, p(gy), p(gP), p(dr), p(dd),
                 p(ctx.ws("pcen_bwd.workspace", lib.mia_pcen_workspace_bytes(B, F))), B, F, Tp)
        for dt in (F32, BF16):
            for h in (0, halo):
                tag = f"[{dt}-halo{h}]"
                yl = ctx.out(f"lt_pcen_fwd{tag}.y", (B, Tp + 2 * h, Fp), dt)
                ctx.call("mia_lt_pcen_fwd", p(P), p(r), p(delta), 1e-6, p(yl), code(dt), B, F, Tp, h)
                gyl = rnd(dev, (B, Tp + 2 * h, Fp), dt, 128)
                gP, dr, dd = (ctx.out(f"lt_pcen_bwd{tag}.gP", (B, F, Tp), F32), ctx.out(f"lt_pcen_bwd{tag}.dr", F, F32),
                              ctx.out(f"lt_pcen_bwd{tag}.ddelta", F, F32))
                ctx.call("mia_lt_pcen_bwd", p(P), p(r), p(delta), 1e-6, p(gyl), code(dt), p(gP), p(dr), p(dd),
                         p(ctx.ws(f"lt_pcen_bwd{tag}.workspace", lib.mia_pcen_workspace_bytes(B, F))), B, F, Tp, h)
    return run


for _s in [(2, 5, 7), (1, 186, 94), (2, 128, 3)]:
    case(f"pcen[{_s}]", "mia_pcen_fwd", "mia_pcen_bwd", "mia_lt_pcen_fwd",
         "mia_lt_pcen_bwd")(functools.partial(lambda dev, s: _pcen_case(dev, *s), s=_s))


def _lt_case(dev, n, t, c, k, dt):
    ot = t // k
    z = rnd(dev, (n, t, c), dt, 131)
    gamma, beta = uni(dev, c, 0.5, 1.5, 132), rnd(dev, c, F32, 133, 0.1)
    gamma[1] = -gamma[1]
    mean, invstd, scale, shift = bn_state(z.view(n * t, c), gamma, beta)
    win, dout, dh = rnd(dev, (n, ot, c), dt, 134), rnd(dev, (n, ot, c), dt, 135), rnd(dev, (n, c), dt, 136)
    g = torch.Generator(device=dev).manual_seed(137)
    argmax = torch.randint(0, k, (n, ot, c), generator=g, device=dev).to(U8)
    gm_in, dgamma, dbeta = rnd(dev, (n, ot, c), F32, 138), rnd(dev, c, F32, 139), rnd(dev, c, F32, 140)

    def run(ctx):
        lib = ctx.lib
        nblk = int(lib.mia_lt_stats_blocks(n, t, c, k))
        assert nblk >= 1
        wn, am = ctx.out("stats.win", (n, ot, c), dt), ctx.out("stats.argmax", (n, ot, c), U8)
        part = ctx.out("stats.partial", (nblk, c, 2), F32, compare=False)
        ctx.call("mia_lt_pool_stats", p(z), code(dt), n, t, c, k, p(gamma), p(beta), p(wn), p(am), p(part), nblk)
        st = [ctx.out(f"stats.{s}", c, F32) for s in ("mean", "invstd", "scale", "shift")]
        ctx.call("mia_bn_finalize_shifted", p(part), nblk, n * t, c, p(beta), p(gamma), p(beta), None, None, 0.1, 1e-5, 1,
                 *[p(s) for s in st])
        wn2, am2 = ctx.out("stats[eval].win", (n, ot, c), dt), ctx.out("stats[eval].argmax", (n, ot, c), U8)
        ctx.call("mia_lt_pool_stats", p(z), code(dt), n, t, c, k, p(gamma), None, p(wn2), p(am2), None, nblk)
        for odt in (F32, BF16):
            o = ctx.out(f"apply[{odt}].out", (n, ot, c), odt)
            ctx.call("mia_lt_pool_apply", p(win), code(dt), n, ot, c, p(scale), p(shift), p(o), code(odt), 0)
            om = ctx.out(f"apply[{odt}-mean].out", (n, c), odt)
            ctx.call("mia_lt_pool_apply", p(win), code(dt), n, ot, c, p(scale), p(shift), p(om), code(odt), 1)
        nws = lib.mia_lt_workspace_bytes(c)
        for tag, d, mm in (("gather", dout, 0), ("gather[mean]", dh, 1)):
            gm, dg, db = ctx.out(f"{tag}.gm", (n, ot, c), F32), ctx.out(f"{tag}.dgamma", c, F32), ctx.out(f"{tag}.dbeta", c, F32)
            ctx.call("mia_lt_pool_bwd_gather", p(d), code(dt), mm, p(win), code(dt), n, ot, c, p(scale), p(shift), p(mean),
                     p(invstd), p(gm), p(dg), p(db), p(ctx.ws(f"{tag}.workspace", nws)))
        dz, dbias = ctx.out("bwd_apply.dz", (n, t, c), dt), ctx.out("bwd_apply.dbias", c, F32)
        ctx.call("mia_lt_pool_bwd_apply", p(gm_in), p(argmax), p(z), code(dt), n, t, c, k, p(gamma), p(mean), p(invstd),
                 p(dgamma), p(dbeta), p(dz), p(dbias), p(ctx.ws("bwd_apply.workspace", nws)))
    return run


for _s in [(2, 9, 8, 4), (1, 4, 384, 4), (3, 11, 256, 2), (2, 37, 1024, 4), (4, 1000, 384, 3)]:
    for _dt in (F32, BF16):
        case(f"leaftrunk[{_s}-{_dt}]", "mia_lt_pool_stats", "mia_lt_pool_apply", "mia_lt_pool_bwd_gather",
             "mia_lt_pool_bwd_apply", "mia_bn_finalize_shifted")(functools.partial(lambda dev, s, d: _lt_case(dev, *s, d), s=_s, d=_dt))


# ================================================================================================ other
def _adam_case(dev, sizes, offset):
    n = len(sizes)
    P0 = [rnd(dev, s, F32, 150 + i) for i, s in enumerate(sizes)]
    G0 = [rnd(dev, s, F32, 160 + i, 3.0) for i, s in enumerate(sizes)]
    M0 = [rnd(dev, s, F32, 170 + i, 0.01) for i, s in enumerate(sizes)]
    V0 = [uni(dev, s, 0.0, 1e-3, 180 + i) for i, s in enumerate(sizes)]
    if offset:  # gradients are inputs: the same 4-byte offset by hand
        G0 = [torch.cat([g.new_zeros(1), g])[1:] for g in G0]

    def run(ctx):
        pp = [ctx.out(f"param{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        mm = [ctx.out(f"exp_avg{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        vv = [ctx.out(f"exp_avg_sq{i}", s, F32, offset=offset) for i, s in enumerate(sizes)]
        sh = [ctx.out(f"shadow{i}", s, BF16, offset=offset // 2) if i == 0 else None for i, s in enumerate(sizes)]
        for dst, src in zip(pp + mm + vv, P0 + M0 + V0):
            dst.copy_(src)
        table = torch.tensor([[t.data_ptr() for t in pp], [t.data_ptr() for t in G0], [t.data_ptr() for t in mm],
                              [t.data_ptr() for t in vv], [0 if t is None else t.data_ptr() for t in sh], list(sizes)],
                             dtype=I64).to(dev)
        tot = ctx.out("total_norm", 1, F32)
        ws = ctx.ws("sqnorm_ws", ctx.lib.mia_adam_workspace_bytes(n))
        ctx.call("mia_clip_adam", p(table[0]), p(table[1]), p(table[2]), p(table[3]), p(table[4]), p(table[5]), n, max(sizes),
                 max(sizes), 1e-3, 0.9, 0.999, 1e-8, 1e-4, 3, 1.0, p(tot), p(ws), None, None, None)
        ctx.keep = (table,)
    return run


case("clip_adam[1-tensor-300001]", "mia_clip_adam")(functools.partial(_adam_case, sizes=(300_001,), offset=0))
case("clip_adam[3-tensors]", "mia_clip_adam")(functools.partial(_adam_case, sizes=(1003, 4096, 7), offset=0))
case("clip_adam[3-tensors-4-byte-offset]", "mia_clip_adam")(functools.partial(_adam_case, sizes=(1003, 4096, 7), offset=4))
case("clip_adam[300001-4-byte-offset]", "mia_clip_adam")(functools.partial(_adam_case, sizes=(300_001, 7), offset=4))


@case("logmel_fwd[B3-T5000]", "mia_logmel_fwd")
def _logmel(dev):
    from src.datasets.features import GpuLogMel
    B, T = 3, 5000
    frames = 1 + T // 160
    lm = GpuLogMel()
    t = lm.tables(dev)
    wav = rnd(dev, (B, T), F32, 190, 0.3)

    def run(ctx):
        out = ctx.out("out", (B, 128, frames), F32)
        err = ctx.out("err", 8, I32)
        err.zero_()  # the header: zero before the first call
        ws = ctx.ws("workspace", ctx.lib.mia_logmel_workspace_bytes(B, frames))
        ctx.call("mia_logmel_fwd", p(wav), B, T, T, lm.cfg, p(t["window"]), p(t["tw512"]), p(t["tw1024"]), p(t["band_start"]),
                 p(t["band_len"]), p(t["band_off"]), p(t["band_w"]), p(out), p(ws), p(err))
    return run


@case("augment+loss", "mia_bc_mix", "mia_bc_partner", "mia_soft_ce", "mia_stretch_gain", "mia_spec_augment_mixup")
def _augment(dev):
    B, T, Np, C = 5, 5000, 9, 50
    x, pool = rnd(dev, (B, T), F32, 191, 0.3), rnd(dev, (Np, T), F32, 192, 0.3)
    labels = torch.tensor([3, 7, 7, 11, 49], dtype=I64, device=dev)
    plabels = torch.tensor([3, 7, 1, 2, 11, 49, 0, 7, 3], dtype=I64, device=dev)
    partner = torch.tensor([2, 0, -1, 8, 4], dtype=I32, device=dev)
    r, u = uni(dev, B, 0.0, 1.0, 193), uni(dev, B, 0.0, 1.0, 194)
    logits, y = rnd(dev, (B, C), F32, 195), torch.softmax(rnd(dev, (B, C), F32, 196), 1)
    factor = torch.tensor([0.8, 1.25, 0.0, 1.0, 1.1], dtype=F64, device=dev)
    gain = uni(dev, B, 0.5, 2.0, 197)
    Fm, Tf = 24, 101
    spec, spool = rnd(dev, (B, Fm, Tf), F32, 198), rnd(dev, (Np, Fm, Tf), F32, 199)
    t0, tl = torch.tensor([0, 5, 90, 50, 100], dtype=I32, device=dev), torch.tensor([3, 0, 11, 20, 1], dtype=I32, device=dev)
    f0, fl = torch.tensor([0, 2, 20, 10, 23], dtype=I32, device=dev), torch.tensor([2, 0, 4, 5, 1], dtype=I32, device=dev)
    lam = uni(dev, B, 0.0, 1.0, 200)

    def run(ctx):
        out, yo, po = ctx.out("bc_mix.out", (B, T), F32), ctx.out("bc_mix.yout", (B, C), F32), ctx.out("bc_mix.p_out", B, F32)
        ws = ctx.ws("bc_mix.workspace", 2 * B * 4)  # the header: 2*B floats
        ctx.call("mia_bc_mix", p(x), p(pool), T, B, p(partner), p(r), p(labels), p(plabels), C, p(out), p(yo), p(po), p(ws))
        pt = ctx.out("bc_partner.partner", B, I32)
        ctx.call("mia_bc_partner", p(labels), B, p(plabels), Np, p(u), p(pt))
        for sig in (0, 1):
            lo, dl, co = ctx.out(f"soft_ce[{sig}].loss", 1, F32), ctx.out(f"soft_ce[{sig}].dlogits", (B, C), F32), ctx.out(f"soft_ce[{sig}].correct", 1, I32)
            ctx.call("mia_soft_ce", p(logits), p(y), B, C, sig, p(lo), p(dl), p(co))
        so = ctx.out("stretch_gain.out", (B, T), F32)
        ctx.call("mia_stretch_gain", p(x), T, B, p(factor), p(gain), p(so))
        ao = ctx.out("spec_augment_mixup.out", (B, Fm, Tf), F32)
        ctx.call("mia_spec_augment_mixup", p(spec), p(spool), p(ao), B, Fm, Tf, p(t0), p(tl), p(f0), p(fl), p(partner), p(lam))
    return run


def _elementwise(dev, numel):
    xf, xb, res = rnd(dev, numel, F32, 201), rnd(dev, numel, BF16, 202), rnd(dev, numel, F32, 203)

    def run(ctx):
        for s, d in ((xf, BF16), (xb, F32), (xf, F32)):
            o = ctx.out(f"cast[{s.dtype}->{d}]", numel, d)
            ctx.call("mia_cast", p(s), code(s.dtype), p(o), code(d), numel)
        for src in (xf, xb):
            o = ctx.out(f"dropout[{src.dtype}]", numel, src.dtype)
            o.copy_(src)
            ctx.call("mia_dropout", p(o), code(src.dtype), numel, 0.3, 77)
            for d in (F32, BF16):
                o = ctx.out(f"dropout_apply[{src.dtype}->{d}]", numel, d)
                ctx.call("mia_dropout_apply", p(src), code(src.dtype), p(res), p(o), code(d), numel, 0.3, 77)
            o = ctx.out(f"add_inplace[{src.dtype}]", numel, F32)
            o.copy_(res)
            ctx.call("mia_add_inplace", p(o), p(src), code(src.dtype), numel)
    return run


for _n in (1, 1003):
    case(f"elementwise[{_n}]", "mia_cast", "mia_dropout", "mia_dropout_apply", "mia_add_inplace")(functools.partial(_elementwise, numel=_n))


def _tokens(dev, D):
    B, Np = 3, 7
    patches, cls, pos = rnd(dev, (B, Np, D), F32, 204), rnd(dev, D, F32, 205), rnd(dev, (Np + 1, D), F32, 206)
    dout, x0 = rnd(dev, (B, Np + 1, D), F32, 207), rnd(dev, (B, Np + 1, D), F32, 208)

    def run(ctx):
        o = ctx.out("tokens_fwd.out", (B, Np + 1, D), F32)
        ctx.call("mia_tokens_fwd", p(patches), p(cls), p(pos), p(o), B, Np, D)
        dp, dc, dpos = ctx.out("tokens_bwd.dpatches", (B, Np, D), F32), ctx.out("tokens_bwd.dcls", D, F32), ctx.out("tokens_bwd.dpos", (Np + 1, D), F32)
        ctx.call("mia_tokens_bwd", p(dout), p(dp), p(dc), p(dpos), B, Np, D)
        dc2, dpos2 = ctx.out("tokens_bwd[no dpatches].dcls", D, F32), ctx.out("tokens_bwd[no dpatches].dpos", (Np + 1, D), F32)
        ctx.call("mia_tokens_bwd", p(dout), None, p(dc2), p(dpos2), B, Np, D)
        if D % 4 == 0:
            x = ctx.out("tokens_fwd_inplace.x", (B, Np + 1, D), F32)
            x.copy_(x0)
            ctx.call("mia_tokens_fwd_inplace", p(x), p(cls), p(pos), B, Np + 1, D)
    return run


case("tokens[D6]", "mia_tokens_fwd", "mia_tokens_bwd")(functools.partial(_tokens, D=6))
case("tokens[D768]", "mia_tokens_fwd", "mia_tokens_bwd", "mia_tokens_fwd_inplace")(functools.partial(_tokens, D=768))


@case("ast_patches+calibration", "mia_ast_patches", "mia_stream_copy", "mia_mfma_rate")
def _patches(dev):
    B, Fm, Tf, ps, st = 2, 32, 50, 16, 10
    N = ((Fm - ps) // st + 1) * ((Tf - ps) // st + 1) + 1
    spec, src = rnd(dev, (B, Fm, Tf), F32, 209), rnd(dev, 1000 * 4, F32, 210)

    def run(ctx):
        o = ctx.out("ast_patches.out", (B * N, ps * ps), BF16)
        ctx.call("mia_ast_patches", p(spec), B, Fm, Tf, ps, st, p(o))
        d = ctx.out("stream_copy.dst", 4000, F32)
        ctx.call("mia_stream_copy", p(src), p(d), 16000)
        sink = ctx.out("mfma_rate.sink", int(ctx.lib.mia_mfma_rate_sink_floats(1)), F32)
        ctx.call("mia_mfma_rate", p(sink), 4, 1)
    return run


COVERS = {name: covers for name, (covers, _) in CASES.items()}


# ================================================================================================ the tests
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_memory_contract(cuda, monkeypatch, name):
    run_three(cuda, CASES[name][1](cuda), monkeypatch)


# ================================================================================================ one step per model
def _envnet(dev):
    from oracle.synth import synth_waveform
    from src.models.envnet_v2 import EnvNetV2
    torch.manual_seed(0)
    with torch.device(dev):  # FC1 alone is 346M parameters: initialise them on the GPU
        m = EnvNetV2(num_classes=50, dropout=0.0, compute_dtype="bf16")
    x = torch.from_numpy(synth_waveform(21, 2, 220_500)[:, None, :]).to(dev)
    return m.to(dev).train(), x, 50


def _ast(dev):
    from oracle import ast as oast
    from oracle.synth import hash_uniform
    from src.models.ast import ASTModel
    hw, hb = oast.head_hash(901, 10)
    m = ASTModel(num_classes=10, compute_dtype="bf16", depth=2)
    m.load_vit_state(oast.deit_hash_state(300, depth=2))
    with torch.no_grad():
        m.head.weight.copy_(torch.from_numpy(hw))
        m.head.bias.copy_(torch.from_numpy(hb))
    return m.to(dev).train(), torch.from_numpy(hash_uniform(31, (2, 128, 1379))).to(dev), 10


def _leaf(dev):
    from src.models.leaf import LeafModel
    torch.manual_seed(0)
    m = LeafModel(n_filters=16, kernel_size=33, num_classes=5, compute_dtype="bf16")
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    x = torch.randn(4, 1, 160 * 40, generator=torch.Generator().manual_seed(1))
    return m.to(dev).train(), x.to(dev), 5


def _mini(dev):
    from src.models.ast_mini import ASTMiniViT
    from tests import _ast_small_ref as R
    _, kw, _, (_, _, si, _) = R.CASES["M"]
    m = ASTMiniViT(**kw)
    ks = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in R.hash_init(ks, si).items()}, strict=True)
    m.compute_dtype = "bf16"
    m = m.to(dev).train()
    m.dropout_seeds = R.case_seeds("M")
    return m, torch.from_numpy(R.case_inputs("M")[0]).to(dev), kw["num_classes"]


MODELS = {"EnvNetV2-bf16-B2": _envnet, "ASTModel-bf16-depth2-B2": _ast, "LeafModel-bf16": _leaf, "ASTMiniViT-bf16": _mini}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_model_step_memory_contract(cuda, monkeypatch, name):
    """Forward + loss + backward + FusedAdam.step() with every ``kernels.workspace`` request served exactly, fresh
    and poisoned from a chunked arena (64 KiB guards): guards clean; loss, every gradient and every updated
    parameter bit-identical between the two poisons and the unpatched run."""
    from src.training.optim import FusedAdam

    m, x, C = MODELS[name](cuda)  # built once; every run starts from the same state
    snap = {k: v.detach().clone() for k, v in m.state_dict().items()}

    def run(ctx):
        m.load_state_dict(snap)
        for q in m.parameters():
            q.grad = None
        y = torch.zeros(x.shape[0], C, device=cuda)
        y[torch.arange(x.shape[0]), torch.arange(x.shape[0]) % C] = 1.0
        opt = FusedAdam(m.parameters(), lr=1e-3, weight_decay=1e-4, clip=1.0)
        z = m(x)
        loss, dz, _ = K.soft_ce(z.detach().float().contiguous(), y, input_sigmoid=False)
        z.backward(dz.to(z.dtype))
        ctx.outs["loss"] = loss.reshape(1).clone()
        for k, q in m.named_parameters():
            if q.grad is not None:
                ctx.outs[f"grad {k}"] = q.grad.detach().clone()
        opt.step()
        ctx.outs["total_norm"] = opt.last_total_norm.reshape(1).clone()
        for k, q in m.named_parameters():
            ctx.outs[f"param {k}"] = q.detach().clone()
        assert sum(k.startswith("grad ") for k in ctx.outs) >= 4
        assert ctx.arena is None or len(ctx.arena.entries) >= 4  # the step did go through the patched workspace

    run_three(cuda, run, monkeypatch, chunk=256 << 20)
    K.check_attention_errors()


@pytest.mark.gpu
def test_harness_sees_a_result_that_depends_on_the_workspace(cuda, monkeypatch):
    """The three-run comparison on torch ops alone: an output formed from workspace words that were never written
    (first case), and an output of which one element is never written (second case), fail the comparison."""
    def reads_unwritten(ctx):
        ws = ctx.ws("workspace", 64)
        ws[:32] = 1
        ctx.out("out", 16, F32).copy_(ws[16:48].view(I32)[:8].float().repeat(2))

    def leaves_a_hole(ctx):
        ctx.out("out", 16, F32)[:15] = 1.0

    def clean(ctx):
        ws = ctx.ws("workspace", 64)
        ws[:] = 3
        ctx.out("out", 16, F32).copy_(ws[:64].view(I32).float())

    for bad in (reads_unwritten, leaves_a_hole):
        with pytest.raises(AssertionError, match="differs between poison 0xFF and 0x00"):
            run_three(cuda, bad, monkeypatch)
    run_three(cuda, clean, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [0xFF, 0x00])
def test_harness_sees_a_torch_write_past_a_taken_buffer(cuda, poison):
    """The harness on the GPU: a torch op that writes 16 bytes behind a taken buffer (inside the arena's own
    guard), and one that writes 2 bytes in front of another, make check() raise."""
    a = GuardedArena(cuda, poison)
    a.f32("clean", 100)
    out = a.bf16("out", (3, 52))
    e = a.entries[-1]
    torch.cuda.synchronize()
    a.check()
    e.store[e.start + e.nbytes:e.start + e.nbytes + 16] = 0x5A
    torch.cuda.synchronize()
    with pytest.raises(GuardDamage, match=r"'out' \(312 bytes\).*past the end: 16 byte\(s\), first at offset \+0, last at offset \+15"):
        a.check()
    e.store[e.start + e.nbytes:e.start + e.nbytes + 16] = poison
    e0 = a.entries[0]
    e0.store[e0.start - 2:e0.start] = 0x5A
    torch.cuda.synchronize()
    with pytest.raises(GuardDamage, match=r"'clean' \(400 bytes\).*before the start: 2 byte\(s\), first at offset -2, last at offset -1"):
        a.check()
    assert out.numel() == 156
