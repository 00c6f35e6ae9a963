"""LEAF frontend on the MI355X: learnable Gabor filterbank -> squared modulus -> average pool -> PCEN.

The frontend of the reference's ``LeafModel`` (its ``gabor``, ``downsample`` and ``pcen`` members, in the
order its forward applies them).  ``LeafFrontend`` keeps the reference's parameter names and shapes for
those modules, so their part of a reference checkpoint loads as is:

    gabor.center_freqs [F]   gabor.bandwidths [F]   gabor.window [1, Kt] (buffer)
    pcen.alpha [F] (unused, no gradient)   pcen.delta [F]   pcen.r [F]

The filter taps are synthesised by torch elementwise ops on [F, Kt] tensors (autograd carries the bank
gradient back to ``center_freqs`` / ``bandwidths``); energy + pooling and PCEN are two autograd Functions
over the HIP kernels (``mia_leaf_energy_*``, ``mia_pcen_*``): no [B, F, T] tensor is ever written.
A CPU tensor takes the same math on torch ops (plumbing runs without a GPU).

``LeafModel`` puts the reference's trunk and classifier behind it: the energy kernel, then one autograd node
(``_LeafTrunk``) over channels-last PCEN (``mia_lt_pcen_*``), three ``mia_gemm`` convolutions each followed by
the fused BN-statistics + max-pool kernels (``mia_lt_pool_*``), the time mean and the four linears.
"""
from __future__ import annotations

import itertools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F_

from ..miaudio import kernels as K
from ..miaudio import lib as L
from .bn_cma import update_factor


class GaborFilters(nn.Module):
    """Parameters of the Gabor bank and its tap synthesis: ``filters()`` -> w [2][F][Kt] (re, im)."""

    def __init__(self, n_filters=186, kernel_size=401, sample_rate=44100, min_freq=60.0, max_freq=7800.0):
        super().__init__()
        self.n_filters, self.kernel_size, self.sample_rate = int(n_filters), int(kernel_size), int(sample_rate)
        self.center_freqs = nn.Parameter(torch.linspace(min_freq, max_freq, n_filters) / (sample_rate / 2))
        self.bandwidths = nn.Parameter(torch.full((n_filters,), 1.0))
        self.register_buffer("window", torch.hann_window(kernel_size).unsqueeze(0))

    def filters(self) -> torch.Tensor:
        h = self.kernel_size // 2
        dev = self.center_freqs.device
        t = (torch.arange(self.kernel_size, device=dev) - h).to(torch.float32) / self.sample_rate
        t = t.view(1, -1)
        cf = self.center_freqs.view(-1, 1)
        bw = self.bandwidths.view(-1, 1)
        env = torch.exp(-0.5 * (t * bw * self.sample_rate) ** 2) * self.window
        # cf is Hz / (sr / 2) and multiplies t in seconds with no further sample-rate factor, as the reference
        ph = 2 * math.pi * cf * t
        return torch.stack([torch.cos(ph) * env, torch.sin(ph) * env])


class PCENParams(nn.Module):
    def __init__(self, num_channels, alpha=0.98, delta=2.0, r=0.5, eps=1e-6, s=0.04):
        super().__init__()
        self.eps = eps
        self.alpha = nn.Parameter(torch.full((num_channels,), alpha))  # present in the reference, takes no part
        self.delta = nn.Parameter(torch.full((num_channels,), delta))
        self.r = nn.Parameter(torch.full((num_channels,), r))
        self.s = s


class _LeafEnergy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, pool, compute):
        ctx.save_for_backward(x, w)
        ctx.pool, ctx.compute = pool, compute
        return K.leaf_energy_fwd(x, w, pool, compute, tag="leaf.energy.fwd")

    @staticmethod
    def backward(ctx, gP):
        x, w = ctx.saved_tensors
        dw = None
        if ctx.needs_input_grad[1]:
            dw = K.leaf_energy_bwd(x, w, gP.contiguous().float(), ctx.pool, ctx.compute, tag="leaf.energy.bwd")
        return None, dw, None, None


class _PCEN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, r, delta, eps):
        ctx.save_for_backward(P, r, delta)
        ctx.eps = eps
        return K.pcen_fwd(P, r, delta, eps, tag="leaf.pcen.fwd")

    @staticmethod
    def backward(ctx, gy):
        P, r, delta = ctx.saved_tensors
        gP, dr, dd = K.pcen_bwd(P, r, delta, ctx.eps, gy.contiguous().float(), tag="leaf.pcen.bwd")
        return gP, dr, dd, None


class LeafFrontend(nn.Module):
    """(B, 1, T) or (B, T) f32 waveform -> (B, F, T // pool) PCEN-compressed Gabor energies."""

    def __init__(self, n_filters: int = 186, kernel_size: int = 401, sample_rate: int = 44100, pool: int = 160,
                 compute_dtype: str | None = "bf16"):
        super().__init__()
        K.leaf_check_args(1, pool, n_filters, kernel_size, pool)
        self.pool = int(pool)
        self.compute_dtype = compute_dtype
        self.gabor = GaborFilters(n_filters, kernel_size, sample_rate)
        self.pcen = PCENParams(n_filters)

    def _compute_code(self) -> int:
        cd = self.compute_dtype
        if cd is None:
            if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16:
                return L.BF16
            return L.F32
        return {"bf16": L.BF16, "bfloat16": L.BF16, "f32": L.F32, "fp32": L.F32, "32": L.F32, "fp8": L.BF16}[str(cd)]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 3 and x.shape[1] == 1:
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ValueError(f"LeafFrontend expects (B,1,T) or (B,T), got {tuple(x.shape)}")
        if x.requires_grad:
            raise RuntimeError("LeafFrontend: the waveform must not require grad (the kernels produce no dx)")
        K.leaf_check_args(x.shape[0], x.shape[1], self.gabor.n_filters, self.gabor.kernel_size, self.pool)
        if not x.is_cuda:
            return self._cpu_forward(x)
        with torch.autocast("cuda", enabled=False):
            w = self.gabor.filters()
            P = _LeafEnergy.apply(x.float().contiguous(), w, self.pool, self._compute_code())
            return _PCEN.apply(P, self.pcen.r, self.pcen.delta, self.pcen.eps)

    def _cpu_forward(self, x: torch.Tensor) -> torch.Tensor:
        """accelerator=cpu plumbing: the same formulas on torch's CPU ops, in the input's dtype."""
        w = self.gabor.filters().to(x.dtype)
        h = self.gabor.kernel_size // 2
        z = F_.conv1d(x[:, None, :], w.reshape(-1, 1, w.shape[-1]), padding=h)
        nf = self.gabor.n_filters
        P = F_.avg_pool1d(z[:, :nf] ** 2 + z[:, nf:] ** 2, self.pool)
        M = F_.avg_pool1d(P, 5, stride=1, padding=2)  # count_include_pad: the divisor stays 5 at the edges
        r, d = self.pcen.r.to(x.dtype).view(1, -1, 1), self.pcen.delta.to(x.dtype).view(1, -1, 1)
        return torch.log(P / (self.pcen.eps + M) ** r + d)


# ------------------------------------------------------------------------------------------------ LeafModel
# (conv index in conv_block, BN index, kernel size, pool window); widths come from the modules
TRUNK_BLOCKS = ((0, 1, 5, 4), (4, 5, 3, 4), (8, 9, 3, 2))
MLP_LAYERS = ((0, 1, 3), (4, 5, 7), (8, 9, 11))  # (Linear, BatchNorm1d, Dropout) indices in classifier
_SEED = itertools.count(0x1EAF)


def _momentum(bn: nn.BatchNorm1d, training: bool) -> float:
    """The update factor of this forward (momentum, or 1/k with momentum=None); a training forward is counted in
    ``num_batches_tracked`` on the device (bn_cma.update_factor)."""
    return update_factor(bn, training, True)


def _trunk_params(m: "LeafModel"):
    """Flat parameter order handed to the autograd Function (also the gradient order)."""
    ps = [m.pcen.r, m.pcen.delta]
    for ci, bi, _, _ in TRUNK_BLOCKS:
        ps += [m.conv_block[ci].weight, m.conv_block[ci].bias, m.conv_block[bi].weight, m.conv_block[bi].bias]
    for li, bi, _ in MLP_LAYERS:
        ps += [m.classifier[li].weight, m.classifier[li].bias, m.classifier[bi].weight, m.classifier[bi].bias]
    ps += [m.classifier[12].weight, m.classifier[12].bias]
    return ps


def _mlp_forward(model, p, h, cd, training):
    """(per-layer saved tensors, logits) of the classifier on (B, 512) rows."""
    B, dev, tdt = h.shape[0], h.device, L.torch_dtype(cd)
    mlp = []
    for j, (li, bi, di) in enumerate(MLP_LAYERS):
        Wt, bias, bnm = p[14 + 4 * j], p[15 + 4 * j], model.classifier[bi]
        fout, fin = Wt.shape
        if cd == L.BF16:
            Wt = K.bf16_shadow(Wt)
        u = torch.empty(B, fout, dtype=tdt, device=dev)
        K.gemm(K.dense(h, L.KC, B, fin), K.dense(Wt, L.KC, fout, fin), K.epilogue(u, fout, bias=bias), B, fout, fin, cd)
        bn = K.bn_fwd_stats(u, B, fout, bnm.weight, bnm.bias, bnm.running_mean, bnm.running_var,
                            _momentum(bnm, training), bnm.eps, training)
        a = K.lt_pool_apply(u.view(B, 1, fout), B, 1, fout, bn, tdt).view(B, fout)
        drop = float(model.classifier[di].p) if training else 0.0
        if drop > 0:
            K.dropout_(a, drop, next(_SEED) * 0x9E3779B1)
        mlp.append(dict(hin=h, W=Wt, u=u, bn=bn, a=a, drop=drop))
        h = a
    W4, b4 = p[26], p[27]
    logits = torch.empty(B, W4.shape[0], dtype=torch.float32, device=dev)
    K.gemm(K.dense(h, L.KC, B, W4.shape[1]), K.dense(W4, L.KC, W4.shape[0], W4.shape[1]),
           K.epilogue(logits, W4.shape[0], bias=b4), B, W4.shape[0], W4.shape[1], cd)
    return mlp, logits


def _mlp_backward(model, s, dcur, grads, dbg):
    """Classifier backward: fills grads[14:28], returns dh (B, 512), the gradient of the time mean."""
    B, cd, dev = s["B"], s["cd"], dcur.device
    tdt = L.torch_dtype(cd)
    W4 = s["W4"]
    fout, fin = W4.shape
    last = s["mlp"][2]
    dW = torch.empty(fout, fin, dtype=torch.float32, device=dev)
    K.gemm(K.dense(dcur, L.RC, B, fout), K.dense(last["a"], L.RC, B, fin), K.epilogue(dW, fin), fout, fin, B, cd)
    grads[26], grads[27] = dW, K.colsum(dcur, B, fout)
    dv = torch.empty(B, fin, dtype=tdt, device=dev)
    keep = 1.0 / (1.0 - last["drop"]) if last["drop"] > 0 else 1.0
    K.gemm(K.dense(dcur, L.KC, B, fout), K.dense(W4, L.RC, fout, fin),
           K.epilogue(dv, fin, act=L.DACT_NZ, aux=last["a"], ldaux=fin, act_scale=keep), B, fin, fout, cd)
    for j in (2, 1, 0):
        ml = s["mlp"][j]
        if dbg is not None:
            dbg["dv"][j] = dv
        bnm = model.classifier[MLP_LAYERS[j][1]]
        fout, fin = ml["W"].shape
        dg, db = K.bn_relu_bwd_reduce(dv, None, ml["u"], B, fout, ml["bn"])
        du = torch.empty(B, fout, dtype=tdt, device=dev)
        dbias = torch.empty(fout, dtype=torch.float32, device=dev)
        K.bn_relu_bwd_apply(dv, ml["u"], du, B, fout, bnm.weight, ml["bn"], dg, db, dbias)
        if dbg is not None:
            dbg["du"][j] = du
        dW = torch.empty(fout, fin, dtype=torch.float32, device=dev)
        K.gemm(K.dense(du, L.RC, B, fout), K.dense(ml["hin"], L.RC, B, fin), K.epilogue(dW, fin), fout, fin, B, cd)
        grads[14 + 4 * j: 18 + 4 * j] = [dW, dbias, dg, db]
        dv = torch.empty(B, fin, dtype=tdt, device=dev)
        if j > 0:
            prev = s["mlp"][j - 1]
            keep = 1.0 / (1.0 - prev["drop"]) if prev["drop"] > 0 else 1.0
            epi = K.epilogue(dv, fin, act=L.DACT_NZ, aux=prev["a"], ldaux=fin, act_scale=keep)
        else:
            epi = K.epilogue(dv, fin)
        K.gemm(K.dense(du, L.KC, B, fout), K.dense(ml["W"], L.RC, fout, fin), epi, B, fin, fout, cd)
    if dbg is not None:
        dbg["dh"] = dv
    return dv


class _LeafTrunk(torch.autograd.Function):
    """P [B][F][Tp] (pooled Gabor energy) -> logits: channels-last PCEN, the three conv blocks (mia_gemm convs
    around the mia_lt_* glue), the time mean and the classifier, as one autograd node.

    ``capture``: None in production.  A test may set it to a callable ``capture(kind, tensors)``; it is then handed
    the forward's saved tensors ("forward") and the backward's dv / du / dz / dinp ("backward").  Nothing is kept on the
    module."""
    capture = None

    @staticmethod
    def forward(ctx, model, P, cd, *p):
        training = model.training
        tdt = L.torch_dtype(cd)
        dev = P.device
        B, F, Tp = P.shape
        Fp = (F + 7) // 8 * 8
        s = {"B": B, "F": F, "Fp": Fp, "Tp": Tp, "cd": cd, "training": training, "P": P}

        def finalize(bnm, z, st, rows, C, kshift):
            if training:
                return K.bn_finalize_shifted(st[0], st[1], rows, C, kshift, bnm.weight, bnm.bias, bnm.running_mean,
                                             bnm.running_var, _momentum(bnm, True), bnm.eps)
            return K.bn_fwd_stats(z, rows, C, bnm.weight, bnm.bias, bnm.running_mean, bnm.running_var,
                                  _momentum(bnm, False), bnm.eps, False)

        y = K.lt_pcen_fwd(P, p[0], p[1], model.pcen.eps, tdt, tag="leaf.pcen_cl.fwd")
        # forward (OHWI) packs of the three conv weights; conv1's input channels F .. Fp - 1 are zero columns
        w4 = []
        for l, (ci, _, k, _) in enumerate(TRUNK_BLOCKS):
            w = p[2 + 4 * l]
            if l == 0 and Fp != F:
                w = torch.nn.functional.pad(w, (0, 0, 0, Fp - F))
            w4.append(w.reshape(w.shape[0], w.shape[1], 1, k).contiguous())
        wpk = K.pack_weights([(w, cd, 0) for w in w4])
        inp, T = y, Tp
        blocks = []
        for l, (ci, bi, k, pk) in enumerate(TRUNK_BLOCKS):
            cout, cin = w4[l].shape[0], w4[l].shape[1]
            bias, bnm = p[3 + 4 * l], model.conv_block[bi]
            if T < pk:
                raise ValueError(f"LeafModel: {T} frames reach conv block {l}, fewer than its pool window {pk}")
            z = torch.empty(B, T, cout, dtype=tdt, device=dev)
            K.gemm(K.conv(inp, L.KC, B, 1, T, cin, 1, T, 1, k, pw=k // 2), K.dense(wpk[l], L.KC, cout, k * cin),
                   K.epilogue(z, cout, bias=bias), B * T, cout, k * cin, cd, tag=f"leaf.b{l}.conv.fwd")
            with K.probe(f"leaf.b{l}.glue.fwd", 0.0, 0.0):
                win, am, part, nblk = K.lt_pool_stats(z, B, T, cout, pk, bnm.weight, bias, stats=training)
                bn = finalize(bnm, z, (part, nblk), B * T, cout, bias)
                out = K.lt_pool_apply(win, B, T // pk, cout, bn, tdt, mean=(l == 2))
            blocks.append(dict(inp=inp, z=z, win=win, am=am, bn=bn, T=T, cin=cin, cout=cout, w4=w4[l]))
            inp, T = out, T // pk
        s["blocks"] = blocks
        # classifier: Linear -> BN -> ReLU -> Dropout three times (rows = clips), then the last Linear in f32
        with K.probe("leaf.mlp.fwd", 0.0, 0.0):
            mlp, logits = _mlp_forward(model, p, inp, cd, training)  # inp (B, 512): the time mean of block 3
        s["mlp"], s["W4"] = mlp, p[26]
        if _LeafTrunk.capture is not None:
            _LeafTrunk.capture("forward", s)
        ctx.s, ctx.model, ctx.p = s, model, p
        return logits

    @staticmethod
    def backward(ctx, glogits):
        s, model, p = ctx.s, ctx.model, ctx.p
        if not s["training"]:
            raise RuntimeError("LeafModel: the backward of eval-mode BatchNorm (running statistics) is not built; "
                               "call model.train() for a training step")
        B, cd = s["B"], s["cd"]
        tdt = L.torch_dtype(cd)
        dev = glogits.device
        grads = [None] * len(p)
        dbg = {"dv": {}, "du": {}, "dz": {}, "dinp": {}} if _LeafTrunk.capture is not None else None
        with K.probe("leaf.mlp.bwd", 0.0, 0.0):
            dv = _mlp_backward(model, s, glogits.contiguous().float(), grads, dbg)
        # ---- conv blocks; the flipped backward-data operands in one launch
        wfl = K.pack_weights([(b["w4"], cd, 1) for b in s["blocks"]])
        dout = dv
        for l in (2, 1, 0):
            b = s["blocks"][l]
            ci, bi, k, pk = TRUNK_BLOCKS[l]
            T, cin, cout = b["T"], b["cin"], b["cout"]
            bnm = model.conv_block[bi]
            with K.probe(f"leaf.b{l}.glue.bwd", 0.0, 0.0):
                gm, dg, db = K.lt_pool_bwd_gather(dout, b["win"], B, T // pk, cout, b["bn"], mean=(l == 2))
                dz, dbias = K.lt_pool_bwd_apply(gm, b["am"], b["z"], B, T, cout, pk, bnm.weight, b["bn"], dg, db)
            if dbg is not None:
                dbg["dz"][l] = dz
            dWp = torch.empty(cout, k * cin, dtype=torch.float32, device=dev)
            K.gemm(K.dense(dz, L.RC, B * T, cout), K.conv(b["inp"], L.RC, B, 1, T, cin, 1, T, 1, k, pw=k // 2),
                   K.epilogue(dWp, k * cin), cout, k * cin, B * T, cd, tag=f"leaf.b{l}.conv.wgrad")
            gw = torch.empty(cout, cin, 1, k, dtype=torch.float32, device=dev)
            K.unpack_ohwi_grad(dWp, (cout, cin, 1, k), gw)
            gw = gw.view(cout, cin, k)
            if l == 0 and cin != s["F"]:
                gw = gw[:, :s["F"]].contiguous()  # the zero pad columns' gradient is discarded
            grads[2 + 4 * l: 6 + 4 * l] = [gw, dbias, dg, db]
            dinp = torch.empty(B, T, cin, dtype=tdt, device=dev)
            K.gemm(K.conv(dz, L.KC, B, 1, T, cout, 1, T, 1, k, pw=k - 1 - k // 2),
                   K.dense(wfl[l], L.KC, cin, k * cout), K.epilogue(dinp, cin), B * T, cin, k * cout, cd,
                   tag=f"leaf.b{l}.conv.dgrad")
            if dbg is not None:
                dbg["dinp"][l] = dinp
            dout = dinp
        gP, dr, dd = K.lt_pcen_bwd(s["P"], p[0], p[1], model.pcen.eps, dout, tag="leaf.pcen_cl.bwd")
        grads[0], grads[1] = dr, dd
        if dbg is not None:
            _LeafTrunk.capture("backward", dbg)
        ctx.s = None
        return (None, gP, None, *grads)


class LeafModel(nn.Module):
    """Drop-in for the reference ``src.models.leaf.LeafModel`` (same constructor, module tree and parameter names,
    default ``nn`` initialisation): (B, 1, T) or (B, T) waveform -> (B, num_classes) f32 logits.

    On the GPU the Gabor energy kernel, channels-last PCEN, the three conv blocks and the classifier run on the
    HIP kernels (``_LeafEnergy`` + ``_LeafTrunk``); the ``nn`` modules only hold the parameters and buffers.  A CPU
    tensor takes the same module sequence on torch ops (plumbing; never the oracle).  ``compute_dtype``: None follows
    autocast, "bf16" / "f32" force a mode, "fp8" runs bf16.

    The conv biases and ``classifier.{0,4,8}.bias`` feed a BatchNorm: their true gradient is zero, what comes out is
    rounding noise (the reference has the same structure); the outputs do not depend on them.
    """

    def __init__(self, n_filters: int = 186, kernel_size: int = 401, sample_rate: int = 44100, num_classes: int = 50,
                 compute_dtype: str | None = None):
        super().__init__()
        self.pool = 160
        K.leaf_check_args(1, self.pool, n_filters, kernel_size, self.pool)
        if n_filters > 1024:
            raise ValueError(f"LeafModel: n_filters {n_filters} > 1024")
        self.compute_dtype = compute_dtype
        self.gabor = GaborFilters(n_filters, kernel_size, sample_rate)
        self.pcen = PCENParams(n_filters)
        self.downsample = nn.AvgPool1d(kernel_size=self.pool, stride=self.pool)
        self.conv_block = nn.Sequential(
            nn.Conv1d(n_filters, 256, kernel_size=5, stride=1, padding=2), nn.BatchNorm1d(256), nn.ReLU(),
            nn.MaxPool1d(4),
            nn.Conv1d(256, 384, kernel_size=3, stride=1, padding=1), nn.BatchNorm1d(384), nn.ReLU(),
            nn.MaxPool1d(4),
            nn.Conv1d(384, 512, kernel_size=3, stride=1, padding=1), nn.BatchNorm1d(512), nn.ReLU(),
            nn.MaxPool1d(2),
        )
        self.pooling = nn.AdaptiveAvgPool1d(1)
        self.classifier = nn.Sequential(
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(256, 512), nn.BatchNorm1d(512), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(512, 256), nn.BatchNorm1d(256), nn.ReLU(), nn.Dropout(0.3),
            nn.Linear(256, num_classes),
        )

    _compute_code = LeafFrontend._compute_code

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.ndim == 3 and x.shape[1] == 1:
            x = x[:, 0, :]
        if x.ndim != 2:
            raise ValueError(f"LeafModel expects (B,1,T) or (B,T), got {tuple(x.shape)}")
        if x.requires_grad:
            raise RuntimeError("LeafModel: the waveform must not require grad (the kernels produce no dx)")
        if self.training and x.shape[0] == 1:
            raise ValueError("LeafModel: a training-mode batch of one clip has no BatchNorm1d variance "
                             "(Expected more than 1 value per channel when training)")
        K.leaf_check_args(x.shape[0], x.shape[1], self.gabor.n_filters, self.gabor.kernel_size, self.pool)
        if not x.is_cuda:
            return self._cpu_forward(x)
        with torch.autocast("cuda", enabled=False):
            cd = self._compute_code()
            w = self.gabor.filters()
            P = _LeafEnergy.apply(x.float().contiguous(), w, self.pool, cd)
            return _LeafTrunk.apply(self, P, cd, *_trunk_params(self))

    def _cpu_forward(self, x: torch.Tensor) -> torch.Tensor:
        """accelerator=cpu plumbing: the reference's module sequence on torch's CPU ops."""
        y = LeafFrontend._cpu_forward(self, x)
        return self.classifier(self.pooling(self.conv_block(y)).squeeze(-1))
