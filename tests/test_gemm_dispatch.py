"""CPU: which kernel mia_gemm picks and how much workspace it asks for, as one table.

mia_gemm_path and mia_gemm_workspace_bytes_ex are pure host functions: they look at the descriptors and at
the alignment of the pointers, never behind them, so the operands here carry made-up addresses and no GPU
is needed.  Every row is (descriptors, M, N, K, compute dtype, split_k) -> (path, workspace bytes).

The expected values in EXPECTED were recorded by running this table against a library built from the commit
BEFORE the dispatch decision was gathered into one selector (one if-chain in mia_gemm, restated in
mia_gemm_path and mia_gemm_workspace_bytes_ex); they were not read off the selector.  The table therefore
pins the selector to what the library did when the decision was still spread out, including mia_gemm_path's
documented probe epilogue (plain bf16: N % 8 == 4 reports 5) and the rolling-window 8x8 weight gradient
reporting as path 2.  A pull request that adds or reroutes a path changes rows here on purpose.

The rows cover: every shape whose path tests/test_gpu_gemm.py and tests/test_gpu_exact.py assert; for every
eligibility predicate one row on each side of each of its conditions; split_k 1 against 2 for the forward /
weight-gradient pairs (1 / 2, 4 / 3); and the a_colsum / colsum / split-K workspace sizes on the tile, the
128x128 and the 256x256 paths.
"""
import pytest

from src.miaudio import lib as L

F32, BF16, KC, RC = L.F32, L.BF16, L.KC, L.RC
PTR = 4096  # 16-byte aligned made-up address


def mat(layout, R, Kd, dt=BF16, pad=0, ptr=PTR, pre=L.PRE_NONE):
    """An R x Kd GEMM operand: KC stores [R][Kd], RC stores [Kd][R]; pad widens the row stride."""
    o = L.MiaOperand()
    o.ptr, o.kind, o.dtype, o.layout, o.pre = ptr, L.OP_DENSE, dt, layout, pre
    o.rows, o.cols = (R, Kd) if layout == KC else (Kd, R)
    o.ld = o.cols + pad
    if pre in (L.PRE_AFFINE, L.PRE_AFFINE_RELU):
        o.pre_scale = o.pre_shift = PTR
    return o


def conv(layout, n, h, w, c, kh, kw, sw=1, sh=1, ph=0, pw=0, dt=BF16, pre=L.PRE_NONE, row=False, ptr=PTR,
         oh=None, ow=None):
    o = L.MiaOperand()
    o.ptr, o.kind, o.dtype, o.layout, o.pre = ptr, (L.OP_CONVROW if row else L.OP_CONV), dt, layout, pre
    o.n, o.h, o.w, o.c, o.kh, o.kw, o.sh, o.sw, o.ph, o.pw = n, h, w, c, kh, kw, sh, sw, ph, pw
    o.oh = (h + 2 * ph - kh) // sh + 1 if oh is None else oh
    o.ow = (w + 2 * pw - kw) // sw + 1 if ow is None else ow
    if pre in (L.PRE_AFFINE, L.PRE_AFFINE_RELU):
        o.pre_scale = o.pre_shift = PTR
    return o


def epi(N, dt=BF16, colsum=False, a_colsum=False, pad=0, act=L.ACT_NONE):
    e = L.MiaEpilogue()
    e.ptr, e.dtype, e.ldc, e.alpha, e.act_scale, e.act = PTR, dt, N + pad, 1.0, 1.0, act
    if act != L.ACT_NONE:
        e.aux, e.aux_dtype, e.ldaux = PTR, BF16, N
    if colsum:
        e.colsum = PTR
    if a_colsum:
        e.a_colsum = PTR
    return e


CASES = {}  # id -> (A, B, E, M, N, K, compute, split)
LAYOUTS = {"kk": (KC, KC), "kr": (KC, RC), "rk": (RC, KC), "rr": (RC, RC)}


def add(name, A, B, M, N, Kd, cd=BF16, split=1, E=None):
    assert name not in CASES, name
    CASES[name] = (A, B, E if E is not None else epi(N), M, N, Kd, cd, split)


def gemm(name, M, N, Kd, la=KC, lb=KC, cd=BF16, split=1, dt=BF16, E=None, **kw):
    add(name, mat(la, M, Kd, dt, **kw), mat(lb, N, Kd, dt, **kw), M, N, Kd, cd, split, E)


# ---------------------------------------------------------------- shapes whose path the GPU tests assert
for ln, (la, lb) in LAYOUTS.items():
    for M, N, Kd in [(37, 50, 200), (130, 70, 8), (300, 32, 64), (64, 600, 40), (256, 128, 96)]:
        for split in (1, 3):
            gemm(f"gpu_p0_{M}x{N}x{Kd}_{ln}_s{split}", M, N, Kd, la, lb, split=split)
    for M, N, Kd, split in [(64, 72, 64, 1), (296, 200, 192, 1), (256, 384, 4096, 4), (256, 256, 128, 1),
                            (128, 1000, 512, 1)]:
        gemm(f"gpu_p5_{M}x{N}x{Kd}_{ln}_s{split}", M, N, Kd, la, lb, split=split)
    for M, N, Kd in [(4096, 768, 768), (4136, 2304, 512), (8192, 264, 3072), (8200, 520, 1024)]:
        gemm(f"gpu_p7_{M}x{N}x{Kd}_{ln}", M, N, Kd, la, lb)
gemm("gpu_p5_padded_ld_kr", 296, 200, 192, KC, RC, pad=8)
gemm("gpu_p5_padded_ld_rk", 296, 200, 192, RC, KC, pad=8)
gemm("gpu_p0_f32_compute", 64, 96, 48, cd=F32, dt=F32)
gemm("gpu_p0_bf16_small", 64, 96, 48)
gemm("gpu_p0_staged_f32_storage", 296, 200, 192, dt=F32)
add("gpu_p5_trunk_w2_overlapping_rows", mat(KC, 444, 128, pad=-64), mat(KC, 128, 128), 444, 128, 128)
gemm("gpu_p7_smallest_grid", 2056, 1024, 128)
gemm("gpu_p7_ragged_n_1028", 2056, 1028, 128)
gemm("gpu_p7_ragged_n_260", 4096, 260, 768)
for Kd in (16384 + 64, 16384 + 72):
    gemm(f"gpu_p7_long_k_{Kd}", 264, 264, Kd, RC, RC)
for M, N, Kd in [(768, 2304, 69632 + 100), (2304, 768, 16384), (768, 768, 421120 // 8)]:
    gemm(f"gpu_p7_wgrad_{M}x{N}x{Kd}", M, N, Kd, RC, RC)
for M, N, Kd in [(2304, 768, 16384 + 40), (768 + 8, 768, 421120 // 8), (520, 264, 300)]:
    gemm(f"gpu_a_colsum_{M}x{N}x{Kd}_rr", M, N, Kd, RC, RC, E=epi(N, F32, a_colsum=True))
    gemm(f"gpu_a_colsum_{M}x{N}x{Kd - Kd % 64}_rk", M, N, Kd - Kd % 64, RC, KC, E=epi(N, F32, a_colsum=True))
gemm("gpu_colsum_p5_900x640x256", 900, 640, 256, E=epi(640, colsum=True))
gemm("gpu_colsum_p7_8229x3072x768", 8229, 3072, 768, E=epi(3072, colsum=True))


def rowconv(name, n, cin, cout, h, w, kh, kw, sw=1, split=1, dt=BF16, pre=L.PRE_NONE, wpad=0, wptr=PTR, cd=BF16,
            **kw_):
    A = conv(KC, n, h, w, cin, kh, kw, sw=sw, dt=dt, pre=pre, **kw_)
    Kd = kh * kw * cin
    add(name, A, mat(KC, cout, Kd, pad=wpad, ptr=wptr), n * A.oh * A.ow, cout, Kd, cd, split)


def rowwgrad(name, n, cin, cout, h, w, kh, kw, sw=1, split=2, dt=BF16, dydt=None, pre=L.PRE_NONE, dypad=0, cd=BF16,
             dyptr=PTR, **kw_):
    Bo = conv(RC, n, h, w, cin, kh, kw, sw=sw, dt=dt, pre=pre, **kw_)
    P = n * Bo.oh * Bo.ow
    add(name, mat(RC, cout, P, dt if dydt is None else dydt, pad=dypad, ptr=dyptr), Bo, cout, kh * kw * cin, P, cd,
        split)


RELU = L.PRE_AFFINE_RELU
for i, (n, cin, cout, h, w, kh, kw, sw, pre, dt) in enumerate([
        (2, 32, 32, 10, 600, 8, 8, 1, RELU, BF16), (2, 32, 32, 9, 300, 8, 8, 1, L.PRE_NONE, F32),
        (2, 32, 64, 1, 3001, 1, 16, 2, RELU, BF16), (2, 32, 32, 1, 1001, 1, 16, 2, L.PRE_NONE, F32),
        (2, 64, 64, 3, 700, 1, 8, 1, L.PRE_NONE, BF16), (2, 64, 32, 2, 555, 1, 8, 1, RELU, BF16),
        (2, 32, 64, 1, 601, 1, 16, 2, L.PRE_NONE, BF16)]):
    rowconv(f"gpu_p1_rowconv_{i}", n, cin, cout, h, w, kh, kw, sw, dt=dt, pre=pre)
# padded backward-data (dY padded by 7 against the flipped weights) and the stride-2 parity dgrad
add("gpu_p1_padded_dgrad", conv(KC, 2, 5, 393, 32, 8, 8, ph=7, pw=7), mat(KC, 32, 2048), 2 * 12 * 400, 32, 2048)
add("gpu_p1_parity_dgrad", conv(KC, 2, 1, 143, 64, 1, 8, pw=7, ow=151), mat(KC, 32, 512), 2 * 151, 32, 512)
for i, (n, cin, cout, h, w, kh, kw, sw, pre, dt) in enumerate([
        (2, 32, 32, 12, 700, 8, 8, 1, RELU, BF16), (2, 32, 64, 1, 3001, 1, 16, 2, RELU, BF16),
        (3, 32, 64, 4, 300, 1, 4, 1, RELU, BF16), (3, 64, 64, 4, 300, 1, 4, 1, L.PRE_NONE, BF16),
        (2, 32, 32, 9, 333, 8, 8, 1, L.PRE_NONE, F32), (2, 32, 32, 1, 901, 1, 16, 2, L.PRE_NONE, BF16),
        (2, 32, 32, 12, 300, 8, 8, 1, RELU, BF16), (70, 32, 32, 20, 400, 8, 8, 1, RELU, BF16)]):
    rowwgrad(f"gpu_p2_rowwgrad_{i}", n, cin, cout, h, w, kh, kw, sw, dt=dt, pre=pre)


def conv1_view(layout, n, T, dt=F32):
    """The frontend conv1 (1x64, stride 2 over the waveform) as the stride-1 pair view: c = 2, kw = 32."""
    return conv(layout, n, 1, T // 2, 2, 1, 32, dt=dt, row=True)


def conv3_view(layout, n, H, W, dt=BF16, kh=8, kw=8):
    return conv(layout, n, H, W, 1, kh, kw, dt=dt, row=True)


def tapwgrad(name, Bo, dydt=BF16, split=2, M=32, N=64, **kw):
    P = Bo.n * Bo.oh * Bo.ow
    add(name, mat(RC, M, P, dydt, **kw), Bo, M, N, P, BF16, split)


def tapconv(name, A, split=1, N=32, Kd=64, **kw):
    add(name, A, mat(KC, N, Kd, **kw), A.n * A.oh * A.ow, N, Kd, BF16, split)


T1 = 2 * 3001 + 64
for dn, dt in (("bf16", BF16), ("f32", F32)):
    tapwgrad(f"gpu_p3_conv1_dy_{dn}", conv1_view(RC, 3, T1), dt)
    tapconv(f"gpu_p4_conv3_x_{dn}", conv3_view(KC, 2, 20, 700, dt))
    for dn2, dt2 in (("bf16", BF16), ("f32", F32)):
        tapwgrad(f"gpu_p3_conv3_x_{dn}_dy_{dn2}", conv3_view(RC, 2, 20, 600, dt), dt2)
tapconv("gpu_p4_conv1", conv1_view(KC, 3, T1))

# ---------------------------------------------------------------- dense 128x128 (path 5): both sides of each condition
gemm("d128_k64", 128, 128, 64)
gemm("d128_k32", 128, 128, 32)
gemm("d128_k96", 128, 128, 96)
gemm("d128_k128", 128, 128, 128)
gemm("d128_m63", 63, 128, 128)
gemm("d128_m64", 64, 128, 128)
gemm("d128_n63", 128, 63, 128)
gemm("d128_n64", 128, 64, 128)
gemm("d128_ld_pad4", 128, 128, 128, pad=4)
gemm("d128_ld_pad8", 128, 128, 128, pad=8)
add("d128_a_misaligned", mat(KC, 128, 128, ptr=PTR + 8), mat(KC, 128, 128), 128, 128, 128)
add("d128_b_misaligned", mat(KC, 128, 128), mat(KC, 128, 128, ptr=PTR + 8), 128, 128, 128)
gemm("d128_rc_m68", 68, 128, 128, RC, KC)
gemm("d128_rc_m72", 72, 128, 128, RC, KC)
gemm("d128_rc_n68", 128, 68, 128, KC, RC)
gemm("d128_rc_n72", 128, 72, 128, KC, RC)
gemm("d128_kc_m68", 68, 68, 128)
gemm("d128_f32_compute", 128, 128, 128, cd=F32)
gemm("d128_f32_storage", 128, 128, 128, dt=F32)
add("d128_a_f32_b_bf16", mat(KC, 128, 128, F32), mat(KC, 128, 128), 128, 128, 128)
add("d128_a_pre_gelu", mat(KC, 128, 128, pre=L.PRE_GELU), mat(KC, 128, 128), 128, 128, 128)
add("d128_b_pre_affine", mat(KC, 128, 128), mat(KC, 128, 128, pre=L.PRE_AFFINE), 128, 128, 128)
add("d128_a_cols_short", mat(KC, 128, 64), mat(KC, 128, 128), 128, 128, 128)
add("d128_a_cols_long", mat(KC, 128, 192), mat(KC, 128, 128), 128, 128, 128)
add("d128_a_rows_not_m", mat(KC, 136, 128), mat(KC, 128, 128), 128, 128, 128)
add("d128_b_rc_rows_short", mat(KC, 128, 128), mat(RC, 128, 64), 128, 128, 128)
gemm("d128_split2", 128, 128, 256, split=2)
gemm("d128_split0", 128, 128, 256, split=0)

# ---------------------------------------------------------------- dense 256x256 (path 7)
gemm("d256_m255_k16384", 255, 256, 16384)
gemm("d256_m256_k16384", 256, 256, 16384)
gemm("d256_n252_k16384", 256, 252, 16384)
gemm("d256_n256_k16384_rr", 256, 256, 16384, RC, RC)
gemm("d256_tiles32_k128", 2048, 1024, 128)
gemm("d256_tiles28_k128", 1792, 1024, 128)
gemm("d256_tiles31_k128", 7681, 256, 128)
gemm("d256_tiles28_k16384", 1792, 1024, 16384)
gemm("d256_tiles28_k16320", 1792, 1024, 16320)
gemm("d256_n1026", 2048, 1026, 128)
gemm("d256_n1028", 2048, 1028, 128)
gemm("d256_n1028_f32_out", 2048, 1028, 128, E=epi(1028, F32))
gemm("d256_n1032", 2048, 1032, 128)
gemm("d256_n1028_rc", 2048, 1028, 128, KC, RC)
gemm("d256_f32_compute", 2048, 1024, 128, cd=F32)
gemm("d256_f32_storage", 2048, 1024, 128, dt=F32)
gemm("d256_k64", 2048, 1024, 64)
gemm("d256_k32", 2048, 1024, 32)
gemm("d256_k96_kc", 2048, 1024, 96)
gemm("d256_k96_rr", 2048, 1024, 96, RC, RC)
gemm("d256_rc_m2052", 2052, 1024, 128, RC, KC)
gemm("d256_rc_m2056", 2056, 1024, 128, RC, KC)
gemm("d256_ld_pad4", 2048, 1024, 128, pad=4)
gemm("d256_ld_pad8", 2048, 1024, 128, pad=8)
add("d256_a_misaligned", mat(KC, 2048, 128, ptr=PTR + 8), mat(KC, 1024, 128), 2048, 1024, 128)
add("d256_a_pre_gelu", mat(KC, 2048, 128, pre=L.PRE_GELU), mat(KC, 1024, 128), 2048, 1024, 128)
gemm("d256_split4_ignored", 2048, 1024, 4096, split=4)
gemm("d256_ldc_pad2", 2048, 1024, 128, E=epi(1024, pad=2))
gemm("d256_ldc_pad4", 2048, 1024, 128, E=epi(1024, pad=4))

# ---------------------------------------------------------------- row-window conv (1) and weight gradient (2)
for c in (16, 32, 64):
    rowconv(f"rc_c{c}", 2, c, 32, 3, 300, 1, 8)
    rowwgrad(f"rw_c{c}", 2, c, 32, 3, 300, 1, 8)
rowconv("rc_c64_s2", 2, 64, 32, 1, 601, 1, 16, sw=2)
rowwgrad("rw_c64_s2", 2, 64, 32, 1, 601, 1, 16, sw=2)
for kw, sw in [(4, 1), (8, 1), (12, 1), (16, 2), (20, 2), (12, 2)]:
    rowconv(f"rc_kw{kw}_s{sw}", 2, 32, 32, 2, 400, 1, kw, sw=sw)
    rowwgrad(f"rw_kw{kw}_s{sw}", 2, 32, 32, 2, 400, 1, kw, sw=sw)
rowconv("rc_kwc64", 2, 32, 32, 2, 400, 1, 2)
rowwgrad("rw_kwc64", 2, 32, 32, 2, 400, 1, 2)
rowconv("rc_kwc192_c64", 2, 64, 32, 2, 400, 1, 3)
rowwgrad("rw_kwc192_c64", 2, 64, 32, 2, 400, 1, 3)
for co in (16, 32, 48, 64, 128):
    rowconv(f"rc_n{co}", 2, 32, co, 2, 400, 1, 8)
    rowwgrad(f"rw_m{co}", 2, 32, co, 2, 400, 1, 8)
for split in (0, 1, 2, 3):
    rowconv(f"rc_split{split}", 2, 32, 32, 9, 300, 8, 8, split=split)
    rowwgrad(f"rw_split{split}", 2, 32, 32, 9, 300, 8, 8, split=split)
rowconv("rc_sw3", 2, 32, 32, 2, 400, 1, 8, sw=3)
rowwgrad("rw_sw3", 2, 32, 32, 2, 400, 1, 8, sw=3)
rowconv("rc_sh2", 2, 32, 32, 9, 300, 1, 8, sh=2)
rowwgrad("rw_sh2", 2, 32, 32, 9, 300, 1, 8, sh=2)
for pn, pre in (("affine", L.PRE_AFFINE), ("relu", RELU), ("gelu", L.PRE_GELU)):
    rowconv(f"rc_pre_{pn}", 2, 32, 32, 2, 400, 1, 8, pre=pre)
    rowwgrad(f"rw_pre_{pn}", 2, 32, 32, 2, 400, 1, 8, pre=pre)
rowconv("rc_f32_compute", 2, 32, 32, 2, 400, 1, 8, cd=F32)
rowwgrad("rw_f32_compute", 2, 32, 32, 2, 400, 1, 8, cd=F32)
rowconv("rc_x_misaligned", 2, 32, 32, 2, 400, 1, 8, ptr=PTR + 8)
rowconv("rc_w_misaligned", 2, 32, 32, 2, 400, 1, 8, wptr=PTR + 8)
rowconv("rc_w_ld_pad4", 2, 32, 32, 2, 400, 1, 8, wpad=4)
rowconv("rc_w_ld_pad8", 2, 32, 32, 2, 400, 1, 8, wpad=8)
add("rc_w_f32", conv(KC, 2, 2, 400, 32, 1, 8), mat(KC, 32, 256, F32), 2 * 2 * 393, 32, 256)
add("rc_a_rc_layout", conv(RC, 2, 2, 400, 32, 1, 8), mat(KC, 32, 256), 2 * 2 * 393, 32, 256)
add("rc_m_not_pixels", conv(KC, 2, 2, 400, 32, 1, 8), mat(KC, 32, 256), 2 * 2 * 393 - 1, 32, 256)
add("rc_k_not_taps", conv(KC, 2, 2, 400, 32, 1, 8), mat(KC, 32, 512), 2 * 2 * 393, 32, 512)
rowwgrad("rw_x_misaligned", 2, 32, 32, 2, 400, 1, 8, ptr=PTR + 8)
rowwgrad("rw_dy_misaligned", 2, 32, 32, 2, 400, 1, 8, dyptr=PTR + 8)
rowwgrad("rw_dy_ld_pad8", 2, 32, 32, 2, 400, 1, 8, dypad=8)
rowwgrad("rw_dy_f32_x_bf16", 2, 32, 32, 2, 400, 1, 8, dydt=F32)
rowwgrad("rw_f32_storage", 2, 32, 32, 2, 400, 1, 8, dt=F32)
add("rw_b_kc_layout", mat(RC, 32, 1572), conv(KC, 2, 2, 400, 32, 1, 8), 32, 256, 1572, BF16, 2)
add("rw_a_kc_layout", mat(KC, 32, 1572), conv(RC, 2, 2, 400, 32, 1, 8), 32, 256, 1572, BF16, 2)
add("rw_k_not_pixels", mat(RC, 32, 1571), conv(RC, 2, 2, 400, 32, 1, 8), 32, 256, 1571, BF16, 2)
# the rolling-window 8x8 special case (reported as 2) and its neighbours (the plain row-window kernel, also 2)
rowwgrad("rw_wgrad8", 2, 32, 32, 12, 300, 8, 8, pre=RELU)
rowwgrad("rw_wgrad8_pre_none", 2, 32, 32, 12, 300, 8, 8)
rowwgrad("rw_wgrad8_pre_affine", 2, 32, 32, 12, 300, 8, 8, pre=L.PRE_AFFINE)
rowwgrad("rw_wgrad8_f32", 2, 32, 32, 12, 300, 8, 8, pre=RELU, dt=F32)
rowwgrad("rw_wgrad8_m64", 2, 32, 64, 12, 300, 8, 8, pre=RELU)
rowwgrad("rw_wgrad8_padded", 2, 32, 32, 12, 300, 8, 8, pre=RELU, ph=1, pw=1)
rowwgrad("rw_wgrad8_kh4", 2, 32, 32, 12, 300, 4, 8, pre=RELU)
rowwgrad("rw_wgrad8_split300", 2, 32, 32, 12, 300, 8, 8, pre=RELU, split=300)

# ---------------------------------------------------------------- single-channel tap conv (4) and weight gradient (3)
for split in (0, 1, 2, 3):
    tapconv(f"tc_conv1_split{split}", conv1_view(KC, 2, 4000), split=split)
    tapconv(f"tc_conv3_split{split}", conv3_view(KC, 2, 12, 300), split=split)
    tapwgrad(f"tw_conv1_split{split}", conv1_view(RC, 2, 4000), split=split)
    tapwgrad(f"tw_conv3_split{split}", conv3_view(RC, 2, 12, 300), split=split)
tapconv("tc_conv1_bf16_input", conv1_view(KC, 2, 4000, BF16))
tapwgrad("tw_conv1_bf16_input", conv1_view(RC, 2, 4000, BF16))
tapconv("tc_conv3_f32_input", conv3_view(KC, 2, 12, 300, F32))
tapwgrad("tw_conv3_f32_input", conv3_view(RC, 2, 12, 300, F32))
tapwgrad("tw_conv3_dy_f32", conv3_view(RC, 2, 12, 300), F32)
tapconv("tc_conv3_4x16", conv3_view(KC, 2, 12, 300, kh=4, kw=16))
tapwgrad("tw_conv3_4x16", conv3_view(RC, 2, 12, 300, kh=4, kw=16))
tapconv("tc_conv1_two_rows", conv(KC, 2, 2, 2000, 2, 1, 32, dt=F32, row=True))
tapwgrad("tw_conv1_two_rows", conv(RC, 2, 2, 2000, 2, 1, 32, dt=F32, row=True))
tapconv("tc_conv3_not_rowkind", conv(KC, 2, 12, 300, 8, 1, 8))
tapconv("tc_conv3_sw2", conv(KC, 2, 12, 300, 1, 8, 8, sw=2, row=True))
tapwgrad("tw_conv3_sw2", conv(RC, 2, 12, 300, 1, 8, 8, sw=2, row=True))
tapconv("tc_conv3_ph1", conv(KC, 2, 12, 300, 1, 8, 8, ph=1, row=True))
tapwgrad("tw_conv3_ph1", conv(RC, 2, 12, 300, 1, 8, 8, ph=1, row=True))
tapconv("tc_n64", conv3_view(KC, 2, 12, 300), N=64)
tapconv("tc_w_misaligned", conv3_view(KC, 2, 12, 300), ptr=PTR + 8)
tapconv("tc_w_ld_pad8", conv3_view(KC, 2, 12, 300), pad=8)
add("tc_w_f32", conv3_view(KC, 2, 12, 300), mat(KC, 32, 64, F32), 2 * 5 * 293, 32, 64)
add("tc_a_rc_layout", conv3_view(RC, 2, 12, 300), mat(KC, 32, 64), 2 * 5 * 293, 32, 64)
add("tc_m_not_pixels", conv3_view(KC, 2, 12, 300), mat(KC, 32, 64), 2 * 5 * 293 + 1, 32, 64)
add("tc_f32_compute", conv3_view(KC, 2, 12, 300), mat(KC, 32, 64), 2 * 5 * 293, 32, 64, F32)
tapwgrad("tw_m64", conv3_view(RC, 2, 12, 300), M=64)
tapwgrad("tw_dy_misaligned", conv3_view(RC, 2, 12, 300), ptr=PTR + 8)
tapwgrad("tw_dy_ld_pad8", conv3_view(RC, 2, 12, 300), pad=8)
add("tw_b_kc_layout", mat(RC, 32, 2930), conv3_view(KC, 2, 12, 300), 32, 64, 2930, BF16, 2)
add("tw_k_not_pixels", mat(RC, 32, 2931), conv3_view(RC, 2, 12, 300), 32, 64, 2931, BF16, 2)
add("tw_f32_compute", mat(RC, 32, 2930), conv3_view(RC, 2, 12, 300), 32, 64, 2930, F32, 2)

# ---------------------------------------------------------------- workspace sizes: split-K slabs, colsum, a_colsum
for pn, (M, N, Kd) in {"p0": (37, 50, 200), "p5": (296, 200, 192), "p7": (2056, 1024, 128),
                       "p7_long_k": (264, 264, 16384 + 64), "p7_wgrad": (768, 2304, 69632 + 100)}.items():
    for split in (1, 4):
        gemm(f"ws_{pn}_plain_f32_s{split}", M, N, Kd, RC, RC, split=split, E=epi(N, F32))
        gemm(f"ws_{pn}_colsum_s{split}", M, N, Kd, RC, RC, split=split, E=epi(N, colsum=True))
        gemm(f"ws_{pn}_a_colsum_s{split}", M, N, Kd, RC, RC, split=split, E=epi(N, F32, a_colsum=True))
        gemm(f"ws_{pn}_both_colsums_s{split}", M, N, Kd, RC, RC, split=split,
             E=epi(N, F32, colsum=True, a_colsum=True))
    # a column sum the 256x256 kernel fuses (behind DACT_MUL); a plain output's column sum leaves that kernel
    gemm(f"ws_{pn}_dact_mul_colsum", M, N, Kd, RC, RC, E=epi(N, colsum=True, act=L.DACT_MUL))
    gemm(f"ws_{pn}_a_colsum_kc_a", M - M % 8, N, Kd - Kd % 64, KC, RC, E=epi(N, F32, a_colsum=True))
rowwgrad("ws_rowwgrad_split16", 2, 32, 64, 1, 3001, 1, 16, sw=2, split=16)
rowwgrad("ws_wgrad8_split16", 2, 32, 32, 12, 300, 8, 8, pre=RELU, split=16)
tapwgrad("ws_tapwgrad_split16", conv3_view(RC, 2, 12, 300), split=16)


# Recorded from the library as it was before the selector existed (see the module docstring).
EXPECTED = {
    "gpu_p0_37x50x200_kk_s1": (0, 0),
    "gpu_p0_37x50x200_kk_s3": (0, 22200),
    "gpu_p0_130x70x8_kk_s1": (0, 0),
    "gpu_p0_130x70x8_kk_s3": (0, 109200),
    "gpu_p0_300x32x64_kk_s1": (0, 0),
    "gpu_p0_300x32x64_kk_s3": (0, 115200),
    "gpu_p0_64x600x40_kk_s1": (0, 0),
    "gpu_p0_64x600x40_kk_s3": (0, 460800),
    "gpu_p0_256x128x96_kk_s1": (0, 0),
    "gpu_p0_256x128x96_kk_s3": (0, 393216),
    "gpu_p5_64x72x64_kk_s1": (5, 0),
    "gpu_p5_296x200x192_kk_s1": (5, 0),
    "gpu_p5_256x384x4096_kk_s4": (5, 1572864),
    "gpu_p5_256x256x128_kk_s1": (5, 0),
    "gpu_p5_128x1000x512_kk_s1": (5, 0),
    "gpu_p7_4096x768x768_kk": (7, 0),
    "gpu_p7_4136x2304x512_kk": (7, 0),
    "gpu_p7_8192x264x3072_kk": (7, 0),
    "gpu_p7_8200x520x1024_kk": (7, 0),
    "gpu_p0_37x50x200_kr_s1": (0, 0),
    "gpu_p0_37x50x200_kr_s3": (0, 22200),
    "gpu_p0_130x70x8_kr_s1": (0, 0),
    "gpu_p0_130x70x8_kr_s3": (0, 109200),
    "gpu_p0_300x32x64_kr_s1": (0, 0),
    "gpu_p0_300x32x64_kr_s3": (0, 115200),
    "gpu_p0_64x600x40_kr_s1": (0, 0),
    "gpu_p0_64x600x40_kr_s3": (0, 460800),
    "gpu_p0_256x128x96_kr_s1": (0, 0),
    "gpu_p0_256x128x96_kr_s3": (0, 393216),
    "gpu_p5_64x72x64_kr_s1": (5, 0),
    "gpu_p5_296x200x192_kr_s1": (5, 0),
    "gpu_p5_256x384x4096_kr_s4": (5, 1572864),
    "gpu_p5_256x256x128_kr_s1": (5, 0),
    "gpu_p5_128x1000x512_kr_s1": (5, 0),
    "gpu_p7_4096x768x768_kr": (7, 0),
    "gpu_p7_4136x2304x512_kr": (7, 0),
    "gpu_p7_8192x264x3072_kr": (7, 0),
    "gpu_p7_8200x520x1024_kr": (7, 0),
    "gpu_p0_37x50x200_rk_s1": (0, 0),
    "gpu_p0_37x50x200_rk_s3": (0, 22200),
    "gpu_p0_130x70x8_rk_s1": (0, 0),
    "gpu_p0_130x70x8_rk_s3": (0, 109200),
    "gpu_p0_300x32x64_rk_s1": (0, 0),
    "gpu_p0_300x32x64_rk_s3": (0, 115200),
    "gpu_p0_64x600x40_rk_s1": (0, 0),
    "gpu_p0_64x600x40_rk_s3": (0, 460800),
    "gpu_p0_256x128x96_rk_s1": (0, 0),
    "gpu_p0_256x128x96_rk_s3": (0, 393216),
    "gpu_p5_64x72x64_rk_s1": (5, 0),
    "gpu_p5_296x200x192_rk_s1": (5, 0),
    "gpu_p5_256x384x4096_rk_s4": (5, 1572864),
    "gpu_p5_256x256x128_rk_s1": (5, 0),
    "gpu_p5_128x1000x512_rk_s1": (5, 0),
    "gpu_p7_4096x768x768_rk": (7, 0),
    "gpu_p7_4136x2304x512_rk": (7, 0),
    "gpu_p7_8192x264x3072_rk": (7, 0),
    "gpu_p7_8200x520x1024_rk": (7, 0),
    "gpu_p0_37x50x200_rr_s1": (0, 0),
    "gpu_p0_37x50x200_rr_s3": (0, 22200),
    "gpu_p0_130x70x8_rr_s1": (0, 0),
    "gpu_p0_130x70x8_rr_s3": (0, 109200),
    "gpu_p0_300x32x64_rr_s1": (0, 0),
    "gpu_p0_300x32x64_rr_s3": (0, 115200),
    "gpu_p0_64x600x40_rr_s1": (0, 0),
    "gpu_p0_64x600x40_rr_s3": (0, 460800),
    "gpu_p0_256x128x96_rr_s1": (0, 0),
    "gpu_p0_256x128x96_rr_s3": (0, 393216),
    "gpu_p5_64x72x64_rr_s1": (5, 0),
    "gpu_p5_296x200x192_rr_s1": (5, 0),
    "gpu_p5_256x384x4096_rr_s4": (5, 1572864),
    "gpu_p5_256x256x128_rr_s1": (5, 0),
    "gpu_p5_128x1000x512_rr_s1": (5, 0),
    "gpu_p7_4096x768x768_rr": (7, 0),
    "gpu_p7_4136x2304x512_rr": (7, 0),
    "gpu_p7_8192x264x3072_rr": (7, 0),
    "gpu_p7_8200x520x1024_rr": (7, 0),
    "gpu_p5_padded_ld_kr": (5, 0),
    "gpu_p5_padded_ld_rk": (5, 0),
    "gpu_p0_f32_compute": (0, 0),
    "gpu_p0_bf16_small": (0, 0),
    "gpu_p0_staged_f32_storage": (0, 0),
    "gpu_p5_trunk_w2_overlapping_rows": (5, 0),
    "gpu_p7_smallest_grid": (7, 0),
    "gpu_p7_ragged_n_1028": (5, 0),
    "gpu_p7_ragged_n_260": (5, 0),
    "gpu_p7_long_k_16448": (7, 4460544),
    "gpu_p7_long_k_16456": (7, 4460544),
    "gpu_p7_wgrad_768x2304x69732": (7, 63700992),
    "gpu_p7_wgrad_2304x768x16384": (7, 63700992),
    "gpu_p7_wgrad_768x768x52640": (7, 66060288),
    "gpu_a_colsum_2304x768x16424_rr": (7, 63783936),
    "gpu_a_colsum_2304x768x16384_rk": (7, 63783936),
    "gpu_a_colsum_776x768x52640_rr": (7, 50126592),
    "gpu_a_colsum_776x768x52608_rk": (7, 50126592),
    "gpu_a_colsum_520x264x300_rr": (0, 2129920),
    "gpu_a_colsum_520x264x256_rk": (5, 2129920),
    "gpu_colsum_p5_900x640x256": (5, 2621440),
    "gpu_colsum_p7_8229x3072x768": (7, 12582912),
    "gpu_p1_rowconv_0": (1, 0),
    "gpu_p1_rowconv_1": (1, 0),
    "gpu_p1_rowconv_2": (1, 0),
    "gpu_p1_rowconv_3": (1, 0),
    "gpu_p1_rowconv_4": (1, 0),
    "gpu_p1_rowconv_5": (1, 0),
    "gpu_p1_rowconv_6": (1, 0),
    "gpu_p1_padded_dgrad": (1, 0),
    "gpu_p1_parity_dgrad": (1, 0),
    "gpu_p2_rowwgrad_0": (2, 524288),
    "gpu_p2_rowwgrad_1": (2, 262144),
    "gpu_p2_rowwgrad_2": (2, 65536),
    "gpu_p2_rowwgrad_3": (2, 131072),
    "gpu_p2_rowwgrad_4": (2, 524288),
    "gpu_p2_rowwgrad_5": (2, 131072),
    "gpu_p2_rowwgrad_6": (2, 524288),
    "gpu_p2_rowwgrad_7": (2, 524288),
    "gpu_p3_conv1_dy_bf16": (3, 16384),
    "gpu_p4_conv3_x_bf16": (4, 0),
    "gpu_p3_conv3_x_bf16_dy_bf16": (3, 16384),
    "gpu_p3_conv3_x_bf16_dy_f32": (3, 16384),
    "gpu_p3_conv1_dy_f32": (3, 16384),
    "gpu_p4_conv3_x_f32": (4, 0),
    "gpu_p3_conv3_x_f32_dy_bf16": (3, 16384),
    "gpu_p3_conv3_x_f32_dy_f32": (3, 16384),
    "gpu_p4_conv1": (4, 0),
    "d128_k64": (5, 0),
    "d128_k32": (0, 0),
    "d128_k96": (0, 0),
    "d128_k128": (5, 0),
    "d128_m63": (0, 0),
    "d128_m64": (5, 0),
    "d128_n63": (0, 0),
    "d128_n64": (5, 0),
    "d128_ld_pad4": (0, 0),
    "d128_ld_pad8": (5, 0),
    "d128_a_misaligned": (0, 0),
    "d128_b_misaligned": (0, 0),
    "d128_rc_m68": (0, 0),
    "d128_rc_m72": (5, 0),
    "d128_rc_n68": (0, 0),
    "d128_rc_n72": (5, 0),
    "d128_kc_m68": (5, 0),
    "d128_f32_compute": (0, 0),
    "d128_f32_storage": (0, 0),
    "d128_a_f32_b_bf16": (0, 0),
    "d128_a_pre_gelu": (0, 0),
    "d128_b_pre_affine": (0, 0),
    "d128_a_cols_short": (0, 0),
    "d128_a_cols_long": (5, 0),
    "d128_a_rows_not_m": (0, 0),
    "d128_b_rc_rows_short": (0, 0),
    "d128_split2": (5, 131072),
    "d128_split0": (5, 0),
    "d256_m255_k16384": (5, 0),
    "d256_m256_k16384": (7, 4194304),
    "d256_n252_k16384": (5, 0),
    "d256_n256_k16384_rr": (7, 4194304),
    "d256_tiles32_k128": (7, 0),
    "d256_tiles28_k128": (5, 0),
    "d256_tiles31_k128": (5, 0),
    "d256_tiles28_k16384": (7, 66060288),
    "d256_tiles28_k16320": (5, 0),
    "d256_n1026": (5, 0),
    "d256_n1028": (5, 0),
    "d256_n1028_f32_out": (5, 0),
    "d256_n1032": (7, 0),
    "d256_n1028_rc": (0, 0),
    "d256_f32_compute": (0, 0),
    "d256_f32_storage": (0, 0),
    "d256_k64": (7, 0),
    "d256_k32": (0, 0),
    "d256_k96_kc": (0, 0),
    "d256_k96_rr": (7, 0),
    "d256_rc_m2052": (0, 0),
    "d256_rc_m2056": (7, 0),
    "d256_ld_pad4": (0, 0),
    "d256_ld_pad8": (7, 0),
    "d256_a_misaligned": (0, 0),
    "d256_a_pre_gelu": (0, 0),
    "d256_split4_ignored": (7, 33554432),
    "d256_ldc_pad2": (7, 0),
    "d256_ldc_pad4": (7, 0),
    "rc_c16": (0, 0),
    "rw_c16": (0, 32768),
    "rc_c32": (1, 0),
    "rw_c32": (2, 65536),
    "rc_c64": (1, 0),
    "rw_c64": (2, 131072),
    "rc_c64_s2": (0, 0),
    "rw_c64_s2": (0, 262144),
    "rc_kw4_s1": (1, 0),
    "rw_kw4_s1": (2, 32768),
    "rc_kw8_s1": (1, 0),
    "rw_kw8_s1": (2, 65536),
    "rc_kw12_s1": (0, 0),
    "rw_kw12_s1": (0, 98304),
    "rc_kw16_s2": (1, 0),
    "rw_kw16_s2": (2, 131072),
    "rc_kw20_s2": (0, 0),
    "rw_kw20_s2": (0, 163840),
    "rc_kw12_s2": (1, 0),
    "rw_kw12_s2": (2, 98304),
    "rc_kwc64": (0, 0),
    "rw_kwc64": (0, 16384),
    "rc_kwc192_c64": (0, 0),
    "rw_kwc192_c64": (0, 49152),
    "rc_n16": (0, 0),
    "rw_m16": (0, 32768),
    "rc_n32": (1, 0),
    "rw_m32": (2, 65536),
    "rc_n48": (0, 0),
    "rw_m48": (0, 98304),
    "rc_n64": (1, 0),
    "rw_m64": (2, 131072),
    "rc_n128": (0, 0),
    "rw_m128": (0, 262144),
    "rc_split0": (1, 0),
    "rw_split0": (0, 0),
    "rc_split1": (1, 0),
    "rw_split1": (0, 0),
    "rc_split2": (0, 300032),
    "rw_split2": (2, 524288),
    "rc_split3": (0, 450048),
    "rw_split3": (2, 786432),
    "rc_sw3": (0, 0),
    "rw_sw3": (0, 65536),
    "rc_sh2": (0, 0),
    "rw_sh2": (0, 65536),
    "rc_pre_affine": (1, 0),
    "rw_pre_affine": (2, 65536),
    "rc_pre_relu": (1, 0),
    "rw_pre_relu": (2, 65536),
    "rc_pre_gelu": (0, 0),
    "rw_pre_gelu": (0, 65536),
    "rc_f32_compute": (0, 0),
    "rw_f32_compute": (0, 65536),
    "rc_x_misaligned": (0, 0),
    "rc_w_misaligned": (0, 0),
    "rc_w_ld_pad4": (0, 0),
    "rc_w_ld_pad8": (1, 0),
    "rc_w_f32": (0, 0),
    "rc_a_rc_layout": (0, 0),
    "rc_m_not_pixels": (0, 0),
    "rc_k_not_taps": (0, 0),
    "rw_x_misaligned": (0, 65536),
    "rw_dy_misaligned": (0, 65536),
    "rw_dy_ld_pad8": (0, 65536),
    "rw_dy_f32_x_bf16": (0, 65536),
    "rw_f32_storage": (2, 65536),
    "rw_b_kc_layout": (0, 65536),
    "rw_a_kc_layout": (0, 65536),
    "rw_k_not_pixels": (0, 65536),
    "rw_wgrad8": (2, 524288),
    "rw_wgrad8_pre_none": (2, 524288),
    "rw_wgrad8_pre_affine": (2, 524288),
    "rw_wgrad8_f32": (2, 524288),
    "rw_wgrad8_m64": (2, 1048576),
    "rw_wgrad8_padded": (2, 524288),
    "rw_wgrad8_kh4": (2, 262144),
    "rw_wgrad8_split300": (2, 78643200),
    "tc_conv1_split0": (4, 0),
    "tc_conv3_split0": (4, 0),
    "tw_conv1_split0": (0, 0),
    "tw_conv3_split0": (0, 0),
    "tc_conv1_split1": (4, 0),
    "tc_conv3_split1": (4, 0),
    "tw_conv1_split1": (0, 0),
    "tw_conv3_split1": (0, 0),
    "tc_conv1_split2": (0, 1008128),
    "tc_conv3_split2": (0, 750080),
    "tw_conv1_split2": (3, 16384),
    "tw_conv3_split2": (3, 16384),
    "tc_conv1_split3": (0, 1512192),
    "tc_conv3_split3": (0, 1125120),
    "tw_conv1_split3": (3, 24576),
    "tw_conv3_split3": (3, 24576),
    "tc_conv1_bf16_input": (0, 0),
    "tw_conv1_bf16_input": (0, 16384),
    "tc_conv3_f32_input": (4, 0),
    "tw_conv3_f32_input": (3, 16384),
    "tw_conv3_dy_f32": (3, 16384),
    "tc_conv3_4x16": (0, 0),
    "tw_conv3_4x16": (0, 16384),
    "tc_conv1_two_rows": (0, 0),
    "tw_conv1_two_rows": (0, 16384),
    "tc_conv3_not_rowkind": (0, 0),
    "tc_conv3_sw2": (0, 0),
    "tw_conv3_sw2": (0, 16384),
    "tc_conv3_ph1": (0, 0),
    "tw_conv3_ph1": (0, 16384),
    "tc_n64": (0, 0),
    "tc_w_misaligned": (0, 0),
    "tc_w_ld_pad8": (0, 0),
    "tc_w_f32": (0, 0),
    "tc_a_rc_layout": (0, 0),
    "tc_m_not_pixels": (0, 0),
    "tc_f32_compute": (0, 0),
    "tw_m64": (0, 32768),
    "tw_dy_misaligned": (0, 16384),
    "tw_dy_ld_pad8": (0, 16384),
    "tw_b_kc_layout": (0, 16384),
    "tw_k_not_pixels": (0, 16384),
    "tw_f32_compute": (0, 16384),
    "ws_p0_plain_f32_s1": (0, 0),
    "ws_p0_colsum_s1": (0, 204800),
    "ws_p0_a_colsum_s1": (0, 151552),
    "ws_p0_both_colsums_s1": (0, 356352),
    "ws_p0_plain_f32_s4": (0, 29600),
    "ws_p0_colsum_s4": (0, 234496),
    "ws_p0_a_colsum_s4": (0, 181248),
    "ws_p0_both_colsums_s4": (0, 386048),
    "ws_p0_dact_mul_colsum": (0, 204800),
    "ws_p0_a_colsum_kc_a": (0, 131072),
    "ws_p5_plain_f32_s1": (5, 0),
    "ws_p5_colsum_s1": (5, 819200),
    "ws_p5_a_colsum_s1": (5, 1212416),
    "ws_p5_both_colsums_s1": (5, 2031616),
    "ws_p5_plain_f32_s4": (5, 947200),
    "ws_p5_colsum_s4": (5, 1766400),
    "ws_p5_a_colsum_s4": (5, 2159616),
    "ws_p5_both_colsums_s4": (5, 2978816),
    "ws_p5_dact_mul_colsum": (5, 819200),
    "ws_p5_a_colsum_kc_a": (5, 1212416),
    "ws_p7_plain_f32_s1": (7, 0),
    "ws_p7_colsum_s1": (7, 4194304),
    "ws_p7_a_colsum_s1": (7, 8448),
    "ws_p7_both_colsums_s1": (7, 12615680),
    "ws_p7_plain_f32_s4": (7, 0),
    "ws_p7_colsum_s4": (7, 37879808),
    "ws_p7_a_colsum_s4": (7, 8448),
    "ws_p7_both_colsums_s4": (7, 46301184),
    "ws_p7_dact_mul_colsum": (7, 167936),
    "ws_p7_a_colsum_kc_a": (7, 8421376),
    "ws_p7_long_k_plain_f32_s1": (7, 4460544),
    "ws_p7_long_k_colsum_s1": (7, 1081344),
    "ws_p7_long_k_a_colsum_s1": (7, 4477440),
    "ws_p7_long_k_both_colsums_s1": (7, 2162688),
    "ws_p7_long_k_plain_f32_s4": (7, 4460544),
    "ws_p7_long_k_colsum_s4": (7, 2196480),
    "ws_p7_long_k_a_colsum_s4": (7, 4477440),
    "ws_p7_long_k_both_colsums_s4": (7, 3277824),
    "ws_p7_long_k_dact_mul_colsum": (7, 4496640),
    "ws_p7_long_k_a_colsum_kc_a": (7, 5541888),
    "ws_p7_wgrad_plain_f32_s1": (7, 63700992),
    "ws_p7_wgrad_colsum_s1": (7, 9437184),
    "ws_p7_wgrad_a_colsum_s1": (7, 63728640),
    "ws_p7_wgrad_both_colsums_s1": (7, 12582912),
    "ws_p7_wgrad_plain_f32_s4": (7, 63700992),
    "ws_p7_wgrad_colsum_s4": (7, 37748736),
    "ws_p7_wgrad_a_colsum_s4": (7, 63728640),
    "ws_p7_wgrad_both_colsums_s4": (7, 40894464),
    "ws_p7_wgrad_dact_mul_colsum": (7, 64023552),
    "ws_p7_wgrad_a_colsum_kc_a": (7, 66846720),
    "ws_rowwgrad_split16": (2, 2097152),
    "ws_wgrad8_split16": (2, 4194304),
    "ws_tapwgrad_split16": (3, 131072),
}


def test_table_and_cases_agree():
    assert set(EXPECTED) == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_dispatch_row(name):
    lib = L.load()
    A, B, E, M, N, Kd, cd, split = CASES[name]
    got = (lib.mia_gemm_path(A, B, M, N, Kd, cd, split), lib.mia_gemm_workspace_bytes_ex(A, B, E, M, N, Kd, cd, split))
    assert got == EXPECTED[name]
