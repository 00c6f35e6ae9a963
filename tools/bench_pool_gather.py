"""Time mia_pool_bwd_gather_ex and mia_pool_bn_relu_bwd_apply_ex at the shapes of an EnvNet B = 256 step (the four
trunk pools and the frontend pool): the MIA_POOL_V1 gather against the default one, gm in f32 against bf16.  Calls go
through ctypes on preallocated buffers, so the host stays ahead of kernels of a few tens of microseconds.
MIAUDIO_LIB selects the library (a build with -DPG_DEPTH=n reads n loop iterations ahead in the gather).
    python tools/bench_pool_gather.py"""
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "dl-sound-classification_amd"))
import torch  # noqa: E402

from src.miaudio import kernels as K  # noqa: E402
from src.miaudio import lib as L  # noqa: E402
from src.models.envnet_hip import TRUNK, TRUNK_POOL, geometry  # noqa: E402

dev = torch.device("cuda:0")
B = 256
geo = geometry(220_500)
#         name, H, W, C, kh, kw, layout of dout
shapes = [("frontend", 1, geo["W2"], 64, 1, 64, 1)]
for blk in range(4):
    (_, _), (_, _), (hb, wb), _ = geo["trunk"][blk]
    shapes.append((f"trunk{blk}", hb, wb, TRUNK[2 * blk + 1][3], *TRUNK_POOL[blk], 2 if blk == 3 else 0))
lib = L.load()
stream = L.stream_ptr()
BF16, F32 = torch.bfloat16, torch.float32


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best * 1e3  # us


print(f"library {L.LIB_PATH}", flush=True)
for name, H, W, C, kh, kw, layout in shapes:
    g = torch.Generator(device=dev).manual_seed(0)
    x = (torch.randn(B, H, W, C, generator=g, device=dev) * 2 + 0.3).to(BF16)
    gamma = torch.randn(C, generator=g, device=dev)
    beta = torch.randn(C, generator=g, device=dev) * 0.5
    bn = K.bn_fwd_stats(x, B * H * W, C, gamma, beta, torch.zeros(C, device=dev), torch.ones(C, device=dev), 0.1, 1e-5,
                        True)
    OH, OW = H // kh, W // kw
    cells = B * OH * OW
    pooled = torch.empty(cells, C, dtype=BF16, device=dev)
    am = torch.empty(cells, C, dtype=torch.uint8, device=dev)
    win = torch.empty(cells, C, dtype=BF16, device=dev)
    K.pool_fwd(x, B, H, W, C, kh, kw, bn, pooled, 0, am, win=win)
    dout = torch.randn(cells * C, generator=g, device=dev).to(BF16)
    dg, db, dbias = (torch.empty(C, device=dev) for _ in range(3))
    dx = torch.empty_like(x)
    ws = torch.empty(lib.mia_bn_partial_bytes(B * H * W, C), dtype=torch.uint8, device=dev)
    gms = {F32: torch.empty(cells, C, dtype=F32, device=dev), BF16: torch.empty(cells, C, dtype=BF16, device=dev)}

    def gather(gdt):
        gm = gms[gdt]
        L.check(lib.mia_pool_bwd_gather_ex(dout.data_ptr(), layout, am.data_ptr(), x.data_ptr(), win.data_ptr(), L.BF16,
                                           B, H, W, C, kh, kw, bn.scale.data_ptr(), bn.shift.data_ptr(),
                                           bn.mean.data_ptr(), bn.invstd.data_ptr(), gm.data_ptr(), L.dtype_code(gm),
                                           dg.data_ptr(), db.data_ptr(), ws.data_ptr(), stream), "gather")

    def apply(gdt):
        gm = gms[gdt]
        L.check(lib.mia_pool_bn_relu_bwd_apply_ex(gm.data_ptr(), L.dtype_code(gm), am.data_ptr(), x.data_ptr(), L.BF16,
                                                  B, H, W, C, kh, kw, gamma.data_ptr(), bn.mean.data_ptr(),
                                                  bn.invstd.data_ptr(), dg.data_ptr(), db.data_ptr(), dx.data_ptr(),
                                                  dbias.data_ptr(), ws.data_ptr(), stream), "apply")

    row = {}
    os.environ["MIA_POOL_V1"] = "1"
    row["gather v1 f32"] = timed(lambda: gather(F32))
    del os.environ["MIA_POOL_V1"]
    for gdt, tag in ((F32, "f32"), (BF16, "bf16")):
        row[f"gather {tag}"] = timed(lambda: gather(gdt))
        row[f"apply {tag}"] = timed(lambda: apply(gdt), reps=10)
    mb = cells * C / 1e6
    print(f"{name:9s} {H}x{W}x{C} ({kh},{kw}) layout {layout}, {mb:.1f} M cell-channels (gather + final, us): "
          + ", ".join(f"{k} {v:.1f}" for k, v in row.items()), flush=True)
    del x, dx, pooled, am, win, dout, gms
