"""GPU: three kernels on csrc/bn_math.h run the same ReLU+BN backward reduce step, bit for bit.

bn_relu_bwd_reduce_kernel (norm.hip), pool_bwd_sparse_ra_kernel (pool.hip: mia_pool_bwd_gather with a (1, 1) window,
NHWC dout and the winners saved, win = x) and lt_pool_bwd_gather_kernel (leaftrunk.hip, mean = False, win = x) all
form g = relu'(bn(x)) d, sum g and sum g xhat per channel through BnRed8::step and fold them through cp_fold<2>.
Where their launch geometries coincide the results must be `torch.equal`: each shape below is ONE block in all three
launchers and gives a thread at most one row, so every thread's sums are a single step from 0 and the fold adds
the same values in the same slot order.  With rslots = 256 / (C / 8) row slots:
  norm       nb = max(1, ceil(P / (8 rslots)))       thread rs walks rows rs, rs + rslots, ..
  pool       nb = max(1, ceil(cells / (2 rslots)))   cells = P under the (1, 1) window
  leaftrunk  nb = max(1, ceil(cells / (2 rslots)))
so P <= rslots gives one block and at most one row per thread in each.
"""
import pytest
import torch

from src.miaudio import kernels as K

pytestmark = pytest.mark.gpu

#        C    P
CASES = [(64, 24),   # rslots = 32: some row slots empty
         (32, 64),   # rslots = 64: one row in every slot
         (256, 5)]   # rslots = 8: fewer rows than slots


@pytest.mark.parametrize("c,p", CASES)
def test_reduce_step_same_bits_in_norm_pool_and_leaftrunk(c, p, monkeypatch):
    for name in ("MIA_POOL_V1", "MIA_POOL_GRID", "MIA_POOL_GM32"):  # the default form of the gather, full grid
        monkeypatch.delenv(name, raising=False)
    rslots = 256 // (c // 8)
    assert p <= rslots  # one block, at most one row per thread (module docstring)
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * c + p)
    x = torch.randn(p, c, generator=g).to(torch.bfloat16).to(dev)
    d = torch.randn(p, c, generator=g).to(torch.bfloat16).to(dev)
    # (mean, invstd, scale, shift), scales of both signs so that the mask follows either side of x
    st = K.BNState((torch.randn(c, generator=g) * 0.1).to(dev), (torch.rand(c, generator=g) + 0.5).to(dev),
                   ((torch.rand(c, generator=g) - 0.3) * 1.5).to(dev), (torch.randn(c, generator=g) * 0.3).to(dev))

    dz = torch.full_like(d, float("nan"))
    dg_n, db_n = K.bn_relu_bwd_reduce(d, dz, x, p, c, st)
    dg_n, db_n = dg_n.clone(), db_n.clone()

    am = torch.zeros(p, c, dtype=torch.uint8, device=dev)  # a (1, 1) window: position 0 everywhere
    gm_p, dg_p, db_p = K.pool_bwd_gather(d, 0, am, x, 1, 1, p, c, 1, 1, st, win=x)
    gm_p, dg_p, db_p = gm_p.clone(), dg_p.clone(), db_p.clone()

    gm_l, dg_l, db_l = K.lt_pool_bwd_gather(d, x, 1, p, c, st, mean=False)
    torch.cuda.synchronize()

    assert 0 < int((dz == 0).sum()) < dz.numel()  # the mask is neither empty nor full
    assert torch.equal(gm_p.float().view(p, c), dz.float())
    assert torch.equal(gm_l.view(p, c), dz.float())
    assert torch.equal(dg_p, dg_n) and torch.equal(db_p, db_n)
    assert torch.equal(dg_l, dg_n) and torch.equal(db_l, db_n)
