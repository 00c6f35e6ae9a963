"""GPU: one EnvNet-v2 bf16 training step (B = 2, T = 220 500, the same weights and clips) with the trunk-backward
switches unset and with both set -- MIA_W2_PADCOPY=1 (the (1, 2)-conv gradients through the copy pass mia_pad_w2
instead of their producers' row-mapped stores) and MIA_C3W_V1=1 (the conv3 weight gradient + BN3 backward before its
reschedule).  The forms differ in schedule and addresses only: logits and every parameter gradient must be
`torch.equal`.  (A third switch was planned for a trimmed conv4 weight gradient; that change measured slower and is
not in the library -- DESIGN.md section 6, "Trunk backward".)"""
import pytest
import torch

from oracle.synth import synth_waveform
from tests._util import envnet_with_hash_params

pytestmark = pytest.mark.gpu

SWITCHES = ("MIA_W2_PADCOPY", "MIA_C3W_V1")


def _step(cuda, x, y):
    from src.miaudio import kernels as K
    m = envnet_with_hash_params(cuda, compute_dtype="bf16").train()
    z = m(x)
    _, dz, _ = K.soft_ce(z.detach().float().contiguous(), y, input_sigmoid=False)
    z.backward(dz)
    torch.cuda.synchronize()
    return z.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def test_envnet_step_same_bits_with_the_previous_forms(cuda, monkeypatch):
    for v in SWITCHES + ("MIA_W2_SHIFT",):
        monkeypatch.delenv(v, raising=False)
    x = torch.from_numpy(synth_waveform(21, 2, 220_500)[:, None, :]).to(cuda)
    y = torch.zeros(2, 50, device=cuda)
    y[0, 3] = 1.0
    y[1, 7], y[1, 12] = 0.8, 0.2
    z_new, g_new = _step(cuda, x, y)
    for v in SWITCHES:
        monkeypatch.setenv(v, "1")
    z_old, g_old = _step(cuda, x, y)
    assert torch.equal(z_new, z_old), "logits differ"
    assert set(g_new) == set(g_old) and len(g_new) > 40
    for n in g_new:
        assert torch.equal(g_new[n], g_old[n]), f"gradient of {n} differs between the forms"
