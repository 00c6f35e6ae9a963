"""CPU: stochastic weight averaging -- the schedule arithmetic and constructor checks of the callback, the CPU
Trainer on a toy model against a plain-torch restatement (SWALR + the averaging expression), early stop, resume
from inside the averaging window, two gloo ranks, the config surface and the C header."""
import importlib.util
import os
import re
import socket
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

from src.training.engine import LitClassifier
from src.training.lite import StochasticWeightAveraging, Trainer
from src.training.swa import swa_window
from src.utils.config import compose
from tests._swa_ref import FixedDM, Recorder, SaveAt, StopAfter, restate_fit

REPO = Path(__file__).resolve().parents[1]
PKG = REPO / "dl-sound-classification_amd"
HEADER = REPO / "include" / "miaudio_swa.h"
SWA = dict(swa_lrs=1e-3, swa_epoch_start=0.5, annealing_epochs=2)


def _lit(model="ToyBN", seed=0):
    torch.manual_seed(seed)
    return LitClassifier({"_target_": f"tests._swa_toy.{model}", "num_classes": 5, "in_samples": 16},
                         {"_target_": "torch.optim.Adam", "lr": 1e-2},
                         {"_target_": "torch.optim.lr_scheduler.CosineAnnealingLR", "T_max": 4})


def _bn(lit):
    return lit.model.net[2]


def test_schedule_arithmetic():
    assert swa_window(4, 0.5) == (1, 3)
    assert swa_window(250, 0.75)[0] == 186
    assert swa_window(10, 1) == (0, 9)
    assert swa_window(10, 0.0) == (0, 9)


@pytest.mark.parametrize("kw", [dict(swa_lrs=0.0), dict(swa_lrs=-1e-3), dict(swa_lrs=1e-3, swa_epoch_start=1.5),
                                dict(swa_lrs=1e-3, swa_epoch_start=-0.1), dict(swa_lrs=1e-3, swa_epoch_start=0),
                                dict(swa_lrs=1e-3, annealing_strategy="exp")])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        StochasticWeightAveraging(**kw)


def test_two_parameter_groups_are_rejected():
    lit = _lit()
    ps = list(lit.parameters())
    lit.configure_optimizers = lambda: torch.optim.SGD([{"params": ps[:1]}, {"params": ps[1:]}], lr=0.1)
    with pytest.raises(ValueError, match="one parameter group"):
        Trainer(max_epochs=2, accelerator="cpu", callbacks=[StochasticWeightAveraging(1e-3)]).fit(lit, FixedDM())


@pytest.mark.parametrize("model,extra", [("ToyBN", 1), ("ToyPlain", 0)])
def test_trainer_matches_plain_torch_restatement(model, extra):
    dm, rec = FixedDM(), Recorder()
    lit = _lit(model)
    Trainer(max_epochs=4, accelerator="cpu", callbacks=[StochasticWeightAveraging(**SWA), rec]).fit(lit, dm)
    want, lrs, total = restate_fit(_lit(model), dm, 4, SWA["swa_lrs"], 0.5, 2)
    assert rec.epochs == list(range(4 + extra)) and total == 4 + extra
    assert rec.lrs == lrs
    assert lrs[-1] == pytest.approx(1e-3) and lrs[0] != lrs[1]
    for got, ref in zip(lit.parameters(), want):
        assert torch.equal(got.detach(), ref)
    for got, ref in zip(rec.final, want):  # nothing after the loop but the transfer (no BN)
        assert torch.equal(got, ref)
    assert rec.steps[3] == 4 * len(dm.train)
    if extra:
        assert rec.steps[4] == rec.steps[3], "the re-estimate epoch takes no optimizer step"
        assert all(int(s["step"]) == 4 * len(dm.train) for s in lit.trainer.optimizer.state.values())


def test_bn_statistics_are_the_cumulative_mean_of_the_extra_epoch():
    dm = FixedDM()
    lit = _lit()
    Trainer(max_epochs=4, accelerator="cpu", callbacks=[StochasticWeightAveraging(**SWA)]).fit(lit, dm)
    bn = _bn(lit)
    assert bn.momentum == 0.1, "momentum restored"
    assert int(bn.num_batches_tracked) == len(dm.train)
    with torch.no_grad():  # the final (averaged) weights are the ones the extra epoch ran on
        hs = [lit.model.net[1](x.flatten(1)).double() for x, _ in dm.train]
    mean = torch.stack([h.mean(0) for h in hs]).mean(0)
    var = torch.stack([h.var(0, unbiased=True) for h in hs]).mean(0)
    # f32 statistics of 8 rows, then k = 1..4 cumulative updates: a few ulp of O(1) values
    assert torch.allclose(bn.running_mean.double(), mean, rtol=0, atol=1e-6)
    assert torch.allclose(bn.running_var.double(), var, rtol=1e-5, atol=1e-6)


def test_early_stop_before_swa_end_transfers_nothing(capsys):
    dm, stop = FixedDM(), StopAfter(3)
    swa = StochasticWeightAveraging(swa_lrs=1e-3, swa_epoch_start=0.5, annealing_epochs=2)
    lit = _lit()
    Trainer(max_epochs=6, accelerator="cpu", callbacks=[swa, stop]).fit(lit, dm)
    assert swa.n_averaged == 2 and (swa.swa_start, swa.swa_end) == (2, 5)
    for p, kept, a in zip(lit.parameters(), stop.params, swa._avg):
        assert torch.equal(p.detach(), kept) and not torch.equal(kept, a)
    assert _bn(lit).momentum == 0.1 and int(_bn(lit).num_batches_tracked) == 4 * len(dm.train)
    assert "not transferred" in capsys.readouterr().out


def test_resume_inside_the_window_matches_the_uninterrupted_run(tmp_path):
    dm = FixedDM()
    swa = dict(swa_lrs=1e-3, swa_epoch_start=0.4, annealing_epochs=3)  # E = 5: swa_start 1
    rec, lit = Recorder(), _lit()
    Trainer(max_epochs=5, accelerator="cpu",
            callbacks=[StochasticWeightAveraging(**swa), rec, SaveAt(2, tmp_path / "mid.ckpt")]).fit(lit, dm)
    rec2, lit2 = Recorder(), _lit(seed=123)
    cb2 = StochasticWeightAveraging(**swa)
    tr2 = Trainer(max_epochs=5, accelerator="cpu", callbacks=[cb2, rec2])
    tr2.fit(lit2, dm, ckpt_path=str(tmp_path / "mid.ckpt"))
    assert rec.epochs == [0, 1, 2, 3, 4, 5] and rec2.epochs == [3, 4, 5]
    assert rec2.lrs == rec.lrs[3:]
    assert type(tr2.scheduler).__name__ == "SWALR" and cb2.n_averaged == 4
    for a, b in zip(lit.parameters(), lit2.parameters()):
        assert torch.equal(a.detach(), b.detach())
    for a, b in zip(_bn(lit).buffers(), _bn(lit2).buffers()):
        assert torch.equal(a, b)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    import torch.distributed as dist
    dm = FixedDM(n_batches=3, seed=10 + rank)  # every rank its own clips
    lit = _lit(seed=rank)                      # and its own initial weights: rank 0's are broadcast
    rec = Recorder()
    Trainer(max_epochs=3, accelerator="cpu", callbacks=[StochasticWeightAveraging(**SWA), rec]).fit(lit, dm)
    q.put((rank, rec.epochs, [p.detach().numpy().copy() for p in lit.parameters()],
           [b.numpy().copy() for b in _bn(lit).buffers()], _bn(lit).momentum))
    dist.destroy_process_group()


def test_two_gloo_ranks_end_with_equal_parameters_and_bn_buffers():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, *rest = q.get(timeout=120)
        res[r] = rest
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in range(world):
        assert res[r][0] == [0, 1, 2, 3] and res[r][3] == 0.1
    for a, b in zip(res[0][1], res[1][1]):
        assert (a == b).all()
    for a, b in zip(res[0][2], res[1][2]):
        assert (a == b).all()
    assert int(res[0][2][2]) == 3  # num_batches_tracked: the three forwards of the extra epoch


def _script():
    spec = importlib.util.spec_from_file_location("train_script", PKG / "scripts" / "train.py")
    ts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ts)
    return ts


def test_config_surface():
    ts = _script()
    none = ts.build_callbacks(compose(PKG / "configs", "training", []))
    assert not any(isinstance(cb, StochasticWeightAveraging) for cb in none)
    cfg = compose(PKG / "configs", "training", ["+swa.enabled=true"])
    (cb,) = [c for c in ts.build_callbacks(cfg) if isinstance(c, StochasticWeightAveraging)]
    assert (cb.swa_lr, cb.swa_epoch_start, cb.annealing_epochs, cb.annealing_strategy) == (1e-3, 0.75, 10, "cos")
    cfg = compose(PKG / "configs", "training", ["+swa.enabled=true", "+swa.swa_lrs=1e-4", "+swa.swa_epoch_start=0.5",
                                                "+swa.annealing_epochs=2", "+swa.annealing_strategy=linear"])
    (cb,) = [c for c in ts.build_callbacks(cfg) if isinstance(c, StochasticWeightAveraging)]
    assert (cb.swa_lr, cb.swa_epoch_start, cb.annealing_epochs, cb.annealing_strategy) == (1e-4, 0.5, 2, "linear")
    off = compose(PKG / "configs", "training", ["+swa.enabled=false", "+swa.swa_lrs=1e-4"])
    assert not any(isinstance(c, StochasticWeightAveraging) for c in ts.build_callbacks(off))


def test_header_functions_are_exported_and_bound():
    from src.miaudio import lib as L
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    decls = dict(re.findall(r"\bint\s+(mia_\w+)\s*\(([^)]*)\)\s*;", text))
    assert set(decls) == {"mia_swa_update", "mia_swa_transfer"}
    assert set(decls) <= set(L.SIGNATURES) and set(decls) <= L.exported_symbols()
    for name, params in decls.items():
        assert len(L.SIGNATURES[name][1]) == len(params.split(",")), name
