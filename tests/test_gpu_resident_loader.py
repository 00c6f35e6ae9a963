"""GPU: the resident data path (ESC50DataModule(resident=True), src/datasets/resident.py) against the host path of
the same data module on the same bundle tree: 5 folds x 12 clips, 4 classes, window_length 0.1 (4410 samples,
pad 2205).  Evaluation batches must be equal, crops included; training batches must be the padded clip
(oracle.data.envnet_preprocess) at the starts the loader reports; the augmentation pools must be equal."""
import pytest
import torch
import torch.nn.functional as F

from oracle import data as odata

pytestmark = pytest.mark.gpu

WL, WINDOW, PAD = 0.1, 4410, 2205
PC = {"window_length": WL, "multi_crop_test": True, "test_crops": 5}
RAGGED = [3000, 3001, 4410, 4413, 5000, 6002, 7003, 8000, 8999, 9000, 4409, 4411]


def _tree(root, lengths):
    for f in range(5):
        d = root / f"fold_{f}"
        d.mkdir(parents=True)
        for i in range(12):
            g = torch.Generator().manual_seed(100 * f + i)
            w = 0.1 * torch.randn(1, lengths[(f + i) % len(lengths)], generator=g)
            torch.save({"waveform": w / w.abs().max(), "label": (f + i) % 4}, d / f"{i:02d}.pt")
    return root


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    base = tmp_path_factory.mktemp("resident")
    return {"even": _tree(base / "even", [9000]), "ragged": _tree(base / "ragged", RAGGED),
            "half": _tree(base / "half", [4500])}


def _dm(root, cuda, resident, **kw):
    from src.datasets.esc50 import ESC50DataModule
    kw.setdefault("preprocessing_config", dict(PC))
    dm = ESC50DataModule(root=str(root), fold=0, batch_size=8, num_workers=0, num_classes=4, resident=resident, **kw)
    dm.attach(cuda)
    dm.setup()
    return dm


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_batches(res_loader, host_loader, cuda, crops):
    n = 0
    assert len(res_loader) == len(host_loader)
    for (xr, yr), (xh, yh) in zip(res_loader, host_loader):
        assert yr.is_cuda and yr.dtype == torch.int64 and torch.equal(yr, yh.to(cuda))
        if crops:
            assert isinstance(xr, list) and len(xr) == len(xh) == crops
            for a, b in zip(xr, xh):
                assert a.is_cuda and a.dtype == torch.float32 and a.shape == b.shape == (yr.numel(), 1, WINDOW)
                assert torch.equal(_bits(a), _bits(b.to(cuda)))
        else:
            assert xr.is_cuda and xr.shape == xh.shape and torch.equal(_bits(xr), _bits(xh.to(cuda)))
        n += 1
    assert n == len(host_loader)


@pytest.mark.parametrize("tree", ["even", "ragged"])
@pytest.mark.parametrize("multi", [True, False])
def test_eval_loaders_equal_the_host_path(cuda, trees, tree, multi):
    pc = dict(PC, multi_crop_test=multi)
    res, host = (_dm(trees[tree], cuda, r, preprocessing_config=pc) for r in (True, False))
    assert [str(f) for f in res._val_set.files] == [str(f) for f in host._val_set.files]
    _same_batches(res.val_dataloader(), host.val_dataloader(), cuda, 5 if multi else 0)
    _same_batches(res.test_dataloader(), host.test_dataloader(), cuda, 5 if multi else 0)
    assert len(res.test_dataloader()) == 2  # 12 clips at B = 8: the last batch is partial


@pytest.mark.parametrize("tree", ["even", "ragged"])
@pytest.mark.parametrize("bc", [False, True])
def test_train_loader_rows_are_the_padded_clip_at_last_start(cuda, trees, tree, bc):
    dm = _dm(trees[tree], cuda, True, enable_bc_mixing=bc)
    store, loader = dm._rstore, dm.train_dataloader()
    assert dm.train_dataloader() is loader
    pad = 0 if bc else PAD
    seen = []
    for epoch in (0, 1):
        loader.set_epoch(epoch)
        order = []
        for x, y in loader:
            assert x.is_cuda and x.dtype == torch.float32 and x.shape == (y.numel(), 1, WINDOW)
            idx, start = loader.last_index.tolist(), loader.last_start.tolist()
            assert torch.equal(y, store.labels[loader.last_index.long()])
            for b, (i, s) in enumerate(zip(idx, start)):
                bundle = torch.load(store.paths[i], weights_only=True)
                assert int(y[b]) == int(bundle["label"])
                w = bundle["waveform"].float()
                p = odata.envnet_preprocess(w, WL, 0.5) if not bc else w
                total = p.shape[-1]
                assert 0 <= s <= max(0, total - WINDOW)
                if total < WINDOW:
                    p = F.pad(p, (0, WINDOW - total))
                assert total == w.shape[-1] + 2 * pad
                assert torch.equal(_bits(x[b]), _bits(p[..., s:s + WINDOW].to(cuda)))
            order += idx
        assert sorted(order) == sorted(store.subset(dm._train_set.files).tolist())  # each training clip once
        seen.append(order)
    assert seen[0] != seen[1]  # a new order every epoch


@pytest.mark.parametrize("tree", ["even", "ragged"])
def test_envnet_pool_equals_the_host_pool(cuda, trees, tree):
    res, host = (_dm(trees[tree], cuda, r, enable_bc_mixing=True) for r in (True, False))
    res._pools()
    host._pools()
    assert res._pool.is_cuda and res._pool.shape == host._pool.shape == (len(host._train_set), WINDOW)
    assert torch.equal(_bits(res._pool), _bits(host._pool))
    assert torch.equal(res._pool_labels, host._pool_labels)


def test_ast_mode_pool_and_batches_equal_the_host_path(cuda, trees):
    kw = dict(is_spectrogram=True, enable_mixup=True, preprocessing_config={})
    res, host = (_dm(trees["even"], cuda, r, **kw) for r in (True, False))
    _same_batches(res.val_dataloader(), host.val_dataloader(), cuda, 0)
    _same_batches(res.test_dataloader(), host.test_dataloader(), cuda, 0)
    x, y = next(iter(res.train_dataloader()))
    assert x.is_cuda and x.shape == (8, 1, 9000) and y.shape == (8,)
    res._pools()
    host._pools()
    assert res._pool.shape == host._pool.shape and torch.equal(_bits(res._pool), _bits(host._pool))
    assert torch.equal(res._pool_labels, host._pool_labels)
    with pytest.raises(ValueError, match="lengths"):
        _dm(trees["ragged"], cuda, True, **kw).val_dataloader()


def test_resampled_store_is_uploaded_as_it_is(cuda, trees):
    pc = dict(PC, sample_rate=44_100)
    res, host = (_dm(trees["half"], cuda, r, sample_rate=22_050, preprocessing_config=pc) for r in (True, False))
    rs, st = res._store, res._rstore
    assert st.data.is_cuda and torch.equal(_bits(st.data), _bits(rs.data.to(cuda)))
    assert st.offsets_host == list(rs.offsets) and st.labels_host == list(rs.labels) and st.paths == rs.paths
    assert st.lengths_host == [9000] * 60 and st.sample_rate == 44_100
    _same_batches(res.val_dataloader(), host.val_dataloader(), cuda, 5)
    _same_batches(res.test_dataloader(), host.test_dataloader(), cuda, 5)


def test_size_cap_and_mixed_crop_counts_raise(cuda, trees):
    from src.datasets import resident as R
    with pytest.raises(ValueError, match="resident_max_gib"):
        _dm(trees["even"], cuda, True, resident_max_gib=1e-3)  # 60 x 9000 f32 = 2.06 MiB > 1.05 MB
    lens = [1000, 9000]
    store = R.ResidentStore(["a", "b"], torch.zeros(sum(lens), device=cuda), [0, 1000, 10000], [0, 1], 44_100)
    starts, counts = R.multi_crop_starts(lens, 0, WINDOW, 5)
    assert counts.tolist() == [1, 5]
    with pytest.raises(ValueError, match="crops"):
        R._ResidentLoader(store, torch.tensor([0, 1]), 2, "multi", 0, WINDOW, False, table=starts.to(cuda),
                          counts=counts)
    one = R._ResidentLoader(store, torch.tensor([0]), 2, "multi", 0, WINDOW, False, table=starts.to(cuda),
                            counts=counts)
    x, y = next(iter(one))
    assert isinstance(x, list) and len(x) == 1 and x[0].shape == (1, 1, WINDOW) and not x[0].any()
