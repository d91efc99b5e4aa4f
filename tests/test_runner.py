"""The experiment runner on the GPU: the fused validation step against the reference's `test()` fixture, the legacy and
chunked datasets against fixtures produced by the reference's loaders, and `main()` end to end on both dataset forms."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, experiment

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import runner_case as RC  # noqa: E402
from stub_model import EVAL_CASES, StubModel  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _npz(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


# ------------------------------------------------------------------------------------------------
# Evaluator
# ------------------------------------------------------------------------------------------------
def _eval_case(tag):
    z = _npz("train_loop_vectors.npz")
    batches = [(torch.tensor(x).to(DEV), torch.tensor(y).to(DEV)) for x, y in zip(z["X"], z["Y"])]
    spec = EVAL_CASES.get(tag)
    if tag == "eval_single_target":
        C = int(z["C"])
        batches = [(X, Y[..., :C].contiguous()) for X, Y in batches]
        spec = dict(lat=True)
    t = lambda a: torch.tensor(a).to(DEV)  # noqa: E731
    kw = dict(lat_weights=t(z["lat_w"]) if spec.get("lat") else None,
              channel_mask=t(z["chan_mask"]) if spec.get("chan") else None,
              spatial_mask=t(z["spatial_mask"]) if spec.get("smask") else None,
              static_channels=spec.get("static"), forcing_channels=spec.get("forcing"),
              use_residual=spec.get("residual", True))
    return StubModel(z["obs"], z["W0"], z["b0"], DEV), batches, kw, z[tag]


@pytest.mark.parametrize("tag", list(EVAL_CASES) + ["eval_single_target"])
def test_evaluator_reproduces_reference_test(tag, lib_built):
    """The bar `train.test` is held to (5e-6 max(1, |v|)); eager and captured passes give the same bits."""
    from graphcast_lite_amd.train import Evaluator

    model, batches, kw, want = _eval_case(tag)
    eager = Evaluator(model, use_graph=False, **kw).evaluate(batches)
    print(tag, "evaluator", eager, "reference", tuple(want))
    for a, b in zip(eager, want):
        assert abs(a - b) <= 5e-6 * max(1.0, abs(b)), (tag, eager, want)
    ev = Evaluator(model, use_graph=True, **kw)
    for call in range(5):
        assert ev.evaluate(batches) == eager, (tag, call)
    assert ev.graph_active and ev.launch_mode == "hipGraph replay"
    bufs = ev.input_buffers()  # batches written into the graph's own inputs: no copy, the same bits
    for X, y in batches:
        bufs[0].copy_(X), bufs[1].copy_(y)
        ev.update(*bufs)
    assert ev.results() == eager and Evaluator(model, use_graph=False, **kw).input_buffers() is None
    # a pass whose last batch is smaller: that batch runs eagerly, the graph stays
    X, y = batches[-1]
    short = batches[:-1] + [(X[:1].contiguous(), y[:1].contiguous())]
    assert ev.evaluate(short) == Evaluator(model, use_graph=False, **kw).evaluate(short)
    assert ev.graph_active
    assert ev.results() == (0.0, 0.0, 0.0)  # results() reset the state


def test_evaluator_update_does_not_synchronise(lib_built):
    """After the first batch of a shape (which builds the cached weight vectors and reads their sums back once) and the
    capture, `update` neither synchronises nor reads back: torch's sync debug mode would raise."""
    from graphcast_lite_amd.train import Evaluator

    model, batches, kw, _ = _eval_case("eval_all")
    X, y = batches[-1]
    short = (X[:1].contiguous(), y[:1].contiguous())
    eager, captured = Evaluator(model, use_graph=False, **kw), Evaluator(model, use_graph=True, **kw)
    for ev in (eager, captured):
        ev.evaluate(batches + [short])
    assert captured.graph_active
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:  # pragma: no cover
        pytest.skip(f"this torch build refuses torch.cuda.set_sync_debug_mode('error'): {e}")
    try:
        for ev in (eager, captured):
            for Xb, yb in batches + [short]:
                assert ev.update(Xb, yb) is None
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert eager.results() == captured.results()


# ------------------------------------------------------------------------------------------------
# datasets
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,five_d,coords,flattened", [("ref4", False, False, True), ("ref5", True, True, True),
                                                         ("nf", False, False, False)])
def test_weather_dataset_matches_reference_loader(tag, five_d, coords, flattened, tmp_path, monkeypatch, lib_built):
    from graphcast_lite_amd import data

    z = _npz("runner_vectors.npz")
    monkeypatch.setitem(data._DATASETS, RC.NAME, RC.TABLE_ROW)
    path = RC.write_legacy(str(tmp_path / tag), z, five_d=five_d, coords=coords)
    sets = data.load_train_and_test_datasets(path, RC.data_config(flattened), device=DEV)
    md = sets[3]
    assert [md.num_longitudes, md.num_latitudes] == list(z[f"{tag}_grid"])
    assert np.array_equal(md.cordinates[0], z[f"{tag}_lats"]) and np.array_equal(md.cordinates[1], z[f"{tag}_lons"])
    assert sets[1].store_X.data_ptr() == sets[2].store_X.data_ptr()  # val and test: two ranges of one upload
    for split, ds in zip(("train", "val", "test"), sets[:3]):
        wX, wy = torch.tensor(z[f"{tag}_X_{split}"]), torch.tensor(z[f"{tag}_y_{split}"])
        n = len(ds)
        assert n == wX.shape[0] and ds.X.is_cuda
        assert torch.equal(ds.X.cpu(), wX) and torch.equal(ds.y.cpu(), wy)
        for i in (0, n - 1):
            Xi, yi = ds[i]
            assert torch.equal(Xi.cpu(), wX[i]) and torch.equal(yi.cpu(), wy[i])
        idx = [n - 1, 0, 0, n // 2]
        Xb, yb = ds.batch(idx)
        assert torch.equal(Xb.cpu(), wX[idx]) and torch.equal(yb.cpu(), wy[idx])
        # into a larger, strided buffer
        sx, sy = ds.batch_shapes(len(idx))
        wideX = torch.full((sx[0] + 1, sx[1] + 2) + tuple(sx[2:]), -7.0, device=DEV)
        wideY = torch.full((sy[0], sy[1] + 1) + tuple(sy[2:]), -7.0, device=DEV)
        outX, outY = wideX[1:, 1:sx[1] + 1], wideY[:, :sy[1]]
        got = ds.batch(idx, out=(outX, outY))
        assert got[0] is outX and torch.equal(outX.cpu(), wX[idx]) and torch.equal(outY.cpu(), wy[idx])
        assert bool((wideX[0] == -7.0).all()) and bool((wideX[:, 0] == -7.0).all()) and bool((wideY[:, -1] == -7.0).all())
        with pytest.raises(ValueError, match="outside"):
            ds.batch([0, n])


@pytest.mark.parametrize("kind", ["reg", "flat"])
def test_chunked_datasets_share_one_upload(kind, tmp_path, lib_built):
    from graphcast_lite_amd.data import TimeseriesChunkDataset, load_chunked_datasets

    z = _npz("runner_vectors.npz")
    path = RC.write_chunked(str(tmp_path / kind), z, flat=kind == "flat")
    kw = dict(obs_window=RC.CH_OBS, pred_steps=RC.CH_PRED)
    train, val, test, md = load_chunked_datasets(path, n_features=RC.CH_FEAT, device=DEV, **kw)
    assert train.chunks[0].is_cuda
    assert train.chunks[0].data_ptr() == val.chunks[0].data_ptr() == test.chunks[0].data_ptr()
    assert [len(train), len(val), len(test)] == list(z[f"chk_{kind}_len"])
    assert md.flat_grid == (kind == "flat")
    for split, ds in (("train", train), ("val", val), ("test_only", test)):
        own = TimeseriesChunkDataset(path, split=split, n_features=RC.CH_FEAT, device=DEV, **kw)
        assert len(own) == len(ds)
        idx = list(range(len(ds)))[::-1]
        for a, b in zip(ds.batch(idx), own.batch(idx)):
            assert torch.equal(a, b)
        tag = "test" if split == "test_only" else split
        X0, Y0 = ds[0]
        assert np.array_equal(X0.cpu().numpy(), z[f"chk_{kind}_{tag}_X0"])
        assert np.array_equal(Y0.cpu().numpy(), z[f"chk_{kind}_{tag}_Y0"])


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
LON, LAT, FEAT = 16, 8, 3
LEGACY_NAME = "demo_era5_small"  # 3 features, 2 observed steps, 1 target step; its 64 x 32 grid is replaced by the files'


def _write_legacy(root, n_train, n_test=10, coords=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    path = os.path.join(root, LEGACY_NAME)
    os.makedirs(path, exist_ok=True)
    for split, n in (("train", n_train), ("test", n_test)):
        X = torch.randn(n, LON, LAT, 2 * FEAT, generator=g)
        y = X[..., FEAT:] + 0.1 * torch.randn(n, LON, LAT, FEAT, generator=g)
        torch.save(X, os.path.join(path, f"X_{split}.pt"))
        torch.save(y, os.path.join(path, f"y_{split}.pt"))
    if coords is not None:
        np.savez(os.path.join(path, "coords.npz"), latitude=coords[0], longitude=coords[1])
    return root


def _write_chunked(path, T=21, seed=0):
    rng = np.random.default_rng(seed)
    series = rng.standard_normal((T, LON, LAT, FEAT)).astype(np.float16)
    z = dict(reg_series=series, reg_mean=np.zeros(FEAT, np.float32), reg_std=np.ones(FEAT, np.float32),
             reg_lon=np.linspace(0, 360, LON, endpoint=False), reg_lat=np.linspace(-90, 90, LAT))
    return RC.write_chunked(path, z)


def _experiment_dir(path, mesh_levels=(1,), **over):
    cfg = experiment("demo_low", list(mesh_levels)).model_dump(mode="json")
    cfg.update(batch_size=4, num_epochs=2, learning_rate=1e-3, wandb_log=False)
    cfg["data"]["dataset_name"] = LEGACY_NAME
    cfg.update(over)
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(cfg, fh)
    return path


class _HandBuilt:
    """Batches indexed by hand out of the whole split, in torch's DataLoader order."""

    def __init__(self, ds, batch_size, shuffle):
        from torch.utils.data import DataLoader

        self.X, self.y = ds.batch(list(range(len(ds))))
        self.index = DataLoader(range(len(ds)), batch_size=batch_size, shuffle=shuffle)

    def __len__(self):
        return len(self.index)

    def __iter__(self):
        for idx in self.index:
            idx = idx.to(self.X.device)
            yield self.X[idx], self.y[idx]


def _second_run(exp_dir, data_root, results_dir):
    """The pieces of `run_experiment` with hand-built batches, `train.test` for validation and no evaluator."""
    from graphcast_lite_amd import main as M
    from graphcast_lite_amd.config import ExperimentConfig
    from graphcast_lite_amd.train import build_optimizer, train

    with open(os.path.join(exp_dir, "config.json")) as fh:
        cfg = ExperimentConfig(**json.load(fh))
    M.set_random_seeds()
    tr, va, te, md = M.load_datasets(cfg, data_root, torch.device(DEV))
    model = M.load_model_from_experiment_config(cfg, torch.device(DEV), md, coordinates=md.cordinates,
                                                region_bounds=M.detect_region_bounds(md.cordinates),
                                                flat_grid=md.flat_grid)
    opt = build_optimizer(model, cfg, pretrained=False)
    os.makedirs(results_dir, exist_ok=True)
    bs = cfg.batch_size
    return train(model, _HandBuilt(tr, bs, True), _HandBuilt(va, bs, False), _HandBuilt(te, bs, False), opt,
                 cfg.num_epochs, torch.device(DEV), cfg, results_dir, dataset_metadata=md, print_losses=False,
                 evaluator=None)


@pytest.mark.parametrize("form", ["legacy", "chunked"])
def test_main_trains_an_experiment_directory(form, tmp_path, lib_built):
    from graphcast_lite_amd import main as M

    root = str(tmp_path / "datasets")
    if form == "legacy":
        _write_legacy(root, n_train=12)
        exp = _experiment_dir(str(tmp_path / "exp"))
    else:
        exp = _experiment_dir(str(tmp_path / "exp"), data_dir=_write_chunked(os.path.join(root, "series")))
    results = M.main([exp], data_root=root)
    out = os.path.join(exp, "results")
    for name in ("training_log.txt", "best_model.pth", "checkpoint.pth", "results.json"):
        assert os.path.exists(os.path.join(out, name)), name
    with open(os.path.join(out, "results.json")) as fh:
        assert json.load(fh) == results
    assert len(results["train_losses"]) == len(results["val_losses"]) == 2
    assert all(np.isfinite(results["train_losses"] + results["val_losses"]))
    log = open(os.path.join(out, "training_log.txt")).read()
    assert " init " in log and "Training finished" in log

    want = _second_run(exp, root, str(tmp_path / "second"))
    print(form, "runner", results, "second run", want)
    for a, b in zip(results["train_losses"], want["train_losses"]):
        assert abs(a - b) <= 1e-5 * abs(b), (results, want)
    for a, b in zip(results["val_losses"], want["val_losses"]):
        assert abs(a - b) <= 5e-6 * max(1.0, abs(b)), (results, want)


def test_resume_continues_at_the_second_epoch(tmp_path, lib_built):
    """One epoch, then `--resume` for the second, against two epochs in one go.  The runner seeds 42 at every start,
    as the reference does, so the resumed epoch draws the first epoch's permutation again: with one batch per epoch
    (4 samples, batch_size 4) the permutation only orders the samples inside the batch, which the sums over the batch
    do not depend on beyond rounding."""
    from graphcast_lite_amd import main as M

    root = _write_legacy(str(tmp_path / "datasets"), n_train=4)
    whole = _experiment_dir(str(tmp_path / "whole"))
    res_whole = M.main([whole], data_root=root, use_graph=False)
    parts = _experiment_dir(str(tmp_path / "parts"), num_epochs=1)
    first = M.main([parts], data_root=root, use_graph=False)
    assert len(first["train_losses"]) == 1
    _experiment_dir(parts)  # two epochs now
    res = M.main([parts, "--resume"], data_root=root, use_graph=False)
    assert len(res["train_losses"]) == 2 and res["train_losses"][0] == first["train_losses"][0]
    assert ">>> Resumed from epoch 1" in open(os.path.join(parts, "results", "training_log.txt")).read()
    for a, b in zip(res["train_losses"] + res["val_losses"], res_whole["train_losses"] + res_whole["val_losses"]):
        assert abs(a - b) <= 1e-5 * abs(b)
    load = lambda d: torch.load(os.path.join(d, "results", "checkpoint.pth"), map_location="cpu", weights_only=True)  # noqa: E731
    a, b = load(parts), load(whole)
    assert a["epoch"] == b["epoch"] == 1
    for k, v in b["model_state_dict"].items():
        if v.is_floating_point():
            err = float((a["model_state_dict"][k] - v).norm() / (v.norm() + 1e-30))
            assert err <= 1e-5, (k, err)


def test_regional_coordinates_prune_the_mesh(tmp_path, lib_built):
    from graphcast_lite_amd import main as M
    from graphcast_lite_amd.config import ExperimentConfig

    coords = (np.linspace(50, 60, LAT), np.linspace(85, 100, LON))
    root = _write_legacy(str(tmp_path / "datasets"), n_train=8, coords=coords)
    exp = _experiment_dir(str(tmp_path / "exp"), mesh_levels=(3,), num_epochs=1)
    with open(os.path.join(exp, "config.json")) as fh:
        cfg = ExperimentConfig(**json.load(fh))
    md = M.load_datasets(cfg, root, torch.device(DEV))[3]
    bounds = M.detect_region_bounds(md.cordinates)
    assert bounds == (50.0, 60.0, 85.0, 100.0)
    model = M.load_model_from_experiment_config(cfg, torch.device(DEV), md, coordinates=md.cordinates,
                                                region_bounds=bounds)
    assert model._num_grid_nodes == LON * LAT and 0 < model._num_mesh_nodes < 642  # 642: the global level-3 mesh
    results = M.main([exp], data_root=root)  # and the runner trains on it
    assert len(results["train_losses"]) == 1 and np.isfinite(results["train_losses"][0])
    state = torch.load(os.path.join(exp, "results", "best_model.pth"), map_location="cpu", weights_only=True)
    assert state["_processing_edge_features"].shape == model._processing_edge_features.shape


def test_pretrained_with_frozen_processor(tmp_path, lib_built):
    from graphcast_lite_amd import main as M

    root = _write_legacy(str(tmp_path / "datasets"), n_train=8)
    donor = _experiment_dir(str(tmp_path / "donor"), num_epochs=1)
    M.main([donor], data_root=root)
    ckpt = os.path.join(donor, "results", "best_model.pth")
    exp = _experiment_dir(str(tmp_path / "exp"), num_epochs=1, freeze_processor_epochs=1)
    M.main([exp, "--pretrained", ckpt], data_root=root)
    before = torch.load(ckpt, map_location="cpu", weights_only=True)
    after = torch.load(os.path.join(exp, "results", "checkpoint.pth"), map_location="cpu", weights_only=True)
    moved = 0
    for k, v in before.items():
        if k.startswith("processor."):
            assert torch.equal(after["model_state_dict"][k], v), k
        elif v.is_floating_point() and not torch.equal(after["model_state_dict"][k], v):
            moved += 1
    assert moved > 0
    groups = after["optimizer_state_dict"]["param_groups"]
    assert len(groups) == 2 and abs(groups[1]["lr"] - 0.1 * groups[0]["lr"]) < 1e-12
