"""graphcast_lite_amd.downscale against the reference's own outputs (tests/golden/downscale_vectors.npz, made by
tests/golden/make_downscale_golden.py on the case of tests/helpers/downscale_case.py).

Rules:
  files        DownscalerPairs.save: coarse.npy / fine.npy byte for byte, the arrays of static_fine.npy, scalers.npz and
               coords.npz equal in dtype and bits, the two JSON files equal as parsed.
  archive      gnn_pred byte-equal to the reference loop driven with the same stub (tests/helpers/diff_stub.py: exact
               arithmetic, so the CPU run of the fixture and the GPU run give the same bits), residual on and off,
               subsample 1 and 2; the captured replay equal to the eager run.
  batches      bit-equal to the reference's __getitem__ (no flip, no noise).
  baseline     relative n 2^-24 + 2^-23 against compute_metrics' float32 column, n the elements per channel and batch:
               the a-priori bound of any float32 summation order of non-negative terms plus the rounding of the
               square.  Nothing is measured.
"""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import downscale_case as DC  # noqa: E402
import multires_case as MC  # noqa: E402
from diff_stub import DiffStub  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def D(lib_built):
    from graphcast_lite_amd import downscale

    return downscale


@pytest.fixture(scope="module")
def gv():
    return DC.golden()


@pytest.fixture(scope="module")
def dirs(gv, tmp_path_factory):
    return DC.write_pair(str(tmp_path_factory.mktemp("downscale_src")), gv["g_data"], gv["r_data"])


@pytest.fixture(scope="module")
def built_pairs(D, gv, dirs):
    """Built once from the directories, 5 frames per launch (three launches, the last short)."""
    return D.build_downscaler_dataset(dirs[0], dirs[1], DC.ROI, static_channels=DC.STATIC, frames_per_launch=5,
                                      device=DEV, global_source=DC.GLOBAL_SOURCE, region_source=DC.REGION_SOURCE)


@pytest.fixture
def pairs(built_pairs):
    """A shallow copy per test: the archives are shared and never written, and a gnn_pred that a test attaches, or
    leaves behind when it fails, stays with that test."""
    assert built_pairs.gnn_pred is None
    return copy.copy(built_pairs)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- host tables (no GPU) --------------------------------------------------------------------------------------------
def test_coarse_tables_restate_the_reference_builder(D, gv):
    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    la0, la1, lo0, lo1 = D.roi_crop(g_lats, g_lons, DC.ROI)
    assert (la1 - la0, lo1 - lo0) == (2, 5)
    pos, w = D.coarse_tables(g_lats, g_lons, r_lats, r_lons, DC.ROI)
    assert pos.dtype == np.int32 and pos.shape == w.shape == (63, 4) and w.min() < -0.7 and w.max() > 1.8
    assert D.coarse_tables(g_lats, g_lons, r_lats, r_lons, DC.ROI)[0] is pos and not pos.flags.writeable
    acc = DC.restate_coarse(gv["g_data"], pos, w)
    assert acc.astype(np.float16).tobytes() == gv["coarse"].tobytes()
    two_step = acc.astype(np.float32).astype(np.float16)
    assert np.count_nonzero(two_step != acc.astype(np.float16)) == int(gv["n_two_step"]) >= 1


def test_prediction_tables_restate_crop_and_upsample(D, gv):
    pos, w = D.prediction_tables(gv["grid_lats"], gv["grid_lons"], DC.ROI, gv["lat32"].astype(np.float64),
                                 gv["lon32"].astype(np.float64))
    v = gv["crop_in"].astype(np.float64)[pos, :]
    acc = np.zeros((pos.shape[0], DC.C))
    for m in range(4):
        acc = acc + v[:, m, :] * w[:, m, None]
    assert bits_equal(acc.astype(np.float32).reshape(7, 9, DC.C), gv["crop_out"])


def test_a_node_set_with_a_hole_raises_before_any_gpu_call(D, gv):
    lats, lons = gv["grid_lats"], gv["grid_lons"]
    inside = np.nonzero((lats >= DC.ROI[0]) & (lats <= DC.ROI[1]) & (lons >= DC.ROI[2]) & (lons <= DC.ROI[3]))[0]
    assert len(inside) == 35
    keep = np.ones(len(lats), dtype=bool)
    keep[inside[[3, 17]]] = False
    with pytest.raises(ValueError, match="2 of the 35 cells"):
        D.prediction_tables(lats[keep], lons[keep], DC.ROI, gv["lat32"], gv["lon32"])
    with pytest.raises(ValueError, match="2 of the 35 cells"):  # the public function: tables first, then the tensor
        D.crop_and_upsample_roi(torch.zeros(int(keep.sum()), DC.C), lats[keep], lons[keep], DC.ROI, gv["lat32"], gv["lon32"])


def test_roi_crop_needs_two_nodes_per_axis(D):
    g_lats, g_lons = MC.global_axes()
    with pytest.raises(ValueError, match="at least 2"):
        D.roi_crop(g_lats, g_lons, (24.0, 30.0, 60.0, 120.0))


# ---- the pairs -------------------------------------------------------------------------------------------------------
@gpu
def test_saved_pairs_equal_the_reference_files(pairs, gv, tmp_path):
    out = pairs.save(str(tmp_path / "pairs"))
    assert sorted(os.listdir(out)) == ["coarse.npy", "coords.npz", "dataset_info.json", "fine.npy", "scalers.npz",
                                       "static_fine.npy", "variables.json"]
    for name in ("coarse", "fine"):
        with open(os.path.join(out, f"{name}.npy"), "rb") as fh:
            assert fh.read() == gv[name].tobytes(), name
    assert bits_equal(np.load(os.path.join(out, "static_fine.npy")), gv["static_fine"])
    sc = np.load(os.path.join(out, "scalers.npz"))
    assert sorted(sc.files) == ["mean", "n", "std"]
    assert bits_equal(sc["mean"], gv["sc_mean"]) and bits_equal(sc["std"], gv["sc_std"]) and bits_equal(sc["n"], gv["sc_n"])
    co = np.load(os.path.join(out, "coords.npz"))
    assert bits_equal(co["latitude"], gv["lat32"]) and bits_equal(co["longitude"], gv["lon32"])
    with open(os.path.join(out, "dataset_info.json")) as fh:
        assert json.load(fh) == DC.info_of(gv)
    with open(os.path.join(out, "variables.json")) as fh:
        assert json.load(fh) == json.loads(str(gv["variables"]))


@gpu
def test_pairs_from_series_on_the_device_and_reloaded(D, pairs, gv, tmp_path):
    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    mean, std, n = DC.scalers(len(g_lons), len(g_lats))
    sc = dict(mean=mean, std=std, n=n)
    up = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
    p2 = D.build_downscaler_dataset((up(gv["g_data"]), {}, (g_lats, g_lons), sc, DC.VARS),
                                    (up(gv["r_data"]), {}, (r_lats, r_lons), sc, DC.VARS), DC.ROI, static_channels=DC.STATIC)
    assert p2.coarse.cpu().numpy().tobytes() == gv["coarse"].tobytes() and torch.equal(p2.fine, pairs.fine)
    p3 = D.DownscalerPairs.load(pairs.save(str(tmp_path / "again")), DEV)
    assert torch.equal(p3.coarse, pairs.coarse) and torch.equal(p3.static_fine, pairs.static_fine) and p3.gnn_pred is None
    assert p3.info == pairs.info and bits_equal(p3.lats, gv["lat32"].astype(np.float64))


# ---- crop_and_upsample_roi -------------------------------------------------------------------------------------------
@gpu
def test_crop_and_upsample_flat_grid_equals_the_reference(D, gv):
    out = D.crop_and_upsample_roi(torch.from_numpy(gv["crop_in"]).to(DEV), gv["grid_lats"], gv["grid_lons"], DC.ROI,
                                  gv["lat32"].astype(np.float64), gv["lon32"].astype(np.float64), flat_grid=True)
    assert out.dtype == torch.float32 and bits_equal(out.cpu().numpy(), gv["crop_out"])


def _cells(u, x):
    i = np.clip(np.searchsorted(u, x, side="right") - 1, 0, len(u) - 2)
    return i, (x - u[i]) / (u[i + 1] - u[i])


@gpu
def test_crop_and_upsample_regular_grid_reads_lat_major_nodes(D):
    """flat_grid=False against a float64 restatement: nodes lat * n_lon + lon, the box widened by 1 degree, scipy's
    bilinear form over (lats, lons)."""
    lats, lons = MC.global_axes()
    n_lat, n_lon, C = len(lats), len(lons), 3
    lat_g, lon_g = np.meshgrid(lats, lons, indexing="ij")
    grid_lats, grid_lons = lat_g.ravel().astype(np.float32), lon_g.ravel().astype(np.float32)
    rng = np.random.default_rng(8)
    pred = rng.standard_normal((n_lat * n_lon, C)).astype(np.float32)
    t_lats, t_lons = np.linspace(20.0, 40.0, 6), np.linspace(55.0, 125.0, 11)
    roi = (21.5, 38.5, 61.0, 119.0)  # +- 1 degree reaches the nodes at 22.5 / 37.5 and 60 / 120
    out = D.crop_and_upsample_roi(torch.from_numpy(pred).to(DEV), grid_lats, grid_lons, roi, t_lats, t_lons, flat_grid=False)
    ii = np.nonzero((lats >= roi[0] - 1) & (lats <= roi[1] + 1))[0]
    jj = np.nonzero((lons >= roi[2] - 1) & (lons <= roi[3] + 1))[0]
    assert (len(ii), len(jj)) == (2, 5)
    field = pred.reshape(n_lat, n_lon, C)[np.ix_(ii, jj)].astype(np.float64)
    i, yi = _cells(lats[ii], t_lats)
    j, yj = _cells(lons[jj], t_lons)
    I, J = i[:, None], j[None, :]
    wa, wb = (1.0 * (1 - yi))[:, None, None], (1.0 * yi)[:, None, None]
    va, vb = (1 - yj)[None, :, None], yj[None, :, None]
    ref = (((0.0 + field[I, J] * (wa * va)) + field[I, J + 1] * (wa * vb)) + field[I + 1, J] * (wb * va)) \
        + field[I + 1, J + 1] * (wb * vb)
    assert bits_equal(out.cpu().numpy(), ref.astype(np.float32))


# ---- the GNN archive -------------------------------------------------------------------------------------------------
def gnn_sets(gv):
    from graphcast_lite_amd.data import TimeseriesChunkDataset

    mean, std = DC.gnn_scalers()
    flat = torch.from_numpy(gv["flat_data"]).to(DEV)
    return [TimeseriesChunkDataset.from_series(flat, mean, std, DC.OBS, 1, split) for split in ("train", "val", "test_only")]


@gpu
@pytest.mark.parametrize("tag,residual", [("res", True), ("abs", False)])
@pytest.mark.parametrize("subsample", [1, 2])
def test_generated_archive_equals_the_reference_loop(D, pairs, gv, tag, residual, subsample):
    mean, std = DC.gnn_scalers()
    n = D.generate_gnn_predictions(DiffStub(DC.OBS, DC.C), gnn_sets(gv), pairs, gv["grid_lats"], gv["grid_lons"], DC.ROI,
                                   mean, std, DC.OBS, DC.C, flat_grid=True, use_residual=residual, subsample=subsample,
                                   batch_size=3)
    assert n == int(gv[f"gnn_{tag}_{subsample}_count"])
    assert pairs.gnn_pred.cpu().numpy().tobytes() == gv[f"gnn_{tag}_{subsample}"].tobytes()


@gpu
def test_captured_archive_replays_the_eager_run(D, pairs, gv, tmp_path):
    mean, std = DC.gnn_scalers()
    sets = gnn_sets(gv)
    arch = D.CapturedGnnPredictions(DiffStub(DC.OBS, DC.C), pairs, gv["grid_lats"], gv["grid_lons"], DC.ROI, mean, std,
                                    DC.OBS, DC.C, True, True, use_graph=True, required=True)
    n = D.generate_gnn_predictions(None, sets, pairs, None, None, None, None, None, DC.OBS, DC.C, batch_size=1, archive=arch)
    assert arch.graph_active and n == int(gv["gnn_res_1_count"])
    assert pairs.gnn_pred.cpu().numpy().tobytes() == gv["gnn_res_1"].tobytes()
    path = arch.save(str(tmp_path))
    assert open(path, "rb").read() == gv["gnn_res_1"].tobytes()


# ---- batches and the baseline ----------------------------------------------------------------------------------------
@gpu
def test_dataset_lengths_and_items_equal_the_reference(D, pairs, gv):
    for split in DC.SPLITS:
        assert len(D.DownscalerDataset(pairs, obs_window=DC.OBS, split=split)) == int(gv[f"len_{split}"]), split
    ds = D.DownscalerDataset(pairs, obs_window=DC.OBS, split="all")
    for i in DC.SAMPLES:
        X, Y = ds[i]
        assert bits_equal(X.cpu().numpy(), gv[f"X{i}"]) and bits_equal(Y.cpu().numpy(), gv[f"Y{i}"]), i
    X, Y = ds.batch(DC.SAMPLES)
    for k, i in enumerate(DC.SAMPLES):
        assert bits_equal(X[k].cpu().numpy(), gv[f"X{i}"]) and bits_equal(Y[k].cpu().numpy(), gv[f"Y{i}"])
    X, Y = D.DownscalerDataset(pairs, obs_window=3, split="all", static_context=False)[1]
    assert bits_equal(X.cpu().numpy(), gv["o3_X1"]) and bits_equal(Y.cpu().numpy(), gv["o3_Y1"])
    with pytest.raises(FileNotFoundError):
        D.DownscalerDataset(pairs, use_gnn_input=True)
    pairs.gnn_pred = torch.from_numpy(gv["gnn_res_1"]).to(DEV)
    X, _ = D.DownscalerDataset(pairs, obs_window=DC.OBS, split="all", use_gnn_input=True)[4]
    assert bits_equal(X.cpu().numpy(), gv["gnn_X4"])


@gpu
def test_augmentations_apply_to_the_train_split_only(D, pairs):
    kw = dict(obs_window=DC.OBS, augment_flip=True, input_noise=0.05, wind_u_channels=DC.U_CHANNELS)
    tr, va = D.DownscalerDataset(pairs, split="train", **kw), D.DownscalerDataset(pairs, split="val", **kw)
    plain = D.DownscalerDataset(pairs, obs_window=DC.OBS, split="train")
    X0, Y0 = plain.batch([0, 1])
    X, Y = tr.batch([0, 1], flip=[1, 0])
    C, u = DC.C, DC.U_CHANNELS[0]
    sign = torch.ones(X0.shape[1], device=DEV)
    sign[[u, C + u]] = -1
    assert torch.equal(X[0], X0[0].flip(-1) * sign[:, None, None]) and torch.equal(X[1], X0[1])
    assert torch.equal(Y[0, u], -Y0[0, u].flip(-1)) and torch.equal(Y[0, 0], Y0[0, 0].flip(-1))
    noise = torch.randn(2, DC.OBS * C, X0.shape[2], X0.shape[3], device=DEV)
    Xn, _ = tr.batch([0, 1], noise=noise)
    assert torch.equal(Xn[:, :DC.OBS * C], X0[:, :DC.OBS * C] + noise * 0.05) and torch.equal(Xn[:, DC.OBS * C:], X0[:, DC.OBS * C:])
    Xv, Yv = va.batch([0], flip=[1], noise=noise[:1])
    Xp, Yp = D.DownscalerDataset(pairs, obs_window=DC.OBS, split="val").batch([0])
    assert torch.equal(Xv, Xp) and torch.equal(Yv, Yp)


@gpu
@pytest.mark.parametrize("split", ["all", "train"])
def test_coarse_baseline_within_the_float32_bound(D, pairs, gv, split):
    ds = D.DownscalerDataset(pairs, obs_window=DC.OBS, split=split)
    got = D.coarse_baseline(ds)
    ref = gv[f"rmse_coarse_{split}"].astype(np.float64)
    n = len(ds) * ds.n_lat * ds.n_lon  # elements per channel of the one batch the reference averaged
    tol = n * 2.0 ** -24 + 2.0 ** -23
    rel = np.abs(got - ref) / ref
    print("relative deviation per channel:", rel, "bound", tol)
    assert (rel <= tol).all()
    named = D.coarse_baseline(ds, DC.VARS)
    assert list(named) == DC.VARS and named["t2m"] == got[0]
