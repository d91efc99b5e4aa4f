"""Fitting the learned-MOS forest (graphcast_lite_amd.mos: training_table, fit_mos_table, MOSFitter, ...) against
sklearn's own fits in tests/golden/mos_fit_vectors.npz (tests/golden/make_mos_fit_golden.py).

CPU: the host arithmetic (bin thresholds, early-stopping split, baseline, stopping rule, feature table) bit for bit, and
the numpy restatement tests/helpers/hgb_ref.py - the yardstick of tests/test_mos_fit_kernels.py - against sklearn's
30-iteration forest.  GPU: the device fit against sklearn's forests, walked from each root."""
import os
import sys
from datetime import datetime, timedelta

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hgb_ref  # noqa: E402

from graphcast_lite_amd import mos  # noqa: E402

FOREST_KEYS = ("feature", "value", "left", "right", "missing_left", "is_leaf")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLDEN, "mos_fit_vectors.npz")))


def table(gold, tag):
    return gold[f"{tag}_X"].astype(np.float64), gold[f"{tag}_y"].astype(np.float64)


def gold_forest(gold, prefix):
    return {k: gold[f"{prefix}_forest_{k}"] for k in FOREST_KEYS}, gold[f"{prefix}_forest_roots"]


def forest_arrays(forest):
    return {k: getattr(forest, k) for k in FOREST_KEYS}, forest.roots


def assert_thresholds(th, gold, prefix):
    nthr = gold[f"{prefix}_nthr"]
    assert [len(t) for t in th] == nthr.tolist()
    for f, t in enumerate(th):
        assert t.dtype == np.float64
        assert t.tobytes() == gold[f"{prefix}_thr"][f, :nthr[f]].tobytes(), f"feature {f}"


# ======================================================================================================================
# CPU: host arithmetic
# ======================================================================================================================
@pytest.mark.parametrize("tag", ["t1", "t2"])
def test_split_thresholds_baseline_match_sklearn(gold, tag):
    X, y = table(gold, tag)
    seed, train, val = mos.early_stopping_split(len(y), 0.1, 42)
    assert np.array_equal(train, gold[f"{tag}_es_train_rows"]) and np.array_equal(val, gold[f"{tag}_es_val_rows"])
    assert len(val) == int(np.ceil(0.1 * len(y))) and len(train) == int(np.floor(0.9 * len(y)))
    assert_thresholds(mos.bin_thresholds(X[train], 255, seed), gold, f"{tag}_es")
    assert_thresholds(mos.bin_thresholds(X, 255, seed), gold, f"{tag}_it30")
    assert np.float64(np.mean(y[train])).tobytes() == gold[f"{tag}_es_forest_baseline"].tobytes()
    nthr = gold[f"{tag}_es_nthr"]
    assert nthr[17] == 0 and nthr[6] < 254 and nthr[0] == 254  # constant, few distinct values, percentiles


def test_thresholds_subsample_matches_binmapper():
    """Above 200 000 rows the thresholds come from sklearn's subsample of the rows."""
    bm = pytest.importorskip("sklearn.ensemble._hist_gradient_boosting.binning")
    rng = np.random.default_rng(5)
    n = 250_000
    X = np.column_stack([rng.normal(0, 10, n), np.round(rng.uniform(0, 50, n)), np.full(n, 3.5),
                         np.where(rng.random(n) < 0.8, 0.0, rng.exponential(1.0, n))])
    seed = mos.early_stopping_split(10, 0.1, 42)[0]
    ref = bm._BinMapper(n_bins=256, random_state=seed).fit(X).bin_thresholds_
    got = mos.bin_thresholds(X, 255, seed)
    assert [len(t) for t in got] == [len(t) for t in ref]
    for a, b in zip(got, ref):
        assert a.tobytes() == np.asarray(b, dtype=np.float64).tobytes()
    other = mos.bin_thresholds(X, 255, seed + 1)
    assert other[0].tobytes() != got[0].tobytes(), "the subsample does not depend on the seed"


def test_stopping_rule():
    p = 16  # n_iter_no_change + 1
    flat = [-1.0] * p
    assert not mos.should_stop(flat[:p - 1], 15, 1e-7), "fewer than p scores never stop"
    assert mos.should_stop(flat, 15, 1e-7), "stops exactly at p scores"
    late = [-1.0] * (p - 1) + [-1.0 + 5e-8]
    assert mos.should_stop(late, 15, 1e-7), "an improvement within tol does not count"
    assert not mos.should_stop([-1.0] * (p - 1) + [-1.0 + 2e-7], 15, 1e-7)
    assert not mos.should_stop([-2.0] + [-1.0] * (p - 1), 15, 1e-7), "the window moved past the old score"
    assert mos.should_stop([-2.0] + [-1.0] * p, 15, 1e-7)
    assert mos.should_stop([-1.0, -1.0, -1.0], 2, None) and not mos.should_stop([-1.0, -1.0], 2, None)


def test_stopping_rule_on_sklearn_scores(gold):
    for tag in ("t1", "t2"):
        sc = gold[f"{tag}_es_validation_score"].tolist()
        n_iter = int(gold[f"{tag}_es_n_iter"])
        assert len(sc) == n_iter + 1
        assert [k for k in range(1, n_iter + 1) if mos.should_stop(sc[:k + 1], 15, 1e-7)] == [n_iter]


def _bf_inputs(gold):
    times = [datetime.strptime(str(t), "%Y-%m-%dT%H") for t in gold["bf_time"]]
    cols = ("era5_temperature_2m", "era5_dewpoint_2m", "era5_windspeed_10m", "era5_winddirection_10m",
            "era5_surface_pressure", "era5_cloudcover", "era5_shortwave_radiation", "era5_precipitation")
    era5 = {c: gold["bf_era5"][:, i] for i, c in enumerate(cols)}
    lat, lon, elev = gold["bf_site"]
    return times, era5, gold["bf_station"], {"lat": float(lat), "lon": float(lon), "elev": float(elev)}


def test_training_table_matches_reference(gold):
    times, era5, station_obs, site = _bf_inputs(gold)
    X, bias, kept = mos.training_table(times, era5, station_obs, site)
    assert list(mos.FEATURE_COLUMNS) == [str(c) for c in gold["bf_columns"]] and mos.NUM_FEATURES == 20
    assert kept == [times[i] for i in gold["bf_rows"]]
    assert X.dtype == np.float64 and X.shape == gold["bf_X"].shape
    for f, name in enumerate(mos.FEATURE_COLUMNS):
        assert X[:, f].tobytes() == gold["bf_X"][:, f].tobytes(), name
    assert bias.tobytes() == gold["bf_bias"].tobytes()


def test_fit_mos_table_round_trips():
    t0 = datetime(2023, 1, 31, 21)
    times = [t0 + timedelta(hours=h) for h in range(96)] + [t0 + timedelta(days=365, hours=h) for h in range(48)]
    rng = np.random.default_rng(3)
    bias = rng.normal(1.0, 2.0, len(times))
    tab = mos.fit_mos_table(times, bias)
    for t in (times[0], times[5], times[100]):
        idx = [i for i, u in enumerate(times) if (u.month, u.hour) == (t.month, t.hour)]
        assert mos.get_t2m_bias(tab, t) == float(np.mean(bias[idx]))
    assert mos.get_t2m_bias(tab, datetime(2023, 7, 1, 0)) == 0.0
    assert all(isinstance(k, str) for k in tab["bias_table"]) and set(tab["bias_table"]) == {"1", "2"}


def test_hgb_ref_reproduces_sklearn_forest(gold):
    """The yardstick of the kernel tests: 30 iterations on table 1, structure and thresholds exact."""
    X, y = table(gold, "t1")
    nthr = gold["t1_it30_nthr"]
    th = [gold["t1_it30_thr"][f, :nthr[f]] for f in range(20)]
    res = hgb_ref.fit(X, y, th, 30)
    got, roots = hgb_ref.flatten(res["trees"])
    ref, ref_roots = gold_forest(gold, "t1_it30")
    assert len(got["value"]) == len(ref["value"])
    bad = hgb_ref.same_forest(got, roots, ref, ref_roots, rtol=1e-12)
    assert not bad, "\n".join(bad)
    assert np.float64(res["baseline"]).tobytes() == gold["t1_it30_forest_baseline"].tobytes()


def test_fit_argument_errors(gold):
    X, y = table(gold, "t1")
    bad = X.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        mos.fit_learned_mos(bad, y)
    bad[3, 4] = np.inf
    with pytest.raises(ValueError, match="NaN or inf"):
        mos.fit_learned_mos(bad, y)
    with pytest.raises(ValueError, match="33 features"):
        mos.fit_learned_mos(np.zeros((100, 33)), np.zeros(100))
    with pytest.raises(ValueError, match="validation row"):
        mos.fit_learned_mos(X, y, validation=(np.zeros((0, 20)), np.zeros(0)))
    with pytest.raises(ValueError, match="validation row"):
        mos.fit_learned_mos(X, y, validation_fraction=0.0)
    with pytest.raises(ValueError, match="rows of X"):
        mos.fit_learned_mos(X, y[:-1])
    with pytest.raises(ValueError, match="max_leaf_nodes"):
        mos.MOSFitter(max_leaf_nodes=1)


def test_forest_of_takes_a_device_fitted_bundle(gold, tmp_path):
    ref, roots = gold_forest(gold, "t1_it30")
    forest = mos.MOSForest(*(ref[k] for k in FOREST_KEYS), roots, float(gold["t1_it30_forest_baseline"]))
    assert mos._forest_of({"model": forest, "feature_columns": list(mos.FEATURE_COLUMNS)}) is forest
    path = str(tmp_path / "learned.npz")
    mos.save_learned_mos(path, forest, stations_trained=["029570"], period="2016-2024", test_mae=1.2345, n_train=1500)
    bundle = mos.load_learned_mos(path)
    assert bundle["feature_columns"] == list(mos.FEATURE_COLUMNS) and bundle["stations_trained"] == ["029570"]
    assert bundle["period"] == "2016-2024" and bundle["test_mae"] == 1.2345 and bundle["n_train"] == 1500
    back = mos._forest_of(bundle)
    for k in mos.MOSForest._FIELDS:
        assert np.array_equal(getattr(back, k), getattr(forest, k)), k
    assert back.baseline == forest.baseline and back.n_features == 20
    with pytest.raises(ValueError, match="npz"):
        mos.save_learned_mos(str(tmp_path / "learned.joblib"), forest)


# ======================================================================================================================
# GPU: the device fit against sklearn's forests
# ======================================================================================================================
@pytest.fixture(scope="module")
def fits(gold):
    """The device fits the GPU tests share: the early-stopping fit of both tables and table 1's 30 iterations."""
    out = {}
    for tag in ("t1", "t2"):
        out[f"{tag}_es"] = mos.fit_learned_mos(*table(gold, tag))
    out["t1_it30"] = mos.fit_learned_mos(*table(gold, "t1"), early_stopping=False, max_iter=30)
    return out


def assert_same_forest(forest, gold, prefix):
    got, roots = forest_arrays(forest)
    ref, ref_roots = gold_forest(gold, prefix)
    bad = hgb_ref.same_forest(got, roots, ref, ref_roots, rtol=1e-12)
    assert not bad, "\n".join(bad)
    assert np.float64(forest.baseline).tobytes() == gold[f"{prefix}_forest_baseline"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["t1", "t2"])
def test_early_stopping_fit_matches_sklearn(gold, fits, tag):
    fit = fits[f"{tag}_es"]
    assert fit.n_iter_ == int(gold[f"{tag}_es_n_iter"]) and fit.forest.num_trees == fit.n_iter_
    assert_thresholds(fit.bin_thresholds, gold, f"{tag}_es")
    assert np.array_equal(fit.train_rows, gold[f"{tag}_es_train_rows"])
    assert np.array_equal(fit.val_rows, gold[f"{tag}_es_val_rows"])
    assert_same_forest(fit.forest, gold, f"{tag}_es")
    ref = gold[f"{tag}_es_validation_score"]
    assert fit.validation_score_.shape == ref.shape and fit.validation_score_.dtype == np.float64
    rel = np.max(np.abs(fit.validation_score_ - ref) / np.abs(ref))
    print(f"{tag}: validation_score_ max rel err {rel:.3e}")
    assert rel <= 1e-12


@pytest.mark.gpu
def test_fixed_iterations_fit_matches_sklearn(gold, fits):
    fit = fits["t1_it30"]
    assert fit.n_iter_ == 30 and fit.validation_score_.size == 0 and fit.val_rows.size == 0
    assert_same_forest(fit.forest, gold, "t1_it30")
    idx = np.arange(fit.forest.num_nodes)
    sp = fit.forest.is_leaf == 0
    assert np.all(fit.forest.left[sp] > idx[sp]) and np.all(fit.forest.right[sp] > idx[sp])


def _bytes(fit):
    nodes, roots = fit.forest.to("cuda")
    return nodes.cpu().numpy().tobytes(), roots.cpu().numpy().tobytes(), fit.validation_score_.tobytes()


@pytest.mark.gpu
def test_two_fits_give_the_same_bytes(gold, fits):
    again = mos.fit_learned_mos(*table(gold, "t1"))
    assert _bytes(again) == _bytes(fits["t1_es"])


@pytest.mark.gpu
@pytest.mark.parametrize("check_every", [1, 500])
def test_check_every_gives_the_same_truncated_forest(gold, fits, check_every):
    """fits["t1_es"] read the scores every 16 iterations."""
    other = mos.fit_learned_mos(*table(gold, "t1"), check_every=check_every)
    assert other.n_iter_ == fits["t1_es"].n_iter_
    assert _bytes(other) == _bytes(fits["t1_es"])


@pytest.mark.gpu
def test_captured_and_eager_give_the_same_bytes(gold):
    X, y = table(gold, "t1")
    kw = dict(early_stopping=False, max_iter=8)
    fitter_g, fitter_e = mos.MOSFitter(**kw), mos.MOSFitter(**kw)
    g = fitter_g.fit(X, y, use_graph=True)
    e = fitter_e.fit(X, y, use_graph=False)
    assert fitter_g.launch_mode == "hipGraph replay" and fitter_e.launch_mode == "eager"
    assert _bytes(g) == _bytes(e)


@pytest.mark.gpu
def test_validation_override(gold):
    """validation=(X_val, y_val) with sklearn's own split rows reproduces the split fit."""
    X, y = table(gold, "t1")
    tr, va = gold["t1_es_train_rows"], gold["t1_es_val_rows"]
    fit = mos.fit_learned_mos(X[tr], y[tr], validation=(X[va], y[va]))
    assert fit.n_iter_ == int(gold["t1_es_n_iter"]) and fit.train_rows.size == tr.size
    assert_same_forest(fit.forest, gold, "t1_es")


@pytest.mark.gpu
def test_fitted_bundle_through_apply_learned_mos(gold, fits):
    """The device-fitted bundle and sklearn's forest (the fixture's arrays) correct a forecast to the same bits."""
    from test_mos import VARS, forecast, global_grid, stations  # the forecasts of tests/test_mos.py

    ref, roots = gold_forest(gold, "t1_es")
    sk = mos.MOSForest(*(ref[k] for k in FOREST_KEYS), roots, float(gold["t1_es_forest_baseline"]))
    lat, lon = global_grid()
    pred = torch.from_numpy(forecast(31, lat.size, 4, VARS)).cuda()
    times = [datetime(2024, 1, 15, 0) + timedelta(hours=6 * s) for s in range(4)]
    bundle = fits["t1_es"].bundle(period="fixture")
    outs = []
    for model in (bundle, sk):
        out, n = mos.apply_learned_mos_t2m(pred, VARS, model, lat, lon, times, stations=stations(), spatial_idw=True)
        outs.append((out.cpu().numpy(), n))
    assert outs[0][1] == outs[1][1] and outs[0][1] > 0
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=2e-5)  # leaf values agree to 1e-12, t2m is float32
    assert not np.array_equal(outs[0][0], pred.cpu().numpy())


@pytest.mark.gpu
def test_evaluate_learned_mos(gold, fits):
    X, y = table(gold, "t1")
    rows = gold["t1_es_val_rows"]
    times = [datetime(2024, 1, 1) + timedelta(hours=int(7 * i)) for i in range(rows.size)]
    tab = mos.fit_mos_table(times, y[rows])
    res = mos.evaluate_learned_mos(fits["t1_es"], X[rows], y[rows], times, table=tab)
    pred = fits["t1_es"].forest.predict_host(X[rows])
    assert res["n"] == rows.size
    assert abs(res["learned"]["mae"] - np.mean(np.abs(y[rows] - pred))) < 1e-12
    assert abs(res["learned"]["rmse"] - np.sqrt(np.mean((y[rows] - pred) ** 2))) < 1e-12
    assert res["raw"]["mae"] == float(np.mean(np.abs(y[rows])))
    assert res["learned"]["mae"] < res["raw"]["mae"]
    assert set(res["per_season"]) <= set(mos.SEASONS) and sum(v["n"] for v in res["per_season"].values()) == rows.size
    assert set(res["per_hour"]) <= set(range(0, 24, 3))
    # -0.5 mean squared error of the validation rows is the last early-stopping score
    assert abs(-0.5 * res["learned"]["rmse"] ** 2 - fits["t1_es"].validation_score_[-1]) < 1e-12
