"""Generate the MOS fixtures by RUNNING the reference's own `src/postprocessing/mos_correction.py` on the shipped
learned-MOS bundle (sklearn, joblib, numpy).

Run from the repo root, only where the reference checkout (`make_golden.REF`) and sklearn exist (never on the GPU box):

    python tests/golden/make_mos_golden.py

Output (data only - arrays, no reference source text): tests/golden/mos_vectors.npz
  forest_*        the bundle's HistGradientBoostingRegressor flattened (global child indices; leaves hold the value,
                  splits the threshold), forest_baseline
  pred_X, pred_y  sklearn `predict` on feature rows with NaN features, values exactly on thresholds, +-1e30
  <case>_out      the corrected t2m column [G, steps] of apply_learned_mos_t2m, <case>_n the n_corrected,
  <case>_feat     every feature row the reference handed to `predict`, in call order (group, step, station),
  <case>_bias     the `predict` results in the same order, <case>_field the IDW bias field [G, steps] (IDW cases)
                  Cases: a (default station, 64 x 32 global grid), b (the 19 MOS stations, station-only, 64 x 32), c
                  (IDW, power 2, 300 km, 41 x 61 0.25 deg box, float32 coordinates), d (IDW, power 1.5, 150 km), e
                  (10u / 10v, no sp / tp), g (float64 forecast), h1 / h2 (valid times across a year end / a leap
                  day).  The forecasts come from `forecast()` below (seeded numpy), which tests/test_mos.py restates.
  table_*         apply_mos_t2m with a synthetic table that misses months and hours (float32 and float64)
"""
import importlib.util
import os
import sys
import warnings
from datetime import datetime, timedelta

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (where the reference checkout lives)

REF = make_golden.REF

STATIONS = [  # scripts/mos_idw_sweep_v2.py MOS_STATIONS
    (56.173, 92.493, 287), (56.283, 90.517, 257), (56.200, 95.633, 207), (53.740, 91.385, 253),
    (57.683, 93.267, 93), (56.900, 93.133, 180), (56.967, 90.683, 181), (56.500, 93.283, 164),
    (56.217, 89.550, 290), (56.067, 92.733, 235), (56.117, 92.200, 479), (55.933, 92.283, 275),
    (57.633, 92.267, 179), (57.200, 94.550, 168), (56.650, 90.550, 231), (56.850, 95.217, 188),
    (56.033, 90.317, 256), (56.100, 91.667, 332), (56.167, 95.267, 357)]
VARS = ["t2m", "u10", "v10", "msl", "tp", "sp", "tcwv", "z_surf", "lsm"]
VARS_E = ["10u", "t2m", "10v", "msl", "tcwv"]
STEPS = 4


def stations():
    return [{"lat": a, "lon": o, "elev": e, "name": f"s{i}"} for i, (a, o, e) in enumerate(STATIONS)]


def global_grid(nlon=64, nlat=32, dtype=np.float64):
    """Per-node coordinates of the regular global grid, longitude-major (node = j * nlat + i)."""
    lats = np.linspace(-90, 90, nlat, endpoint=True)
    lons = np.linspace(0, 360, nlon, endpoint=False)
    return np.tile(lats, nlon).astype(dtype), np.repeat(lons, nlat).astype(dtype)


def box_grid(dtype=np.float32):
    """The 41 x 61 0.25 deg box 50-60N x 85-100E, longitude-major."""
    lats = 50.0 + 0.25 * np.arange(41)
    lons = 85.0 + 0.25 * np.arange(61)
    return np.tile(lats, 61).astype(dtype), np.repeat(lons, 41).astype(dtype)


def forecast(seed, G, steps, var_order, dtype=np.float32):
    """Seeded synthetic forecast [G, steps, C] in physical units."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((G, steps, len(var_order)))
    for c, name in enumerate(var_order):
        if name == "t2m":
            x[..., c] = 265.0 + 15.0 * x[..., c]
        elif name in ("u10", "10u", "v10", "10v"):
            x[..., c] = 6.0 * x[..., c]
        elif name == "sp":
            x[..., c] = 95000.0 + 3000.0 * x[..., c]
        elif name == "tp":
            x[..., c] = 1e-3 * np.abs(x[..., c])
    return x.astype(dtype)


def valid_times(start, steps=STEPS):
    return [start + timedelta(hours=6 * s) for s in range(steps)]


def _ref_mos():
    spec = importlib.util.spec_from_file_location(
        "_ref_mos", os.path.join(REF, "src", "postprocessing", "mos_correction.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    """Stands in for the model: records every feature row and prediction of the reference's loop."""

    def __init__(self, model):
        self.model, self.X, self.y = model, [], []

    def predict(self, X):
        y = self.model.predict(X)
        self.X.append(np.array(X[0]))
        self.y.append(float(y[0]))
        return y


def flatten(model):
    feat, val, left, right, miss, leaf, roots = [], [], [], [], [], [], []
    off = 0
    for it in model._predictors:
        n = it[0].nodes
        lf = n["is_leaf"].astype(bool)
        roots.append(off)
        feat.append(np.where(lf, 0, n["feature_idx"]))
        val.append(np.where(lf, n["value"], n["num_threshold"]))
        left.append(np.where(lf, 0, n["left"].astype(np.int64) + off))
        right.append(np.where(lf, 0, n["right"].astype(np.int64) + off))
        miss.append(n["missing_go_to_left"])
        leaf.append(lf)
        off += len(n)
    return {"forest_feature": np.concatenate(feat).astype(np.int8),
            "forest_value": np.concatenate(val).astype(np.float64),
            "forest_left": np.concatenate(left).astype(np.int32),
            "forest_right": np.concatenate(right).astype(np.int32),
            "forest_missing_left": np.concatenate(miss).astype(np.uint8),
            "forest_is_leaf": np.concatenate(leaf).astype(np.uint8),
            "forest_roots": np.asarray(roots, dtype=np.int32),
            "forest_baseline": np.float64(np.ravel(model._baseline_prediction)[0])}


def predict_rows(model, fl, rng):
    """~200 feature rows: plausible values, NaNs, values exactly on split thresholds, +-1e30."""
    n = 200
    X = np.column_stack([
        rng.normal(0, 15, n), rng.normal(-5, 10, n), rng.gamma(2, 2, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.normal(990, 15, n), rng.uniform(0, 100, n), rng.uniform(0, 600, n), rng.exponential(0.3, n),
        rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.uniform(-60, 60, n), rng.gamma(2, 2, n), rng.normal(0, 15, n), rng.normal(0, 3, n),
        rng.uniform(53, 58, n), rng.uniform(89, 96, n), rng.uniform(90, 480, n)])
    X[rng.random(X.shape) < 0.15] = np.nan
    X[:, [1, 6, 7, 14]] = np.where(rng.random((n, 4)) < 0.7, np.nan, X[:, [1, 6, 7, 14]])
    split = np.nonzero(fl["forest_is_leaf"] == 0)[0]
    for r in range(40, 120):  # every feature of these rows sits exactly on some split threshold of that feature
        for f in range(20):
            cand = split[fl["forest_feature"][split] == f]
            if cand.size:
                X[r, f] = fl["forest_value"][cand[rng.integers(cand.size)]]
    X[120:140] = np.where(rng.random((20, 20)) < 0.5, 1e30, -1e30)
    X[140:150] = np.nan
    return X, model.predict(X)


def check_wind_margin(feat, fl):
    """No wind-direction feature within 1e-9 of a threshold on that feature: a one-ulp device difference in sin / cos
    then cannot flip a split."""
    split = fl["forest_is_leaf"] == 0
    for f in (3, 4):
        th = fl["forest_value"][split & (fl["forest_feature"] == f)]
        x = feat[:, f]
        x = x[~np.isnan(x)]
        if th.size and x.size:
            assert np.min(np.abs(x[:, None] - th[None, :])) > 1e-9, f"wind feature {f} on a threshold"


def main():
    warnings.filterwarnings("ignore")
    ref = _ref_mos()
    bundle = ref.load_learned_mos(os.path.join(REF, "live_runtime_bundle", "learned_mos_t2m.joblib"))
    model = bundle["model"]
    out = flatten(model)
    rng = np.random.default_rng(2026)
    out["pred_X"], out["pred_y"] = predict_rows(model, out, rng)

    t0 = datetime(2024, 1, 15, 0)
    cases = {  # name: (coords, var_order, dtype, stations, idw, power, radius, start, seed)
        "a": (global_grid(), VARS, np.float32, None, False, 2.0, 300.0, t0, 11),
        "b": (global_grid(), VARS, np.float32, stations(), False, 2.0, 300.0, t0, 12),
        "c": (box_grid(), VARS, np.float32, stations(), True, 2.0, 300.0, datetime(2024, 7, 1, 6), 13),
        "d": (box_grid(), VARS, np.float32, stations(), True, 1.5, 150.0, datetime(2024, 7, 1, 6), 14),
        "e": (global_grid(), VARS_E, np.float32, stations(), False, 2.0, 300.0, t0, 15),
        "g": (global_grid(), VARS, np.float64, stations(), False, 2.0, 300.0, t0, 16),
        "h1": (box_grid(), VARS, np.float32, stations(), False, 2.0, 300.0, datetime(2023, 12, 31, 6), 17),
        "h2": (box_grid(), VARS, np.float32, stations(), False, 2.0, 300.0, datetime(2024, 2, 28, 12), 18),
    }
    fields = {}
    real_idw = ref._idw_interpolate_bias

    def idw_recorder(*a, **k):
        f = real_idw(*a, **k)
        fields["last"] = f
        return f
    ref._idw_interpolate_bias = idw_recorder
    for name, (coords, vo, dt, sts, idw, pw, rad, start, seed) in cases.items():
        lat, lon = coords
        steps = 8 if name.startswith("h") else STEPS
        pred = forecast(seed, lat.size, steps, vo, dt)
        rec = Recorder(model)
        fields.clear()
        kw = {} if sts is None else {"stations": sts}
        corrected, n = ref.apply_learned_mos_t2m(pred, vo, {"model": rec}, lat, lon, valid_times(start, steps),
                                                 spatial_idw=idw, idw_power=pw, idw_max_radius_km=rad, **kw)
        feat = np.array(rec.X)
        check_wind_margin(feat, out)
        out[f"{name}_out"] = corrected[:, :, vo.index("t2m")]
        out[f"{name}_n"] = np.int64(n)
        out[f"{name}_feat"] = feat
        out[f"{name}_bias"] = np.array(rec.y)
        if idw:
            out[f"{name}_field"] = fields["last"]
    ref._idw_interpolate_bias = real_idw

    table = {"bias_table": {"1": {"0": -1.25, "6": 0.7312345678901234, "18": 2}, "2": {"12": -0.1},
                            "12": {"0": 0.333333333333, "6": -2.5, "12": 1e-7}}}
    times = [datetime(2023, 12, 31, 0) + timedelta(hours=6 * s) for s in range(10)]
    times += [datetime(2024, 2, 29, 12), datetime(2024, 3, 1, 0)]
    for dt, tag in ((np.float32, "f32"), (np.float64, "f64")):
        pred = forecast(21, 300, len(times) + 2, VARS, dt)
        out[f"table_{tag}_out"] = ref.apply_mos_t2m(pred, VARS, table, times)[:, :, 0]
    out["table_biases"] = np.array([ref.get_t2m_bias(table, t) for t in times], dtype=np.float64)

    path = os.path.join(HERE, "mos_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
