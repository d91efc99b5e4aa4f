"""Generate the fixtures of the learned-MOS fit by RUNNING sklearn's `HistGradientBoostingRegressor` with the
hyper-parameters of the reference's `scripts/build_learned_mos.py:357-367`, and the reference's own `build_features` /
`solar_elevation` on a small table (sklearn, pandas, numpy).

Run from the repo root, only where the reference checkout (`make_golden.REF`), sklearn and pandas exist (never on the GPU
box):

    python tests/golden/make_mos_fit_golden.py

Output (data only - arrays and names, no reference source text): tests/golden/mos_fit_vectors.npz
  t<k>_X, t<k>_y             fitting table k (1: 1 500 rows, 2: 3 000 rows; 20 features; values rounded to float32): one
                             constant feature (17), one with 41 distinct values (6), one with many repeated zeros (8),
                             the rest continuous
  t<k>_es_*                  the early-stopping fit with the reference's hyper-parameters: thr / nthr (the bin
                             thresholds [20, 255] and their counts), train_rows / val_rows, baseline, n_iter,
                             validation_score, forest_* (the `MOSForest.from_sklearn` arrays)
  t<k>_it30_*                `early_stopping=False, max_iter=30` on all rows: thr / nthr, baseline, forest_*
  bf_*                       a `build_features` pair: the input columns (bf_time as "YYYY-mm-ddTHH" strings, bf_era5
                             [n, 8], bf_station), the station (bf_site = lat, lon, elev), and what the reference's row
                             filters (:313-315, :332) and build_features leave: bf_X [m, 20], bf_bias, bf_rows (indices
                             of the kept rows)

The generator asserts what makes the fixture a fair yardstick, and fails otherwise:
  (a) fitting a row-permuted copy of each table gives the identical forest, so the float64 sums are exact at this size
      and the order of summation cannot decide a split;
  (b) no two splittable leaves of one tree ever hold equal gains, so sklearn's heap order never decides.
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import hgb_ref  # noqa: E402
import make_golden  # noqa: E402  (where the reference checkout lives)
from make_mos_golden import flatten  # noqa: E402

REF = make_golden.REF
HYPER = dict(max_iter=500, max_depth=8, learning_rate=0.05, min_samples_leaf=20, l2_regularization=0.1,
             early_stopping=True, validation_fraction=0.1, n_iter_no_change=15, random_state=42)
ERA5 = ["era5_temperature_2m", "era5_dewpoint_2m", "era5_windspeed_10m", "era5_winddirection_10m",
        "era5_surface_pressure", "era5_cloudcover", "era5_shortwave_radiation", "era5_precipitation"]


def table(n, seed):
    """A MOS-like table: (X [n, 20], y [n]) with float32-representable values."""
    rng = np.random.default_rng(seed)
    hour = rng.integers(0, 24, n)
    doy = rng.integers(1, 366, n)
    t2m = rng.normal(0, 15, n)
    X = np.column_stack([
        t2m, t2m - rng.gamma(2, 2, n), rng.gamma(2, 2, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.normal(990, 15, n), np.round(rng.uniform(0, 100, n) / 2.5) * 2.5, rng.uniform(0, 600, n),
        np.where(rng.random(n) < 0.7, 0.0, rng.exponential(0.5, n)), np.sin(2 * np.pi * hour / 24),
        np.cos(2 * np.pi * hour / 24), np.sin(2 * np.pi * doy / 365.25), np.cos(2 * np.pi * doy / 365.25),
        rng.uniform(-60, 60, n), rng.gamma(2, 2, n), t2m + rng.normal(0, 3, n), rng.normal(0, 3, n),
        np.full(n, 56.017), rng.uniform(89, 96, n), rng.uniform(90, 480, n)])
    y = (0.08 * X[:, 0] - 1.5 * X[:, 10] + 0.004 * X[:, 7] * (X[:, 13] > 0) - 0.3 * np.tanh(X[:, 16])
         + 0.5 * (X[:, 8] > 0) + rng.normal(0, 0.8, n))
    return X.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)


def thresholds_of(model):
    th = model._bin_mapper.bin_thresholds_
    thr = np.zeros((len(th), 255))
    for f, t in enumerate(th):
        thr[f, :len(t)] = t
    return thr, np.array([len(t) for t in th], dtype=np.int32)


def same(a, b):
    fa, fb = flatten(a), flatten(b)
    return all(np.array_equal(fa[k], fb[k]) for k in fa)


def check_distinct_gains(X, y, model, what):
    """(b): replay the fit with the numpy restatement and look at every gain that entered the heap."""
    th = model._bin_mapper.bin_thresholds_
    bins = hgb_ref.bin_rows(X, th)
    nthr = [len(t) for t in th]
    raw = np.full(y.shape, float(np.mean(y)))
    for it in range(model.n_iter_):
        gains = []
        _, leaves = hgb_ref.grow_tree(bins, nthr, th, hgb_ref.gradients(raw, y), gains=gains)
        assert len(set(gains)) == len(gains), f"{what}: equal gains among the splittable leaves of tree {it}"
        for rows, v in leaves:
            raw[rows] += v


def fit_table(out, tag, X, y, seed):
    from sklearn.ensemble import HistGradientBoostingRegressor as HGB

    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(y))
    for name, kw in (("es", HYPER), ("it30", {**HYPER, "early_stopping": False, "max_iter": 30})):
        model = HGB(**kw).fit(X, y)
        if name == "es":  # sklearn shuffles itself: the permuted copy is given the same training rows in another order
            s = int(np.random.RandomState(42).randint(np.iinfo(np.uint32).max, dtype="u8"))
            p = np.random.RandomState(s).permutation(len(y))
            nv = int(np.ceil(0.1 * len(y)))
            val, train = p[:nv], p[nv:nv + int(np.floor(0.9 * len(y)))]
            plain = HGB(**{**kw, "early_stopping": False, "max_iter": model.n_iter_}).fit(X[train], y[train])
            assert same(plain, model), f"{tag}: the restated split does not reproduce the early-stopping fit"
            tp = rng.permutation(train)
            other = HGB(**{**kw, "early_stopping": False, "max_iter": model.n_iter_}).fit(X[tp], y[tp])
            check_distinct_gains(X[train], y[train], model, f"{tag}_{name}")
            out[f"{tag}_es_train_rows"], out[f"{tag}_es_val_rows"] = train.astype(np.int32), val.astype(np.int32)
            out[f"{tag}_es_n_iter"] = np.int32(model.n_iter_)
            out[f"{tag}_es_validation_score"] = np.asarray(model.validation_score_, dtype=np.float64)
        else:
            other = HGB(**kw).fit(X[perm], y[perm])
            check_distinct_gains(X, y, model, f"{tag}_{name}")
        assert same(other, model), f"{tag}_{name}: a row-permuted copy fits another forest (choose another seed)"
        thr, nthr = thresholds_of(model)
        out[f"{tag}_{name}_thr"], out[f"{tag}_{name}_nthr"] = thr, nthr
        for k, v in flatten(model).items():
            out[f"{tag}_{name}_{k}"] = v
        print(f"{tag}_{name}: {model.n_iter_} iterations, {len(out[f'{tag}_{name}_forest_value'])} nodes")


def _ref_script():
    spec = importlib.util.spec_from_file_location("_ref_blm", os.path.join(REF, "scripts", "build_learned_mos.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_features_pair(out):
    import pandas as pd

    ref = _ref_script()
    rng = np.random.default_rng(7)
    n = 72
    time = pd.date_range("2023-12-30 00:00", periods=n, freq="h")
    era5 = np.column_stack([rng.normal(-12, 6, n), rng.normal(-16, 6, n), rng.gamma(2, 2, n), rng.uniform(0, 360, n),
                            rng.normal(990, 10, n), rng.uniform(0, 100, n), rng.uniform(0, 300, n),
                            rng.exponential(0.2, n)])
    station = era5[:, 0] + rng.normal(1.0, 2.0, n)
    era5[[5, 40], 0] = np.nan      # no t2m
    station[[9, 10, 33]] = np.nan  # no observation
    station[20] += 30.0            # |bias| >= 20
    era5[50, 1] = np.nan           # a NaN feature (dropped after the lag is taken)
    lat, lon, elev = 56.017, 92.750, 277
    df = pd.DataFrame({"time": time, **{c: era5[:, i] for i, c in enumerate(ERA5)}, "station_t2m_C": station})
    df["row"] = np.arange(n)
    # the reference's row filters, :313-315 and :332, around its build_features
    df = df.dropna(subset=["era5_temperature_2m", "station_t2m_C"])
    df["bias"] = df["station_t2m_C"] - df["era5_temperature_2m"]
    df = df[df["bias"].abs() < 20.0]
    df = ref.build_features(df, lat, lon, elev)
    df = df.dropna(subset=ref.FEATURE_COLUMNS + ["bias"])
    out["bf_time"] = np.array([t.strftime("%Y-%m-%dT%H") for t in time])
    out["bf_era5"], out["bf_station"] = era5, station
    out["bf_site"] = np.array([lat, lon, elev], dtype=np.float64)
    out["bf_X"] = df[ref.FEATURE_COLUMNS].values.astype(np.float64)
    out["bf_bias"] = df["bias"].values.astype(np.float64)
    out["bf_rows"] = df["row"].values.astype(np.int32)
    out["bf_columns"] = np.array(ref.FEATURE_COLUMNS)
    assert len(out["bf_rows"]) < n - 6


def main():
    warnings.filterwarnings("ignore")
    out = {}
    for tag, n, seed in (("t1", 1500, 101), ("t2", 3000, 202)):
        X, y = table(n, seed)
        out[f"{tag}_X"], out[f"{tag}_y"] = X.astype(np.float32), y.astype(np.float32)
        fit_table(out, tag, X, y, seed + 1)
    build_features_pair(out)
    path = os.path.join(HERE, "mos_fit_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
