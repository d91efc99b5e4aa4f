"""Generate the WRF-benchmark fixtures by RUNNING the reference's own `scripts/compare_wrf_era5.py` and
`scripts/compare_wrf.py` (numpy, scipy, torch on the CPU).

Run from the repo root, only where the reference checkout (`make_golden.REF`) and scipy exist (never on the GPU box):

    python tests/golden/make_wrf_golden.py

Output (data only - arrays and recorded text, no reference source text):
  tests/golden/wrf_case.json     a WRF JSON export: 12 x 10 curvilinear grid (perturbed, not separable), 25 hourly steps
                                 from 2023-01-20_00:00:00, `domain_fields`, `domain_mean`, `domain`
  tests/golden/wrf_vectors.npz
    interp                 `interpolate_era5_to_wrf` of every mapped variable x matched step [4, 5, 12, 10] (float64)
    interp_f32             the same function on a float32 field (series[8, :, :, 0] * 1.5)
    era5_results           compare_wrf_era5's `compute_metrics` per variable x step [4, 5, 3]
    era5_text              stdout of compare_wrf_era5.main() from the per-variable block on
    match_steps            (era5 index, WRF hourly index) of the matched steps
    wrf_means_25 / _7 / _3 `_load_wrf_json` of the full export and of its first 7 / 3 hourly steps [4, n]
    region_regular / _flat the region rows `load_predictions_and_truth` picks (read off an index-valued forecast)
    match_<list>           `_find_wrf_matching_sample` for the three offset lists (-1: None)
    match_formats          the same for every `time_start` format of wrf_case.TIME_FORMATS (list "match")
    <kind>_pred_mean, <kind>_truth_mean   `load_predictions_and_truth(...)` then `.mean(axis=1)` for kind in regular,
                           flat, legacy
    text_<kind>_<list>     stdout of compare_wrf.main() from "OUR MODEL metrics" on
    grid_sums              [3, P, 4, 6]: n, sum d, sum d^2, sum |d|, sum a, sum b of the reference's own
                           `interpolate_era5_to_wrf` applied to the denormalised forecast / truth of the regular
                           bundle, by numpy in float64: forecast vs truth over all samples, forecast vs WRF and WRF vs
                           truth for the matching sample
    grid_mags              [3, P, 4, 6]: the sums of the magnitudes of the same terms (what the bound is taken against)
    grid_metrics           [3, P, 4, 3]: the reference's `compute_metrics` on the matching sample's fields
The seeded inputs live in tests/helpers/wrf_case.py, which the tests use as well.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402  (where the reference checkout lives)
import wrf_case as WC  # noqa: E402

REF = make_golden.REF
WRF_SEED = 0  # the first seed that passes check_placement() and the margin check in era5_section()
KEYS = ("t2_K", "u10_ms", "v10_ms", "psfc_Pa")
OURS = ("t2m", "10u", "10v", "sp")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def wrf_export(seed):
    """The WRF JSON: edge rows and columns straddle the ERA5 axes (90-96 E, 54-58 N), one point sits exactly on the last
    longitude node and one on the last latitude node, and about 3 % of u10 is NaN."""
    rng = np.random.default_rng(seed)
    lon = np.tile(np.linspace(89.95, 96.05, 10), (12, 1)) + rng.uniform(-0.1, 0.1, (12, 10))
    lat = np.tile(np.linspace(53.95, 58.05, 12)[:, None], (1, 10)) + rng.uniform(-0.1, 0.1, (12, 10))
    lon[5, 9], lat[11, 4] = 96.0, 58.0
    lon, lat = np.round(lon, 4), np.round(lat, 4)
    times = ["2023-01-%02d_%02d:00:00" % (20 + h // 24, h % 24) for h in range(25)]
    base = {"t2_K": (258.0, 6.0), "u10_ms": (1.0, 3.0), "v10_ms": (-0.5, 3.0), "psfc_Pa": (98300.0, 600.0)}
    fields, means = {}, {}
    for k, (c, s) in base.items():
        x = c + s * (0.5 * np.sin(lon / 1.7) + 0.5 * np.cos(lat / 1.3))[None] + 0.3 * s * rng.standard_normal((25, 12, 10))
        x = np.round(x, 1 if k == "psfc_Pa" else 2)
        if k == "u10_ms":
            x[rng.random(x.shape) < 0.03] = np.nan
        fields[k] = x
        means[k] = [round(float(np.nanmean(x[t])), 3) for t in range(25)]
    return {"domain": {"lat_min": float(lat.min()), "lat_max": float(lat.max()), "lon_min": float(lon.min()),
                       "lon_max": float(lon.max())},
            "times": times, "lat": lat.tolist(), "lon": lon.tolist(),
            "domain_fields": {k: v.tolist() for k, v in fields.items()}, "domain_mean": means}


def check_placement(export):
    lons, lats = WC.axes()
    lon, lat = np.array(export["lon"], dtype=np.float32), np.array(export["lat"], dtype=np.float32)
    sides = {"west": lon < lons[0], "east": lon > lons[-1], "south": lat < lats[0], "north": lat > lats[-1]}
    outside = sides["west"] | sides["east"] | sides["south"] | sides["north"]
    frac = outside.mean()
    print("outside the ERA5 axes: %.1f %% (%s)" % (100 * frac, ", ".join(f"{k} {int(v.sum())}" for k, v in sides.items())))
    assert all(v.sum() >= 3 for v in sides.values()), "every side must have points outside"
    assert 0.15 <= frac <= 0.25, frac
    assert lon[5, 9] == np.float32(lons[-1]) and not outside[5, 9]
    assert lat[11, 4] == np.float32(lats[-1]) and not outside[11, 4]
    u = np.array(export["domain_fields"]["u10_ms"], dtype=np.float32)
    nan_frac = np.isnan(u).mean()
    assert 0.02 <= nan_frac <= 0.04, nan_frac
    keep = (~outside[None] & ~np.isnan(u)).reshape(25, -1).sum(axis=1)
    assert keep.min() >= 60, "every job must keep at least half of its 120 points"


def margin_ok(x, decimals, eps):
    """x is more than eps from a rounding boundary of its printed decimals."""
    return abs(abs(x) * 10.0 ** decimals % 1.0 - 0.5) > eps * 10.0 ** decimals


def era5_section(era5, out, tmp):
    data_dir = WC.dataset_dir(Path(tmp) / "era5")
    fields, wlat, wlon, times, _ = silent(era5.load_wrf_json, WC.WRF_JSON)
    data, lons, lats, names, info = silent(era5.load_era5, data_dir)
    base = 8
    interp = np.zeros((4, 5, 12, 10))
    res = np.zeros((4, 5, 3))
    for a, (k, v) in enumerate(era5.VAR_MAP.items()):
        vi = names.index(v["era5"])
        for h in range(5):
            f = era5.interpolate_era5_to_wrf(data[base + h, :, :, vi].astype(np.float32), lons, lats, wlat, wlon)
            interp[a, h] = f
            conv = fields[k][h * 6] * v["era5_to_wrf"]
            res[a, h] = era5.compute_metrics(conv, f)
            assert (~(np.isnan(conv) | np.isnan(f))).sum() >= 60
            # the printed digits must not hinge on the order of a float64 sum: the bound on two orders of 120 terms is
            # below 1e-9 here, the margin asked for 1e-6
            for x, d in ((res[a, h, 0], 3), (res[a, h, 1], 3), (res[a, h, 2], 3), (np.nanmean(conv), 1),
                         (np.nanmean(f), 1)):
                assert margin_ok(float(x), d, 1e-6), "a printed number sits on a rounding boundary; change WRF_SEED"
        assert margin_ok(float(np.mean(res[a, 1:, 0])), 3, 1e-6), "change WRF_SEED"
    out["interp"], out["era5_results"] = interp, res
    out["interp_f32"] = era5.interpolate_era5_to_wrf(data[8, :, :, 0].astype(np.float32) * np.float32(1.5), lons, lats,
                                                     wlat, wlon)
    out["match_steps"] = np.array([(base + h, 6 * h) for h in range(5)])
    text = run_main(era5, ["--wrf-json", WC.WRF_JSON, "--era5-dir", str(data_dir)])
    out["era5_text"] = np.array(text[text.index("\n" + "=" * 75):])
    return interp, fields, wlat, wlon


def silent(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def run_main(mod, argv):
    buf = io.StringIO()
    old = sys.argv
    sys.argv = ["x"] + argv
    try:
        with contextlib.redirect_stdout(buf):
            mod.main()
    finally:
        sys.argv = old
    return buf.getvalue()


def cut_sections(text):
    """stdout of compare_wrf.main() from the all-sample block on, without what load_wrf and the first date matching
    print between the blocks."""
    i = text.index("\n" + "=" * 70 + "\nOUR MODEL metrics")
    j = text.index("\nWRF dataset (JSON):")
    marks = [text.find("\n" + "=" * 70 + "\nWRF vs ERA5 vs Ours"), text.find("\nWARNING: Could not find")]
    k = min(m for m in marks if m >= 0)
    return text[i:j] + text[k:]


def main():
    make_golden._placeholders()
    era5 = _load(os.path.join(REF, "scripts", "compare_wrf_era5.py"), "_ref_wrf_era5")
    cw = _load(os.path.join(REF, "scripts", "compare_wrf.py"), "_ref_wrf")
    out = {}
    export = wrf_export(WRF_SEED)
    check_placement(export)
    Path(WC.WRF_JSON).write_text(json.dumps(export, separators=(",", ":")))
    # the perturbed grid is not separable: no row shares its longitudes with another
    assert len({tuple(r) for r in export["lon"]}) == 12

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        interp, wfields, wlat, wlon = era5_section(era5, out, tmp)

        # --- _load_wrf_json: the 25 / 7 / 3 step rules -----------------------------------------------------------------
        for n in (25, 7, 3):
            path = WC.WRF_JSON if n == 25 else WC.shortened_wrf(tmp / f"wrf{n}.json", n)
            wd = silent(cw._load_wrf_json, str(path), WC.P)
            out[f"wrf_means_{n}"] = np.stack([wd[o] for o in OURS])
            assert out[f"wrf_means_{n}"].dtype == np.float32

        # --- region rows, read off a forecast whose value is its row number ---------------------------------------------
        for kind, flat in (("regular", False), ("flat", True)):
            d = WC.dataset_dir(tmp / f"ident_{kind}", flat=flat, identity=True)
            idx = torch.arange(425, dtype=torch.float32)[None, :, None].expand(1, 425, WC.P * WC.C).contiguous()
            torch.save({"predictions": idx, "ground_truth": idx, "n_features": WC.C}, tmp / "idx.pt")
            pr, _, _, _, _ = silent(cw.load_predictions_and_truth, d, tmp / "idx.pt", tmp, WC.P)
            out[f"region_{kind}"] = pr[0, :, 0, 0].astype(np.int64)
            assert out[f"region_{kind}"].size == 45

        # --- the matching sample -------------------------------------------------------------------------------------------
        reg = WC.dataset_dir(tmp / "regular")
        flat = WC.dataset_dir(tmp / "flat", flat=True)
        for name, offs in WC.OFFSETS.items():
            r = silent(cw._find_wrf_matching_sample, reg, WC.WRF_JSON, offs, WC.OBS, WC.P)
            out[f"match_{name}"] = np.int64(-1 if r is None else r)
        assert (out["match_match"], out["match_plus2"], out["match_none"]) == (2, 4, -1)
        fm = []
        for ts in WC.TIME_FORMATS:
            d = WC.dataset_dir(tmp / "fmt", time_start=ts if ts else None, with_series=False)
            r = silent(cw._find_wrf_matching_sample, d, WC.WRF_JSON, WC.OFFSETS["match"], WC.OBS, WC.P)
            fm.append(-1 if r is None else r)
        out["match_formats"] = np.array(fm, dtype=np.int64)

        # --- means and tables -----------------------------------------------------------------------------------------------
        for kind, d, is_flat, legacy in (("regular", reg, False, False), ("flat", flat, True, False),
                                         ("legacy", reg, False, True)):
            for lname, offs in WC.OFFSETS.items():
                if kind != "regular" and lname != "match":
                    continue
                pt = tmp / f"pred_{kind}_{lname}.pt"
                torch.save(WC.bundle(is_flat, offs, legacy), pt)
                if lname == "match":
                    pr, tr, names, P, n = silent(cw.load_predictions_and_truth, d, pt, tmp, WC.P)
                    out[f"{kind}_pred_mean"], out[f"{kind}_truth_mean"] = pr.mean(axis=1), tr.mean(axis=1)
                    assert pr.dtype == np.float32 and pr.shape[1] == 45
                text = run_main(cw, ["--predictions", str(pt), "--data-dir", str(d), "--wrf-path", WC.WRF_JSON,
                                     "--experiment-dir", str(tmp), "--ar-steps", str(WC.P)])
                out[f"text_{kind}_{lname}"] = np.array(cut_sections(text))

        # --- field-level scores on the WRF grid (regular bundle, list "match") ------------------------------------------
        mean, std = WC.scalers()
        pred, truth = WC.predictions()
        lons, lats = WC.axes()
        lats32, lons32 = (a.astype(np.float32).astype(np.float64) for a in (lats, lons))
        phys = [(x.reshape(WC.N_SAMPLES, 425, WC.P, WC.C) * std[None, None, None, :WC.C] + mean[None, None, None, :WC.C])
                for x in (pred, truth)]
        assert phys[0].dtype == np.float32
        si = int(out["match_match"])
        sums = np.zeros((3, WC.P, 4, 2, 6))
        mets = np.zeros((3, WC.P, 4, 3))

        def six(a, b):
            m = ~(np.isnan(a) | np.isnan(b))
            d = a[m] - b[m]
            return np.array([[m.sum(), d.sum(), (d * d).sum(), np.abs(d).sum(), a[m].sum(), b[m].sum()],
                             [0.0, np.abs(d).sum(), (d * d).sum(), np.abs(d).sum(), np.abs(a[m]).sum(),
                              np.abs(b[m]).sum()]], dtype=np.float64)

        for v, (k, name) in enumerate(zip(KEYS, OURS)):
            vi = WC.VAR_NAMES.index(name)
            for h in range(WC.P):
                wrf = wfields[k][(h + 1) * 6] * era5.VAR_MAP[k]["era5_to_wrf"]
                for s in range(WC.N_SAMPLES):
                    f, t = (era5.interpolate_era5_to_wrf(np.ascontiguousarray(x[s, :, h, vi]).reshape(25, 17), lons32,
                                                         lats32, wlat, wlon) for x in phys)
                    sums[0, h, v] += six(f, t)
                    if s == si:
                        sums[1, h, v], sums[2, h, v] = six(f, wrf.astype(np.float64)), six(wrf.astype(np.float64), t)
                        mets[0, h, v] = era5.compute_metrics(f, t)
                        mets[1, h, v] = era5.compute_metrics(f, wrf)
                        mets[2, h, v] = era5.compute_metrics(wrf, t)
                        assert sums[1, h, v, 0, 0] >= 60
        out["grid_sums"], out["grid_mags"], out["grid_metrics"] = sums[..., 0, :], sums[..., 1, :], mets

    path = os.path.join(HERE, "wrf_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e3:.1f} kB, {len(out)} arrays) and {WC.WRF_JSON} "
          f"({os.path.getsize(WC.WRF_JSON) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
