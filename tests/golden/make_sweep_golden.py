"""Generate the MOS/IDW sweep fixtures by RUNNING the reference's own `apply_learned_mos_t2m`
(`src/postprocessing/mos_correction.py`) once per IDW setting, as `scripts/mos_idw_sweep.py:260-272` does.

Run from the repo root, only where the reference checkout (`make_golden.REF`) and sklearn exist (never on the GPU box):

    python tests/golden/make_sweep_golden.py

Output (data only - arrays, no reference source text): tests/golden/sweep_vectors.npz
  powers, radii      the settings of the kernel tests: the scripts' ten (v2's order), then power 1.0 / 300 km and
                     power 2.0 / 1 km
  box1_out, box1_n   the corrected t2m [12, G] and n_corrected [12] of every setting, one step, the 19 stations on the
                     61 x 41 box of tests/test_mos.py (float32 forecast `forecast(81, ...)`)
  box4_out, box4_n   the same for four steps [3, G, 4] and the settings box4_cfg (indices into powers / radii)
  box_reach          [10, 3]: non-station rows with no / exactly one / several points inside the radius of each of the
                     ten settings (condition (a) below)

Evaluator cases (`pipeline.MosIdwSweep`), on the 7 x 9 regional grid, the two samples and the stand-in model of
tests/golden/make_multires_golden.py, whose fixture (pipeline_vectors.npz / multires_vectors.npz) supplies the raw and
lapse-corrected forecasts, the truth, persistence and the small forest; the stations and radii are EV_STATIONS /
EV_CONFIGS of tests/helpers/sweep_case.py (the grid's cells are ~600 x 800 km):
  mr_<s>_<h>_fields  [4 + 10, 63] the t2m of every row of the script's table (Persistence, GNN_raw, GNN+lapse,
                     GNN+lapse+MOS_station, then the ten settings) for sample s, horizon h, as
                     scripts/mos_idw_sweep.py:196-282 forms them; mr_<s>_<h>_truth [63]
  mr_rmse, mr_rmse64 [14, AR] the script's RMSE (float32 `np.sum` added to a Python float, :242-276, :306-308) and the
                     same from float64 sums; mr_best [AR] the index of the best setting (:345-357)
  mg_<s>_fields, mg_<s>_truth, mg_rmse, mg_rmse64, mg_best   the same for scripts/mos_idw_sweep_v2.py:229-304 on the
                     sample's first step: truth and persistence de-normalised from the z-scored frames, the lapse by
                     v2's own apply_lapse_correction with a Python-float elevation

The generator asserts on the reference alone:
  (a) every one of the ten settings has rows with no point in range, rows with exactly one and rows with several;
  (b) in both evaluator cases the best and the second-best setting differ by at least 1e-4 relative in RMSE at every
      horizon;
  (c) in the evaluator cases at least three settings have two or more points in range for at least a quarter of the
      non-station rows;
  and that the script's float32-summed RMSE and its float64 recomputation agree to 1e-5 relative.
"""
import os
import sys
import warnings
from datetime import datetime

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402  (placeholder modules for the reference's imports)
import make_mos_golden as mg  # noqa: E402  (the reference loader, the stations, the grids and the forecasts)
import make_multires_golden as mm  # noqa: E402  (tiny_mos, _load)
import multires_case as MC  # noqa: E402
import sweep_case as SC  # noqa: E402

CONFIGS = [  # scripts/mos_idw_sweep_v2.py:192-203, then the two extra settings of the kernel tests
    (2.0, 300.0), (2.0, 200.0), (2.0, 150.0), (2.0, 100.0), (2.0, 50.0), (3.0, 300.0), (3.0, 150.0), (3.0, 100.0),
    (1.5, 300.0), (1.5, 150.0), (1.0, 300.0), (2.0, 1.0)]
BOX4 = [0, 7, 9]
START = datetime(2024, 7, 1, 6)


def reach_counts(ref, lat, lon, stations, radii):
    """Per radius: how many non-station rows have 0 / 1 / >= 2 station points inside it (the reference's own
    haversine and nearest-node search)."""
    pts = []
    for st in stations:
        gi = int(np.argmin((lat - st["lat"]) ** 2 + (lon - st["lon"]) ** 2))
        if gi not in pts:
            pts.append(gi)
    d = np.array([[ref._haversine_km(float(lat[g]), float(lon[g]), float(lat[k]), float(lon[k])) for k in pts]
                  for g in range(lat.size)])
    rows = np.setdiff1d(np.arange(lat.size), pts)
    out = []
    for r in radii:
        n = (d[rows] < r).sum(axis=1)
        out.append([int((n == 0).sum()), int((n == 1).sum()), int((n >= 2).sum())])
    return np.array(out, dtype=np.int64), len(pts), float(d[rows].min())


def tables(se, count, labels):
    """RMSE per table row and horizon, and the best setting per horizon, as the scripts compute them."""
    rmse = np.array([[np.sqrt(se[n][h] / max(count[h], 1)) for h in range(len(count))] for n in se])
    names = list(se)
    best = []
    for h in range(len(count)):
        best_cfg, best_rmse = None, 9999.0
        for i, label in enumerate(labels):
            r = rmse[names.index(f"GNN+lapse+MOS+IDW_{label}")][h]
            if r < best_rmse:
                best_rmse, best_cfg = r, i
        best.append(best_cfg)
        idw = np.sort(rmse[4:, h])
        assert (idw[1] - idw[0]) / idw[0] >= 1e-4, "condition (b): the two best settings are too close"
    return rmse, np.array(best, dtype=np.int64)


def evaluator_part(ref, out):
    pv = np.load(os.path.join(HERE, "pipeline_vectors.npz"))
    gv = np.load(os.path.join(HERE, "multires_vectors.npz"))
    make_golden._placeholders()
    sys.path.insert(0, mg.REF)
    V2 = mm._load("_ref_sweep_v2", "scripts", "mos_idw_sweep_v2.py")
    E = mm._load("_ref_eval_pipeline", "scripts", "evaluate_full_pipeline.py")
    model = mm.tiny_mos(np.random.default_rng(20262))
    for k, v in mg.flatten(model).items():
        assert np.array_equal(v, pv[k]), f"the refitted forest differs from pipeline_vectors.npz ({k})"
    rec = mg.Recorder(model)
    bundle = {"model": rec}
    mean, std = gv["mean"], gv["std"]
    r_lats, r_lons = MC.regional_axes()
    lo_m, la_m = np.meshgrid(r_lons, r_lats)
    lat32, lon32 = la_m.ravel().astype(np.float32), lo_m.ravel().astype(np.float32)
    t2m, z = MC.VARS.index("t2m"), MC.VARS.index("z_surf")
    labels = [c[2] for c in SC.EV_CONFIGS]
    names = ["Persistence", "GNN_raw", "GNN+lapse", "GNN+lapse+MOS_station"] + [f"GNN+lapse+MOS+IDW_{lb}" for lb in labels]

    reach, npts, _ = reach_counts(ref, lat32, lon32, SC.EV_STATIONS, [c[1] for c in SC.EV_CONFIGS])
    rows = 63 - npts
    print(f"evaluator: {len(SC.EV_STATIONS)} stations on {npts} points; rows with several points in range per setting:",
          reach[:, 2].tolist())
    assert (reach[:, 2] >= rows / 4).sum() >= 3, "condition (c)"
    out["ev_reach"] = reach

    def variants(lapse_3d, vt):
        res = [ref.apply_learned_mos_t2m(lapse_3d.copy(), MC.VARS, bundle, lat32, lon32, vt, stations=SC.EV_STATIONS,
                                         spatial_idw=False)[0][:, 0, t2m]]
        for pw, rad, _ in SC.EV_CONFIGS:
            res.append(ref.apply_learned_mos_t2m(lapse_3d.copy(), MC.VARS, bundle, lat32, lon32, vt,
                                                 stations=SC.EV_STATIONS, spatial_idw=True, idw_power=pw,
                                                 idw_max_radius_km=rad)[0][:, 0, t2m])
        assert any(np.any(r != res[0]) for r in res[1:])
        return res

    def add(se, se64, fields, gt, h):
        for n, f in zip(names, fields):
            d = (f - gt) ** 2
            assert d.dtype == np.float32
            se[n][h] += np.sum(d)
            se64[n][h] += float(d.astype(np.float64).sum())

    def finish(tag, se, se64, count):
        rmse, best = tables(se, count, labels)
        rmse64, best64 = tables(se64, count, labels)
        assert np.array_equal(best, best64)
        assert np.all(np.abs(rmse - rmse64) <= 1e-5 * rmse64), "the float32 sums leave the 1e-5 bound"
        out[f"{tag}_rmse"], out[f"{tag}_rmse64"], out[f"{tag}_best"] = rmse, rmse64, best
        print(f"{tag}: best per horizon {[labels[b] for b in best]}, float32-sum error "
              f"{np.max(np.abs(rmse - rmse64) / rmse64):.2e}")

    # scripts/mos_idw_sweep.py:196-282 (the lapse elevation is argparse's untouched default, an np.float64)
    elev = SC.lapse_elev()
    S = len(MC.SAMPLE_STARTS)
    se, se64 = ({n: [0.0] * MC.AR for n in names} for _ in range(2))
    for s in range(S):
        for h in range(MC.AR):
            raw, gt, persist = pv[f"ev_{s}_{h}_GNN"], pv[f"ev_{s}_{h}_truth"], pv[f"ev_{s}_{h}_Persistence"]
            lapse_3d = E.apply_lapse(raw[:, np.newaxis, :].copy(), MC.VARS, elev)
            fields = [persist[:, t2m], raw[:, t2m], lapse_3d[:, 0, t2m]] + variants(lapse_3d, [MC.valid_time(h)])
            out[f"mr_{s}_{h}_fields"], out[f"mr_{s}_{h}_truth"] = np.stack(fields), gt[:, t2m]
            add(se, se64, fields, gt[:, t2m], h)
    finish("mr", se, se64, [S * 63] * MC.AR)

    # scripts/mos_idw_sweep_v2.py:229-304 on the same windows: X = the two z-scored frames, Y = the next one
    se, se64 = ({n: [0.0] for n in names} for _ in range(2))
    for s in range(S):
        raw = pv[f"ev_{s}_0_GNN"]
        gt_norm = (pv[f"ev_{s}_0_truth"] - mean) / std
        persist_norm = (pv[f"ev_{s}_0_Persistence"] - mean) / std
        assert gt_norm.dtype == np.float32
        gt = gt_norm[:, t2m] * std[t2m] + mean[t2m]
        persist = persist_norm[:, t2m] * std[t2m] + mean[t2m]
        lapse_3d = V2.apply_lapse_correction(raw[:, np.newaxis, :], MC.VARS, float(elev), raw[:, z])
        assert lapse_3d.dtype == np.float32
        fields = [persist, raw[:, t2m], lapse_3d[:, 0, t2m]] + variants(lapse_3d, [MC.valid_time(0)])
        out[f"mg_{s}_fields"], out[f"mg_{s}_truth"] = np.stack(fields), gt
        add(se, se64, fields, gt, 0)
    finish("mg", se, se64, [S * 63])
    mg.check_wind_margin(np.array(rec.X), mg.flatten(model))


def main():
    warnings.filterwarnings("ignore")
    ref = mg._ref_mos()
    bundle = ref.load_learned_mos(os.path.join(mg.REF, "live_runtime_bundle", "learned_mos_t2m.joblib"))
    lat, lon = mg.box_grid()
    sts = mg.stations()
    out = {"powers": np.array([c[0] for c in CONFIGS]), "radii": np.array([c[1] for c in CONFIGS]),
           "box4_cfg": np.array(BOX4, dtype=np.int64)}

    reach, npts, dmin = reach_counts(ref, lat, lon, sts, [c[1] for c in CONFIGS[:10]])
    print(f"{len(sts)} stations on {npts} points, nearest non-station row at {dmin:.1f} km")
    for (pw, rad), (n0, n1, n2) in zip(CONFIGS, reach):
        print(f"  power {pw} radius {rad:5.0f} km: {n0} rows out of range, {n1} with one point, {n2} with several")
        assert n0 > 0 and n1 > 0 and n2 > 0, "condition (a): a setting misses a case"
    out["box_reach"] = reach

    def run(pred, steps, cfgs):
        res, ns = [], []
        for pw, rad in cfgs:
            cor, n = ref.apply_learned_mos_t2m(pred.copy(), mg.VARS, bundle, lat, lon, mg.valid_times(START, steps),
                                               stations=sts, spatial_idw=True, idw_power=pw, idw_max_radius_km=rad)
            res.append(cor[:, :, 0])
            ns.append(n)
        return np.stack(res), np.array(ns, dtype=np.int64)

    o1, out["box1_n"] = run(mg.forecast(81, lat.size, 1, mg.VARS), 1, CONFIGS)
    out["box1_out"] = o1[:, :, 0]
    out["box4_out"], out["box4_n"] = run(mg.forecast(82, lat.size, 4, mg.VARS), 4, [CONFIGS[i] for i in BOX4])

    evaluator_part(ref, out)

    path = os.path.join(HERE, "sweep_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
