"""Generate the multires-input and full-pipeline fixtures by RUNNING the reference's own
`scripts/build_multires_dataset.py`, `scripts/evaluate_full_pipeline.py`, `src/data/dataloader_chunked.py`,
`src/postprocessing/mos_correction.py` and `src/assimilation/optimal_interpolation.py` on the CPU.

Run from the repo root, only where the reference checkout (`make_golden.REF`), scipy and sklearn exist (never on the
GPU box):

    python tests/golden/make_multires_golden.py

The inputs are a synthetic pair of datasets (tests/helpers/multires_case.py): global 24 x 12, regional 9 x 7 that
reaches past the box (15, 46, 60, 120), 5 features, 12 frames.  Outputs (data only - arrays and strings of results,
no reference source text):

tests/golden/multires_vectors.npz
  g_data, r_data, mean, std        the two fp16 series and the float32 scalers
  nm_* / mc_*                      build_node_mapping / build_multires_coords outputs
  interp_data, merge_data          data.npy as build_interpolate_mode / build_merge_mode wrote it
  interp_info, merge_info          their dataset_info.json (a JSON string; the source_* paths blanked)
  interp_X<i>, interp_y<i>, merge_X<i>, merge_y<i>   the reference TimeseriesChunkDataset windows (obs 2, pred 2, "all")
  frame_interp_<t>, frame_merge_<t>  build_multires_frame without / with regional_data, normalised as at :463
  fine_f64                         float64 RegularGridInterpolator((lats, lons)) output of frame 3, channel 0 at the
                                   41 x 61 targets of multires_case.fine_axes()

tests/golden/pipeline_vectors.npz
  lapse2_in, lapse3_in             [n, 2] / [m, 3, 2] inputs in the order ("z_surf", "t2m")
  lapse2_f32, lapse2_f64, ...      the t2m column of apply_lapse for the elevation 250 as a Python float and as an
                                   np.float64; lapse3_mean for elev_f64, the np.float64 mean station elevation
  stn_rows_sim, stn_rows_score     the float64 search of simulate_station_obs, the float32 search of :406-410
  sim_truth, sim_obs               simulate_station_obs input and output (the reference's function sizes its field by
                                   len(r_lats) and raises IndexError here; restated with the field sized by the grid),
  sim_head_obs                     the reference's own output for multires_case.FIRST_ROW_STATIONS, where it does run:
                                   the first len(r_lats) rows of the field
  starts_<k>_args, starts_<k>      (T_overlap, obs, ar, max_samples) and the sample starts of :371-387
  forest_*                         a small HistGradientBoostingRegressor fitted here, flattened (make_mos_golden.flatten)
  ev_<s>_<h>_<variant>             every variant's [G, C] prediction of sample s, step h, in the order of
                                   multires_case.VARIANTS ("truth" too); ev_<s>_<h>_oi64 the OI analysis in float64
  ev_<s>_<h>_sum32                 [V, C] the float32 `diff.sum(axis=0)` the script adds,
  ev_<s>_<h>_sum64 / _stn64        the same sums (grid / scoring stations) in float64 from the float32 squares
The evaluation loop is assembled here from the reference's helpers (build_multires_frame, denormalize, apply_lapse,
apply_learned_mos_t2m, simulate_station_obs, OptimalInterpolation) in the order of
scripts/evaluate_full_pipeline.py:449-666, driving tests/helpers/diff_stub.py with use_residual.
"""
import argparse
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402  (where the reference checkout lives, placeholder modules)
import make_assim_golden  # noqa: E402  (_oi_pair: the reference's OI in float32 and float64)
import make_mos_golden  # noqa: E402  (flatten, Recorder, check_wind_margin)
import multires_case as MC  # noqa: E402
from diff_stub import DiffStub  # noqa: E402

REF = make_golden.REF


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_series(rng, n_lon, n_lat, lats, lons):
    """fp16 (T, lon, lat, 5) of realistic size: t2m [K], winds [m/s], surface height [m], precipitation [m]."""
    la = np.radians(lats)[None, None, :]
    lo = np.radians(lons)[None, :, None]
    t = np.arange(MC.T)[:, None, None]
    noise = lambda s: s * rng.standard_normal((MC.T, n_lon, n_lat))  # noqa: E731
    x = np.empty((MC.T, n_lon, n_lat, 5))
    x[..., 0] = 288.0 - 35.0 * np.sin(la) ** 2 + 4.0 * np.sin(lo + 0.5 * t) + noise(1.5)
    x[..., 1] = 8.0 * np.cos(2 * la) * np.cos(lo + 0.3 * t) + noise(1.0)
    x[..., 2] = 6.0 * np.sin(la + lo) + noise(1.0)
    x[..., 3] = np.abs(900.0 + 1400.0 * np.sin(2 * lo) * np.cos(la) + 0 * t) + 200.0 * np.cos(3 * la)
    x[..., 4] = 1e-3 * np.abs(noise(1.0))
    assert np.abs(x).max() < 6e4
    return x.astype(np.float16)


def multires_part(B, E, dirs):
    from src.data.dataloader_chunked import TimeseriesChunkDataset

    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    rng = np.random.default_rng(20260)
    g_data = synthetic_series(rng, len(g_lons), len(g_lats), g_lats, g_lons)
    r_data = synthetic_series(rng, len(r_lons), len(r_lats), r_lats, r_lons)
    mean = np.array([275.0, 0.5, -0.25, 800.0, 8e-4], dtype=np.float32)
    std = np.array([14.0, 6.0, 5.0, 650.0, 7e-4], dtype=np.float32)
    gdir = MC.write_dataset(os.path.join(dirs, "global"), g_data, g_lats, g_lons, mean, std, MC.VARS)
    rdir = MC.write_dataset(os.path.join(dirs, "region"), r_data, r_lats, r_lons, mean, std, MC.VARS)
    out = dict(g_data=g_data, r_data=r_data, mean=mean, std=std)

    with contextlib.redirect_stdout(io.StringIO()):
        nm = B.build_node_mapping(g_lats, g_lons, r_lats, r_lons, MC.ROI)
    for k, v in zip(("flat_lats", "flat_lons", "global_mask", "region_mask", "keep_global"), nm):
        out[f"nm_{k}"] = v
    mc = E.build_multires_coords(g_lats, g_lons, r_lats, r_lons, MC.ROI)
    for k, v in zip(("flat_lats", "flat_lons", "region_mask", "keep_global"), mc[:4]):
        out[f"mc_{k}"] = v
    out["mc_n_global_kept"] = np.int64(mc[4])
    assert len(nm[0]) == 341 and int(mc[4]) == 278

    runs = {
        "interp": (B.build_interpolate_mode, dict(region_coords=os.path.join(rdir, "coords.npz"))),
        "merge": (B.build_merge_mode, dict(region_dir=rdir, time_offset_global=None, time_offset_region=None)),
    }
    for tag, (fn, extra) in runs.items():
        odir = os.path.join(dirs, tag)
        with contextlib.redirect_stdout(io.StringIO()):
            fn(argparse.Namespace(global_dir=gdir, roi=list(MC.ROI), out_dir=odir, **extra))
            ds = TimeseriesChunkDataset(odir, obs_window=MC.OBS, pred_steps=MC.PRED, split="all")
        out[f"{tag}_data"] = np.fromfile(os.path.join(odir, "data.npy"), dtype=np.float16).reshape(MC.T, 341, 5)
        with open(os.path.join(odir, "dataset_info.json")) as fh:
            info = json.load(fh)
        out[f"{tag}_info"] = np.array(json.dumps({k: ("" if k.startswith("source_") else v) for k, v in info.items()}))
        for i in MC.WINDOW_INDICES:
            X, y = ds[i]
            out[f"{tag}_X{i}"], out[f"{tag}_y{i}"] = X.numpy(), y.numpy()

    keep_global, n_kept = mc[3], mc[4]
    for t in MC.FRAME_TIMES:
        for tag, reg in (("interp", None), ("merge", r_data)):
            frame = E.build_multires_frame(g_data, g_lats, g_lons, r_lats, r_lons, keep_global, n_kept, 63, 5,
                                           t_global=t, t_regional=t, regional_data=reg)
            assert frame.dtype == np.float32 and frame.shape == (341, 5)
            out[f"frame_{tag}_{t}"] = (frame - mean) / std
    assert np.array_equal(E.build_multires_frame(g_data, g_lats, g_lons, r_lats, r_lons, keep_global, n_kept, 63, 5,
                                                 3, 3, r_data).astype(np.float16), out["merge_data"][3])

    # the float64 interpolator output that pins the corner order
    from scipy.interpolate import RegularGridInterpolator

    f_lats, f_lons = MC.fine_axes()
    field = g_data[3, :, :, 0].astype(np.float32).T  # (lat, lon)
    lo_m, la_m = np.meshgrid(f_lons, f_lats)
    pts = np.stack([la_m.ravel(), lo_m.ravel()], axis=-1)
    fine = RegularGridInterpolator((g_lats, g_lons), field, method="linear", bounds_error=False, fill_value=None)(pts)
    assert fine.dtype == np.float64 and fine.shape == (2501,)
    from graphcast_lite_amd.verify import regrid_tables

    cell, w = regrid_tables(g_lats, g_lons, f_lats, f_lons)  # (lons, lats) order, targets longitude-major
    v = field.T.astype(np.float64)
    jl, il = cell[:, 0], cell[:, 1]
    other = ((v[jl, il] * w[:, 0] + v[jl, il + 1] * w[:, 1]) + v[jl + 1, il] * w[:, 2]) + v[jl + 1, il + 1] * w[:, 3]
    other = other.reshape(len(f_lons), len(f_lats)).T.ravel()
    assert np.any(other != fine), "the (lons, lats) corner order gives the same float64 values: the fixture pins nothing"
    out["fine_f64"] = fine
    return out, (g_data, r_data, mean, std, g_lats, g_lons, r_lats, r_lons, keep_global, n_kept, mc[2])


def lapse_part(E, out):
    rng = np.random.default_rng(20261)
    elev64 = MC.mean_station_elev()
    assert type(elev64) is np.float64
    out["elev_f64"] = elev64
    order = ["z_surf", "t2m"]
    x2 = np.stack([rng.normal(600, 400, 20000), rng.normal(260, 12, 20000)], axis=1).astype(np.float32)
    x3 = np.stack([rng.normal(600, 400, (3000, 3)), rng.normal(260, 12, (3000, 3))], axis=2).astype(np.float32)
    out["lapse2_in"], out["lapse3_in"] = x2, x3
    for tag, x in (("lapse2", x2), ("lapse3", x3)):
        a = E.apply_lapse(x, order, MC.LAPSE_ELEV_FLOAT)
        b = E.apply_lapse(x, order, np.float64(MC.LAPSE_ELEV_FLOAT))
        c = E.apply_lapse(x, order, elev64)
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a[..., 0], x[..., 0])
        assert np.count_nonzero(a[..., 1] != b[..., 1]) >= (50 if tag == "lapse2" else 10), "scalar types agree"
        out[f"{tag}_f32"], out[f"{tag}_f64"] = a[..., 1], b[..., 1]
        if tag == "lapse3":
            out[f"{tag}_mean"] = c[..., 1]
    assert E.apply_lapse(x2, ["t2m", "u"], 1.0) is x2


def sample_starts(T_overlap, obs, ar, max_samples):
    """scripts/evaluate_full_pipeline.py:371-387, inline in its main(): restated."""
    n_test_total = int(T_overlap * 0.2)
    n_val = n_test_total // 2
    test_start = T_overlap - n_test_total + n_val
    valid = list(range(test_start, T_overlap - (obs + ar) + 1))
    n = min(max_samples, len(valid))
    if n < len(valid):
        step = len(valid) // n
        return [valid[i * step] for i in range(n)]
    return valid[:n]


def tiny_mos(rng):
    from sklearn.ensemble import HistGradientBoostingRegressor

    n = 600
    X = np.column_stack([
        rng.normal(10, 15, n), rng.normal(-5, 10, n), rng.gamma(2, 2, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.normal(990, 15, n), rng.uniform(0, 100, n), rng.uniform(0, 600, n), rng.exponential(0.3, n),
        rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.uniform(-60, 60, n), rng.gamma(2, 2, n), rng.normal(10, 15, n), rng.normal(0, 3, n),
        rng.uniform(14, 47, n), rng.uniform(58, 122, n), rng.uniform(90, 480, n)])
    X[:, [1, 5, 6, 7, 14]] = np.where(rng.random((n, 5)) < 0.6, np.nan, X[:, [1, 5, 6, 7, 14]])
    y = 0.08 * X[:, 0] - 0.2 * X[:, 2] + 1.5 * X[:, 9] + 0.01 * X[:, 13] + 0.05 * X[:, 15] + rng.normal(0, 0.3, n)
    return HistGradientBoostingRegressor(max_iter=12, max_depth=3, random_state=0).fit(X, y)


def simulate_station_obs(E, truth, r_lats, r_lons, stations, var_order):
    """scripts/evaluate_full_pipeline.py:203-222 with the field sized by the grid.  The reference sizes it by
    `len(r_lats)` (the latitude AXIS it is called with at :617), so it raises IndexError for any station whose nearest
    node is not among the first len(r_lats) nodes - asserted here - and the search and the row copy are restated."""
    try:
        E.simulate_station_obs(truth, r_lats, r_lons, stations, var_order)
        raise AssertionError("the reference's simulate_station_obs ran: call it instead of this restatement")
    except IndexError:
        pass
    lo_m, la_m = np.meshgrid(r_lons, r_lats)
    flat_lats, flat_lons = la_m.ravel(), lo_m.ravel()
    obs = np.full((flat_lats.size, len(var_order)), np.nan, dtype=np.float32)
    for st in stations:
        gidx = int(np.argmin((flat_lats - st["lat"]) ** 2 + (flat_lons - st["lon"]) ** 2))
        obs[gidx, :] = truth[gidx, :]
    return obs


def evaluation_part(E, geo, out):
    from src.assimilation.optimal_interpolation import OptimalInterpolation

    g_data, r_data, mean, std, g_lats, g_lons, r_lats, r_lons, keep_global, n_kept, region_mask = geo
    C, G, N = 5, 63, 341
    model = tiny_mos(np.random.default_rng(20262))
    forest = make_mos_golden.flatten(model)
    out.update(forest)
    rec = make_mos_golden.Recorder(model)
    bundle = {"model": rec}
    stub = DiffStub(MC.OBS, C)
    elev = MC.mean_station_elev()

    lo_m, la_m = np.meshgrid(r_lons, r_lats)
    r_flat_lats, r_flat_lons = la_m.ravel().astype(np.float32), lo_m.ravel().astype(np.float32)
    score_rows = [int(np.argmin((r_flat_lats - st["lat"]) ** 2 + (r_flat_lons - st["lon"]) ** 2)) for st in MC.STATIONS]
    sim_rows = [int(np.argmin((la_m.ravel() - st["lat"]) ** 2 + (lo_m.ravel() - st["lon"]) ** 2)) for st in MC.STATIONS]
    assert len(set(sim_rows)) == 3 and sim_rows[0] == sim_rows[1]
    out["stn_rows_score"], out["stn_rows_sim"] = np.array(score_rows, np.int64), np.array(sim_rows, np.int64)
    truth0 = r_data[5].astype(np.float32).transpose(1, 0, 2).reshape(-1, C)
    out["sim_truth"] = truth0
    out["sim_obs"] = simulate_station_obs(E, truth0, r_lats, r_lons, MC.STATIONS, MC.VARS)
    assert np.array_equal(np.nonzero(~np.isnan(out["sim_obs"][:, 0]))[0], np.unique(sim_rows))
    # where the reference's own function does run (every station nearest to one of the first len(r_lats) nodes) its
    # output is the head of the field
    head = E.simulate_station_obs(truth0, r_lats, r_lons, MC.FIRST_ROW_STATIONS, MC.VARS)
    assert head.shape == (len(r_lats), C) and (~np.isnan(head[:, 0])).sum() == 2
    out["sim_head_obs"] = head

    oi_args = (r_lats, r_lons, MC.OI_SIGMA_B, MC.OI_SIGMA_O, MC.OI_L, "cpu")
    mos_kw = dict(stations=MC.STATIONS)
    idw_kw = dict(spatial_idw=True, idw_power=MC.IDW_POWER, idw_max_radius_km=MC.IDW_RADIUS_KM)
    for si, t_start in enumerate(MC.SAMPLE_STARTS):
        frames = []
        for t_off in range(MC.OBS):
            f = E.build_multires_frame(g_data, g_lats, g_lons, r_lats, r_lons, keep_global, n_kept, G, C,
                                       t_global=t_start + t_off, t_regional=t_start + t_off, regional_data=r_data)
            frames.append((f - mean) / std)
        curr = torch.from_numpy(np.stack(frames, axis=1)).unsqueeze(0).float()
        persist = np.array(r_data[t_start + MC.OBS - 1], dtype=np.float32).transpose(1, 0, 2).reshape(-1, C)
        for h in range(MC.AR):
            gt = np.array(r_data[t_start + MC.OBS + h], dtype=np.float32).transpose(1, 0, 2).reshape(-1, C)
            with torch.no_grad():
                pred = stub(X=curr.view(1, N, MC.OBS * C), attention_threshold=0.0)
            gnn_out = curr[:, :, -1, :] + pred
            roi_norm = gnn_out[0].numpy()[region_mask]
            roi_phys = E.denormalize(roi_norm, mean, std)
            assert roi_phys.dtype == np.float32 and np.array_equal(roi_phys, roi_norm * std + mean)
            out[f"ev_{si}_{h}_norm"] = roi_norm
            gnn_3d = roi_phys[:, np.newaxis, :]
            vt = [MC.valid_time(h)]

            def mos(x3, **kw):
                return E.apply_learned_mos_t2m(x3, MC.VARS, bundle, r_flat_lats, r_flat_lons, vt, **mos_kw, **kw)[0]

            preds = {
                "GNN": gnn_3d[:, 0, :],
                "GNN+lapse": E.apply_lapse(gnn_3d.copy(), MC.VARS, elev)[:, 0, :],
                "GNN+MOS": mos(gnn_3d.copy())[:, 0, :],
                "GNN+lapse+MOS": mos(E.apply_lapse(gnn_3d.copy(), MC.VARS, elev))[:, 0, :],
                "GNN+lapse+MOS+IDW": mos(E.apply_lapse(gnn_3d.copy(), MC.VARS, elev), **idw_kw)[:, 0, :],
            }
            assert np.any(preds["GNN+lapse+MOS+IDW"] != preds["GNN+lapse+MOS"]), "IDW reaches no other point"
            obs = simulate_station_obs(E, gt, r_lats, r_lons, MC.STATIONS, MC.VARS)
            base = torch.from_numpy(preds["GNN+lapse+MOS+IDW"].copy()).float()
            x32, x64 = make_assim_golden._oi_pair(OptimalInterpolation, oi_args, {}, base, torch.from_numpy(obs).float())
            preds["GNN+lapse+MOS+IDW+OI"] = x32
            changed = np.any(x32 != base.numpy(), axis=1)
            assert changed.sum() > len(set(sim_rows)), "OI reaches no other point"
            preds["Persistence"] = persist
            out[f"ev_{si}_{h}_oi64"] = x64
            out[f"ev_{si}_{h}_truth"] = gt
            s32, s64, t64 = [], [], []
            for name in MC.VARIANTS:
                p = np.ascontiguousarray(preds[name], dtype=np.float32)
                out[f"ev_{si}_{h}_{name}"] = p
                diff = (p - gt) ** 2
                assert diff.dtype == np.float32
                s32.append(diff.sum(axis=0))
                s64.append(diff.astype(np.float64).sum(axis=0))
                t64.append(sum(diff[i].astype(np.float64) for i in score_rows))
            out[f"ev_{si}_{h}_sum32"], out[f"ev_{si}_{h}_sum64"] = np.array(s32), np.array(s64)
            out[f"ev_{si}_{h}_stn64"] = np.array(t64)
            curr = torch.cat([curr[:, :, 1:, :], gnn_out.unsqueeze(2)], dim=2)
    make_mos_golden.check_wind_margin(np.array(rec.X), forest)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    warnings.filterwarnings("ignore")
    make_golden._placeholders()
    sys.path.insert(0, REF)
    B = _load("_ref_build_multires", "scripts", "build_multires_dataset.py")
    E = _load("_ref_eval_pipeline", "scripts", "evaluate_full_pipeline.py")
    with tempfile.TemporaryDirectory() as d:
        mr, geo = multires_part(B, E, d)
    path = os.path.join(HERE, "multires_vectors.npz")
    np.savez_compressed(path, **mr)
    print(f"wrote {path}: {len(mr)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")

    out = {}
    lapse_part(E, out)
    for k, args in enumerate([(1460, 2, 4, 50), (200, 2, 4, 500), (97, 2, 2, 3)]):
        out[f"starts_{k}_args"] = np.array(args, dtype=np.int64)
        out[f"starts_{k}"] = np.array(sample_starts(*args), dtype=np.int64)
    assert len(out["starts_1"]) < 500
    evaluation_part(E, geo, out)
    path = os.path.join(HERE, "pipeline_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
