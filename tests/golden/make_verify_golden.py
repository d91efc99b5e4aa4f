"""Generate the forecast-scoring and regional-blending fixtures by RUNNING the reference's own inference-script helpers
(`scripts/predict.py`, `scripts/predict_pipeline.py`, `scripts/interpolate_to_region.py`; torch, numpy, scipy).

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_verify_golden.py

Output (data only - arrays, no reference source text): tests/golden/verify_vectors.npz
  sm_<case>_*     StreamingMetrics after several updates: the inputs (t<k>, p<k> per update), the reference's value of
                  every property and attribute (ref_*) and a float64 restatement of the same sums written here (x64_*),
                  the arbiter between two float32 results.  Cases: `excl` (C 5, P 3, exclude [1, 4], a column 1e4
                  standard deviations from 0, a constant column), `pipe` (the same data through the predict_pipeline
                  variant, no exclusion), `onestep` (P 1), `region` (19 channels, 2 steps, the rows of the 50-60N x 83-98E
                  box of the 512 x 256 grid only: region_idx numbers them as region_node_indices does)
  rg_<case>_*     interpolate_global_to_region from the 64 x 32 grid: `box` (a 0.25 deg 61 x 41 box), `desc` (the same
                  box with descending latitudes), `east` (355-359.75E, past the last global longitude), `edge` (targets
                  on the poles and on grid nodes); the targets' scipy cell indices / normalised distances (find_indices)
  f2d_*           interpolate_field_2d of a float64 field onto the `box` targets
  taper_<n_lat>_<n_lon>_<w>   build_taper_mask_2d, and blend_* the taper blend of the pipeline (`box`, width 3)
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (where the reference checkout lives; inert placeholders for absent modules)

REF = make_golden.REF
BOX = (50.0, 60.0, 83.0, 98.0)


def _script(name):
    spec = importlib.util.spec_from_file_location(f"_ref_{name}", os.path.join(REF, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PROPS = ("n", "total_elem", "sum_se", "sum_ae", "sum_se_per_ch", "elem_per_ch", "sum_acc", "acc_count", "mse", "rmse",
         "mae", "acc", "acc_per_channel", "rmse_per_channel")
PIPE_PROPS = ("n", "total_elem", "sum_se", "sum_ae", "sum_se_per_ch", "elem_per_ch", "sum_acc", "acc_count", "rmse",
              "acc", "acc_per_channel", "rmse_per_channel")


def _restated(C, exclude, pairs):
    """The metric sums in float64 from the float32 inputs: se / ae from float64 differences, the correlation centred
    in float64 with the 1e-8 added to the product of the norms."""
    excl = set(exclude or [])
    s = dict(n=0, total_elem=0, sum_se=0.0, sum_ae=0.0, sum_se_per_ch=np.zeros(C), elem_per_ch=np.zeros(C, np.int64),
             sum_acc=np.zeros(C), acc_count=np.zeros(C, np.int64))
    for t, p in pairs:
        t, p = t.astype(np.float64), p.astype(np.float64)
        d = p - t
        keep = [k for k in range(t.shape[1]) if k % C not in excl]
        for k in range(t.shape[1]):
            ta, pa = t[:, k] - t[:, k].mean(), p[:, k] - p[:, k].mean()
            s["sum_se_per_ch"][k % C] += float(np.sum(d[:, k] ** 2))
            s["elem_per_ch"][k % C] += t.shape[0]
            s["sum_acc"][k % C] += float(np.sum(ta * pa) / (np.sqrt(np.sum(ta * ta)) * np.sqrt(np.sum(pa * pa)) + 1e-8))
            s["acc_count"][k % C] += 1
        if keep:
            s["sum_se"] += float(np.sum(d[:, keep] ** 2))
            s["sum_ae"] += float(np.sum(np.abs(d[:, keep])))
            s["total_elem"] += t.shape[0] * len(keep)
        s["n"] += 1
    te = max(s["total_elem"], 1)
    s["mse"] = s["sum_se"] / te
    s["rmse"] = float(np.sqrt(s["mse"]))
    s["mae"] = s["sum_ae"] / te
    s["acc_per_channel"] = s["sum_acc"] / np.maximum(s["acc_count"], 1)
    s["rmse_per_channel"] = np.sqrt(s["sum_se_per_ch"] / np.maximum(s["elem_per_ch"], 1))
    dyn = [c for c in range(C) if c not in excl]
    s["acc"] = float(s["acc_per_channel"][dyn].mean()) if dyn else 0.0
    return s


def _sm_case(out, tag, sm, props, C, exclude, pairs):
    for k, (t, p) in enumerate(pairs):
        sm.update(torch.from_numpy(t), torch.from_numpy(p))
        out[f"sm_{tag}_t{k}"], out[f"sm_{tag}_p{k}"] = t, p
    x64 = _restated(C, exclude, pairs)
    for name in props:
        out[f"sm_{tag}_ref_{name}"] = np.asarray(getattr(sm, name))
        out[f"sm_{tag}_x64_{name}"] = np.asarray(x64[name])
    out[f"sm_{tag}_C"] = np.int64(C)
    out[f"sm_{tag}_nupd"] = np.int64(len(pairs))
    out[f"sm_{tag}_exclude"] = np.asarray(sorted(exclude or []), dtype=np.int64)


def _sample(rng, G, C, P, big_col=None, const_col=None):
    t = rng.randn(G, C * P).astype(np.float32)
    p = (t + 0.3 * rng.randn(G, C * P)).astype(np.float32)
    if big_col is not None:  # |mean| / std = 1e4
        t[:, big_col] = (5.0e4 + 5.0 * rng.randn(G)).astype(np.float32)
        p[:, big_col] = (t[:, big_col] + 2.0 * rng.randn(G)).astype(np.float32)
    if const_col is not None:
        t[:, const_col] = np.float32(3.1)
    return t, p


def main():
    from scipy.interpolate import RegularGridInterpolator  # noqa: F401  (the reference imports it lazily)
    from scipy.interpolate._rgi_cython import find_indices

    make_golden._placeholders()
    sys.path.insert(0, REF)
    pr, pp, itr = _script("predict"), _script("predict_pipeline"), _script("interpolate_to_region")
    out = {}

    # ---- StreamingMetrics
    rng = np.random.RandomState(21)
    C, P, G = 5, 3, 300
    pairs = [_sample(rng, G, C, P, big_col=7, const_col=3) for _ in range(3)]
    _sm_case(out, "excl", pr.StreamingMetrics(C, exclude_channels=[1, 4]), PROPS, C, [1, 4], pairs)
    _sm_case(out, "pipe", pp.StreamingMetrics(C), PIPE_PROPS, C, None, pairs)
    pairs1 = [_sample(rng, G, C, 1, big_col=2, const_col=0) for _ in range(2)]
    _sm_case(out, "onestep", pr.StreamingMetrics(C, exclude_channels=[4]), PROPS, C, [4], pairs1)
    lats, lons = pr.linspace_lats_lons(256, 512)
    ridx = pr.region_node_indices(*BOX, lats, lons)
    out["region_idx"] = ridx
    C, P = 19, 2
    pairsr = [_sample(rng, len(ridx), C, P, big_col=20, const_col=5) for _ in range(2)]
    _sm_case(out, "region", pr.StreamingMetrics(C, exclude_channels=[7, 18]), PROPS, C, [7, 18], pairsr)

    # ---- regridding 64 x 32 -> regional boxes
    g_lats, g_lons = pr.linspace_lats_lons(32, 64)
    gpred = rng.randn(32 * 64, 6).astype(np.float32)
    gpred[:, 4] += np.float32(250.0)
    out.update(rg_g_lats=g_lats, rg_g_lons=g_lons, rg_gpred=gpred)
    box_lats = np.linspace(50, 60, 41).astype(np.float32)
    box_lons = np.linspace(85, 100, 61).astype(np.float32)
    cases = {
        "box": (box_lats, box_lons),
        "desc": (box_lats[::-1].copy(), box_lons),
        "east": (box_lats, np.arange(355.0, 359.76, 0.25).astype(np.float32)),
        "edge": (np.array([-90, -87.09677, 0, 60, 84.193545, 90], dtype=np.float32),
                 np.array([0, 5.625, 180, 354.375, 359, 359.99], dtype=np.float32)),
    }
    for tag, (r_lats, r_lons) in cases.items():
        res = pp.interpolate_global_to_region(torch.from_numpy(gpred), g_lats, g_lons, r_lats, r_lons)
        lon_g, lat_g = np.meshgrid(r_lons, r_lats, indexing="ij")
        pts = np.stack([lon_g.ravel(), lat_g.ravel()], axis=1).astype(np.float64)
        idx, dist = find_indices((np.asarray(g_lons, float), np.asarray(g_lats, float)), pts.T.copy())
        out.update({f"rg_{tag}_lats": r_lats, f"rg_{tag}_lons": r_lons, f"rg_{tag}_out": res.numpy(),
                    f"rg_{tag}_idx": np.asarray(idx), f"rg_{tag}_dist": np.asarray(dist)})
    field = rng.randn(64, 32) * 3.0 + 10.0
    out["f2d_field"] = field
    out["f2d_out"] = itr.interpolate_field_2d(field, g_lons, g_lats, box_lons, box_lats)

    # ---- taper masks and the blend
    for n_lat, n_lon, w in ((41, 61, 0), (41, 61, 1), (41, 61, 3), (41, 61, 5), (5, 7, 3)):
        out[f"taper_{n_lat}_{n_lon}_{w}"] = pp.build_taper_mask_2d(n_lat, n_lon, w).numpy()
    mask = pp.build_taper_mask_2d(41, 61, 3)
    g_interp = torch.from_numpy(out["rg_box_out"])
    r_out = torch.from_numpy(rng.randn(41 * 61, 6).astype(np.float32))
    out["blend_r"] = r_out.numpy()
    out["blend_out"] = (mask * r_out + (1.0 - mask) * g_interp).numpy()

    path = os.path.join(HERE, "verify_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
