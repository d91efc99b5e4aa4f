"""Learned-MOS timing (graphcast_lite_amd.mos): 512 x 256 grid, the 19 MOS stations, 40 steps, IDW on and off.

    python tools/mos_bench.py [--steps 40] [--iters 50] [--out profiles/mos_bench.json] [--reference DIR]

Prints one JSON line: `LearnedMOS.apply` eager and replayed from a hipGraph (device events, median ms), for a float32
forecast.  With --reference (a checkout of the reference project, CPU only) it also times the reference's
`apply_learned_mos_t2m` host loop on the same inputs (4 steps, as the loop grows linearly in the steps).  Per-kernel
medians come from a `rocprofv3 --kernel-trace --stats` run of this tool (profiles/mos_kernel_stats.csv).
"""
import argparse
import json
import os
import sys
import time
from datetime import datetime, timedelta

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STATIONS = [
    (56.173, 92.493, 287), (56.283, 90.517, 257), (56.200, 95.633, 207), (53.740, 91.385, 253),
    (57.683, 93.267, 93), (56.900, 93.133, 180), (56.967, 90.683, 181), (56.500, 93.283, 164),
    (56.217, 89.550, 290), (56.067, 92.733, 235), (56.117, 92.200, 479), (55.933, 92.283, 275),
    (57.633, 92.267, 179), (57.200, 94.550, 168), (56.650, 90.550, 231), (56.850, 95.217, 188),
    (56.033, 90.317, 256), (56.100, 91.667, 332), (56.167, 95.267, 357)]
VARS = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm",
        "t@850", "u@850", "v@850", "z@850", "q@850", "t@500", "u@500", "v@500", "z@500", "q@500"]
BUNDLE = os.path.join(ROOT, "tests", "golden", "mos_vectors.npz")


def grid():
    lats = np.linspace(-90, 90, 256, endpoint=True)
    lons = np.linspace(0, 360, 512, endpoint=False)
    return np.tile(lats, 512), np.repeat(lons, 256)


def inputs(steps):
    rng = np.random.default_rng(0)
    G = 512 * 256
    x = rng.standard_normal((G, steps, len(VARS))).astype(np.float32)
    x[..., 0] = 265.0 + 15.0 * x[..., 0]
    x[..., 5] = 95000.0 + 3000.0 * x[..., 5]
    x[..., 4] = 1e-3 * np.abs(x[..., 4])
    times = [datetime(2024, 1, 15) + timedelta(hours=6 * s) for s in range(steps)]
    return x, times


def stations():
    return [{"lat": a, "lon": o, "elev": e, "name": str(i)} for i, (a, o, e) in enumerate(STATIONS)]


def forest():
    from graphcast_lite_amd import mos

    z = np.load(BUNDLE)
    return mos.MOSForest(z["forest_feature"], z["forest_value"], z["forest_left"], z["forest_right"],
                         z["forest_missing_left"], z["forest_is_leaf"], z["forest_roots"], float(z["forest_baseline"]))


def time_device(fn, iters):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def time_reference(ref_dir, idw):
    import importlib.util
    import warnings

    warnings.filterwarnings("ignore")
    spec = importlib.util.spec_from_file_location(
        "_ref_mos", os.path.join(ref_dir, "src", "postprocessing", "mos_correction.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    bundle = ref.load_learned_mos(os.path.join(ref_dir, "live_runtime_bundle", "learned_mos_t2m.joblib"))
    x, times = inputs(4)
    lat, lon = grid()
    t = time.perf_counter()
    try:
        _, n = ref.apply_learned_mos_t2m(x, VARS, bundle, lat, lon, times, stations=stations(), spatial_idw=idw)
    except ValueError:  # math.sqrt(1 - a) with a > 1 at a node antipodal to a station
        return None, None
    return time.perf_counter() - t, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mos_bench.json"))
    ap.add_argument("--reference", default=None)
    a = ap.parse_args()
    res = {"grid": "512x256", "stations": len(STATIONS), "steps": a.steps, "dtype": "float32"}
    if a.reference:
        for idw in (False, True):
            s, n = time_reference(a.reference, idw)
            res[f"reference_cpu_4steps_{'idw' if idw else 'station'}_s"] = None if s is None else round(s, 3)
            res[f"reference_n_corrected_{'idw' if idw else 'station'}"] = None if n is None else int(n)
    else:
        import torch

        import graphcast_lite_amd  # noqa: F401
        from graphcast_lite_amd import mos

        f = forest()
        lat, lon = grid()
        x, times = inputs(a.steps)
        xd = torch.from_numpy(x).cuda()
        out = torch.empty_like(xd)
        for idw in (False, True):
            tag = "idw" if idw else "station"
            m = mos.LearnedMOS(f, VARS, lat, lon, stations(), idw)
            tf = m.time_features(times)
            res[f"apply_eager_{tag}_ms"] = round(time_device(lambda: m.apply(xd, tf, out=out), a.iters), 4)
            c = mos.CapturedLearnedMOS(f, VARS, lat, lon, stations(), idw)
            res[f"apply_captured_{tag}_ms"] = round(time_device(lambda: c(xd, tf), a.iters), 4)
            res[f"captured_{tag}_mode"] = c.launch_mode
            res[f"n_corrected_{tag}"] = int(c(xd, tf)[1].item())
            t = time.perf_counter()
            m.time_features(times)
            torch.cuda.synchronize()
            res[f"time_features_host_{tag}_ms"] = round(1e3 * (time.perf_counter() - t), 3)
        res["device"] = torch.cuda.get_device_name(0)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh)
            fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
