"""MOS/IDW sweep timing: one step of `LearnedMOS.sweep` (the ten settings of `mos.IDW_SWEEP_CONFIGS`, steps = 1, the
19 MOS stations) against the same answer without the sweep kernel - one `LearnedMOS.apply` plus one
`gcl_pipeline_sqerr` per setting.

    python tools/mos_sweep_bench.py [--iters 50] [--out profiles/mos_sweep_bench.json]

Runs on the 61 x 41 regional box and on the 512 x 256 global grid.  Prints one JSON line: device-event medians (ms) of
both ways, launched eagerly and replayed from a hipGraph, their ratios, and whether the two ways agree on the ten
sums.  Per-kernel medians come from a `rocprofv3 --kernel-trace --stats` run of this tool
(profiles/mos_sweep_kernel_stats.csv).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mos_bench import STATIONS, VARS, forest, stations, time_device  # noqa: E402
from mos_bench import grid as global_grid  # noqa: E402


def box_grid():
    lats = 50.0 + 0.25 * np.arange(41)
    lons = 85.0 + 0.25 * np.arange(61)
    return np.tile(lats, 61).astype(np.float32), np.repeat(lons, 41).astype(np.float32)


def inputs(G):
    rng = np.random.default_rng(0)
    x = rng.standard_normal((G, 1, len(VARS))).astype(np.float32)
    x[..., 0] = 265.0 + 15.0 * x[..., 0]
    x[..., 5] = 95000.0 + 3000.0 * x[..., 5]
    x[..., 4] = 1e-3 * np.abs(x[..., 4])
    truth = x[:, 0, :] + rng.normal(0.0, 2.0, (G, len(VARS))).astype(np.float32)
    return x, truth


def bench_grid(name, lat, lon, iters):
    import torch
    from datetime import datetime

    from graphcast_lite_amd import hip, mos
    from graphcast_lite_amd.capture import Captured

    class Replayed(Captured):
        def __init__(self, fn):
            Captured.__init__(self, use_graph=True, required=True)
            self.fn = fn

        def _work(self, x):
            return self.fn(x)

        def __call__(self, x):
            return self._run(x)

    f, cfgs = forest(), list(mos.IDW_SWEEP_CONFIGS)
    P, G, C = len(cfgs), lat.size, len(VARS)
    x, truth = inputs(G)
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(truth).cuda()
    t2m = td[:, 0:1]  # [G, 1], a strided view
    sweeper = mos.LearnedMOS(f, VARS, lat, lon, stations(), True)
    tf = sweeper.time_features([datetime(2020, 6, 1, 6)])
    acc_s = torch.zeros(P, 1, dtype=torch.float64, device="cuda")
    singles = [mos.LearnedMOS(f, VARS, lat, lon, stations(), True, pw, rad) for pw, rad, _ in cfgs]
    bufs = torch.empty(P, G, 1, C, device="cuda")
    acc_a = torch.zeros(P, 1, C, dtype=torch.float64, device="cuda")

    def sweep(xin):
        return sweeper.sweep(xin, tf, t2m, cfgs, acc_s)

    def apply_each(xin):
        for p, m in enumerate(singles):
            m.apply(xin, tf, out=bufs[p])
            hip.pipeline_sqerr(bufs[p].view(1, G, C), td, None, 0, acc_a[p:p + 1])
        return acc_a

    sweep(xd)
    apply_each(xd)
    torch.cuda.synchronize()
    same = bool(torch.equal(acc_s[:, 0], acc_a[:, 0, 0]))
    rel = float(((acc_s[:, 0] - acc_a[:, 0, 0]).abs() / acc_a[:, 0, 0]).max())
    res = {"rows": int(G), "points": sweeper.num_points, "sums_bit_equal": same, "sums_max_rel_diff": rel,
           "sweep_eager_ms": round(time_device(lambda: sweep(xd), iters), 4),
           "apply_each_eager_ms": round(time_device(lambda: apply_each(xd), iters), 4)}
    rs, ra = Replayed(sweep), Replayed(apply_each)
    res["sweep_graph_ms"] = round(time_device(lambda: rs(xd), iters), 4)
    res["apply_each_graph_ms"] = round(time_device(lambda: ra(xd), iters), 4)
    res["graph_modes"] = [rs.launch_mode, ra.launch_mode]
    res["speedup_eager"] = round(res["apply_each_eager_ms"] / res["sweep_eager_ms"], 2)
    res["speedup_graph"] = round(res["apply_each_graph_ms"] / res["sweep_graph_ms"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mos_sweep_bench.json"))
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("the median needs at least 20 timed runs")
    import torch

    import graphcast_lite_amd  # noqa: F401

    res = {"settings": 10, "steps": 1, "stations": len(STATIONS), "dtype": "float32", "iters": a.iters,
           "box_61x41": bench_grid("box", *box_grid(), a.iters),
           "global_512x256": bench_grid("global", *global_grid(), a.iters),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
