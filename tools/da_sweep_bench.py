"""DA grid search timing (graphcast_lite_amd.pipeline.DaSweep, gcl_oi_analysis_rows).

(a) The whole sweep: `da_grid_search.sh`'s 20 settings plus the no-DA row on the `wb2_512x256_19f_ar` model, 4 AR
    steps, stations drawn in the 50-60N x 83-98E box (294 nodes), synthetic data.  ms per sample of `DaSweep` (one
    captured rollout at batch 21, then 21 verifier updates) against one captured rollout per setting at batch 1, summed
    (`CapturedAssimilatedRollout` with that setting's own assimilator; `CapturedRollout` for the no-DA row).
(b) The analysis kernel alone: one `gcl_oi_analysis_rows` launch for the 6 OI settings of one density (corr_len 5 / 10 /
    50 km x sigma_o 0.3 / 0.5, 19 channels) against six `gcl_oi_analysis` launches, on the box (294 OI nodes, 29
    stations) and on the full 512 x 256 grid (131 072 nodes, 1 310 stations).

    python tools/da_sweep_bench.py --part a [--iters 20]
    python tools/da_sweep_bench.py --part b --shape large|small [--iters 30]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/da_sweep_bench.py --part b --shape large
    python tools/da_sweep_bench.py --summarise DIR    # medians per kernel from the kernel trace under DIR

Every mode prints one JSON line.  Device-event medians are reported by the tool itself; the per-kernel figures of (b)
come from the kernel trace (the six launches are summed per repetition, then the median is taken).
"""
import argparse
import csv
import glob
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = (50.0, 60.0, 83.0, 98.0)
AR_STEPS = 4


def axes():
    return np.linspace(-90, 90, 256, endpoint=True), np.linspace(0, 360, 512, endpoint=False)


def box_rows(lats, lons):
    li = np.where((lats >= BOX[0]) & (lats <= BOX[1]))[0]
    lj = np.where((lons >= BOX[2]) & (lons <= BOX[3]))[0]
    return (lj[:, None] * len(lats) + li[None, :]).ravel().astype(np.int64)


def median_ms(fn, iters, warmup=3):
    import torch

    for _ in range(warmup):
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


def alternating_ms(f1, f2, iters, warmup=3):
    """Medians of two ways timed in turn, so that a drift of the clock or the box hits both alike."""
    import torch

    def once(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    t1, t2 = [], []
    for i in range(warmup + iters):
        t1.append(once(f1))
        t2.append(once(f2))
    return float(np.median(t1[warmup:])), float(np.median(t2[warmup:]))


class SyntheticDS:
    def __init__(self, n, G, C, obs, dev):
        import torch

        g = torch.Generator().manual_seed(1234)
        self.device, self.coordinates, self.flat_grid = dev, axes(), False
        self.X = torch.randn(n, G, obs * C, generator=g).to(dev)
        self.Y = torch.randn(n, G, AR_STEPS * C, generator=g).to(dev)

    def __len__(self):
        return self.X.shape[0]

    def batch(self, indices):
        i = int(indices[0])
        return self.X[i:i + 1], self.Y[i:i + 1]


def part_a(iters):
    import torch

    from graphcast_lite_amd import assimilation as A
    from graphcast_lite_amd.experiments import experiment
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.pipeline import DaSweep
    from graphcast_lite_amd.predict import CapturedRollout

    dev = torch.device("cuda:0")
    lats, lons = axes()
    cfg = experiment("wb2_512x256_19f_ar")
    torch.manual_seed(42)
    model = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev)
    G, C, obs = len(lats) * len(lons), cfg.data.num_features_used, cfg.data.obs_window_used
    roi = box_rows(lats, lons)
    settings = A.da_grid(baseline=True)
    ds = SyntheticDS(2, G, C, obs, dev)
    sweep = DaSweep(model, ds, settings, AR_STEPS, roi, region_idxs=roi)
    for _ in range(3):
        sweep.update([0])
    t_update = median_ms(lambda: sweep.update([1]), iters)
    X, Y = ds.batch([1])
    XS = X.expand(len(settings), -1, -1)
    t_rollout = median_ms(lambda: sweep._rollout(XS, Y, None), iters)
    eager = A.DASweepAssimilator((lats, lons), settings, roi, 42, roi_idx=roi, device=dev)
    step = torch.randn(len(settings), G, C, device=dev)
    t_apply = median_ms(lambda: eager.apply_(step, Y[:, :, :C]), iters)
    each = A.DASweepAssimilator((lats, lons), settings, roi, 42, roi_idx=roi, device=dev, per_setting=True)
    t_apply_each = median_ms(lambda: each.apply_(step, Y[:, :, :C]), iters)

    # the parent's way: one captured rollout per setting at batch 1
    total, captured = 0.0, sweep.graph_active
    for s in settings:
        if s.method == "none":
            run = CapturedRollout(model, AR_STEPS, use_residual=False)
            fn = lambda run=run: run(X)  # noqa: E731
        else:
            st = A.station_network(roi, s.sparsity, 42)
            if s.method == "nudging":
                asm = A.NudgingAssimilator(alpha=s.alpha, device=dev)
            else:
                asm = A.OptimalInterpolation(lats, lons, s.sigma_b, s.sigma_o, s.corr_len, dev,
                                             roi_idx=roi).prepare_network(st)
            obs_s = torch.full_like(Y, float("nan"))
            obs_s[:, st] = Y[:, st]
            run = A.CapturedAssimilatedRollout(model, AR_STEPS, asm, use_residual=False)
            fn = lambda run=run, obs_s=obs_s: run(X, obs_s)  # noqa: E731
        total += median_ms(fn, iters)
        captured = captured and run.graph_active
    return {"part": "a", "model": "wb2_512x256_19f_ar", "grid_points": G, "channels": C, "ar_steps": AR_STEPS,
            "settings": len(settings), "box_nodes": int(len(roi)),
            "stations": {str(d): int(len(v)) for d, v in sweep.assimilator.networks.items()}, "all_captured": captured,
            "sweep_rollout_ms": round(t_rollout, 3), "sweep_update_ms": round(t_update, 3),
            "per_setting_rollouts_ms": round(total, 3), "ratio_rollouts": round(total / t_rollout, 2),
            "ratio_against_update": round(total / t_update, 2),
            "sweep_assimilation_step_ms": round(t_apply, 4), "per_setting_assimilation_step_ms": round(t_apply_each, 4)}


def part_b(shape, iters):
    import torch

    from graphcast_lite_amd import assimilation as A
    from graphcast_lite_amd import hip

    dev = torch.device("cuda:0")
    lats, lons = axes()
    G, C = len(lats) * len(lons), 19
    if shape == "small":
        pool, roi, sparsity = box_rows(lats, lons), box_rows(lats, lons), 0.1
    else:
        pool, roi, sparsity = np.arange(G), None, 0.01
    settings = A.da_grid(nudging_alphas=(), sparsities=(sparsity,))
    sw = A.DASweepAssimilator((lats, lons), settings, pool, 42, roi_idx=roi, device=dev)
    sw.prepare(C)
    g = sw._groups[0]
    n, nch = g["n"], C
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(n, G, C, generator=gen).to(dev)
    truth = torch.randn(1, G, C, generator=gen).to(dev)
    sw.apply_(x.clone(), truth)  # fills W
    xa_rows, xa_six = x.clone(), x.clone()
    fac, W = g["fac"], g["W"]

    def rows():
        hip.oi_analysis_rows(x, xa_rows, g["chans"], g["node_row"], g["nodes"], fac.stations, W, g["sb2"], g["rl2"],
                             g["th_cut"], g["a_cut"])

    def six():
        for j, net in enumerate(g["nets"]):
            o = net.oi
            hip.oi_analysis(x[j:j + 1], xa_six[j:j + 1], g["chans"], o._node_row, o._nodes, fac.stations,
                            W[j * nch:(j + 1) * nch], o._sb2, o._rl2, o._th_cut, o._a_cut)

    rows()
    six()
    torch.cuda.synchronize()
    same = bool(torch.equal(xa_rows, xa_six))
    t_rows, t_six = alternating_ms(rows, six, iters)
    return {"part": "b", "shape": shape, "oi_nodes": int(g["nodes"][0].numel()), "stations": int(fac.m), "settings": n,
            "channels": nch, "corr_len_km": [s.corr_len / 1000 for s in sw.settings_by_row],
            "bit_equal": same, "rows_event_ms": round(t_rows, 4), "six_event_ms": round(t_six, 4),
            "six_over_rows_event": round(t_six / t_rows, 3)}


def summarise(directory):
    """Median kernel time (us) of the rows launch and of the six single-setting launches (summed per repetition) from a
    rocprofv3 kernel trace; the first 4 repetitions (set-up and warm-up) are dropped."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel trace under {directory}")
    rows, single = [], []
    with open(files[0]) as fh:
        recs = sorted(csv.DictReader(fh), key=lambda r: int(r["Start_Timestamp"]))
    for r in recs:
        dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        if "oi_analysis_rows_kernel" in r["Kernel_Name"]:
            rows.append(dur)
        elif "oi_analysis_kernel" in r["Kernel_Name"]:
            single.append(dur)
    sixes = [sum(single[i:i + 6]) for i in range(0, len(single) - len(single) % 6, 6)]
    rows, sixes = rows[4:], sixes[4:]
    if len(rows) < 20 or len(sixes) < 20:
        raise SystemExit(f"the medians need at least 20 launches each, got {len(rows)} and {len(sixes)}")
    names = sorted({m.group(0) for r in recs for m in [re.search(r"oi_analysis\w*<[^>]*>", r["Kernel_Name"])] if m})
    return {"trace": os.path.relpath(files[0], directory), "kernels": names, "launches": [len(rows), len(sixes)],
            "rows_kernel_us": round(float(np.median(rows)), 2), "six_kernels_us": round(float(np.median(sixes)), 2),
            "six_over_rows": round(float(np.median(sixes) / np.median(rows)), 3),
            "rows_kernel_us_p10_p90": [round(float(np.percentile(rows, p)), 2) for p in (10, 90)],
            "six_kernels_us_p10_p90": [round(float(np.percentile(sixes, p)), 2) for p in (10, 90)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"], default="a")
    ap.add_argument("--shape", choices=["small", "large"], default="large")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--summarise", metavar="DIR")
    a = ap.parse_args()
    if a.summarise:
        print(json.dumps(summarise(a.summarise)))
        return
    if a.iters < 20:
        ap.error("the median needs at least 20 timed runs")
    import torch

    assert torch.cuda.is_available(), "da_sweep_bench needs a GPU"
    res = part_a(a.iters) if a.part == "a" else part_b(a.shape, a.iters)
    res.update(tool="da_sweep_bench", iters=a.iters, device=torch.cuda.get_device_name(0))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
