"""Device-event timings of data assimilation on the HIP path (graphcast_lite_amd.assimilation).

(a) The reference's DA-experiment shape: the `wb2_512x256_19f_ar` model at batch 1, 4 AR steps, OI on the
    50-60N x 83-98E box (grid indices numbered as the reference's predict script numbers them, 294 nodes) with 10 %
    stations (seed 42), all 19 channels, sigma_b 0.8, sigma_o 0.5, L 150 km.  ms per sample of the captured assimilated
    rollout against the plain `CapturedRollout` (both without the residual, as the reference's DA loops run).
(b) Full-grid OI on all 131 072 nodes of the 512 x 256 grid (the reference would need a 68 GB B), 1 % and 5 %
    stations, 19 channels: the one-off factor, one `OINetwork.apply`, and the analysis kernel's node x station pairs
    per second.

    python tools/assim_bench.py [--steps K] [--warmup W] [--parts ab]

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOX = (50.0, 60.0, 83.0, 98.0)
SIGMA_B, SIGMA_O, L_M = 0.8, 0.5, 150e3


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def region_rows(lats, lons):
    li = np.where((lats >= BOX[0]) & (lats <= BOX[1]))[0]
    lj = np.where((lons >= BOX[2]) & (lons <= BOX[3]))[0]
    return (lj[:, None] * len(lats) + li[None, :]).ravel().astype(np.int64)


def part_a(args, dev, lats, lons):
    from graphcast_lite_amd.assimilation import CapturedAssimilatedRollout, OptimalInterpolation
    from graphcast_lite_amd.experiments import experiment
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.predict import CapturedRollout

    cfg = experiment("wb2_512x256_19f_ar")
    torch.manual_seed(42)
    model = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev)
    G, C, P = len(lats) * len(lons), cfg.data.num_features_used, 4
    roi = region_rows(lats, lons)
    rng = np.random.RandomState(42)
    st = np.sort(rng.choice(roi, max(1, int(len(roi) * 0.1)), replace=False))
    oi = OptimalInterpolation(lats, lons, SIGMA_B, SIGMA_O, L_M, dev, roi_idx=roi)
    net = oi.prepare_network(st)
    g = torch.Generator().manual_seed(1234)
    X = torch.randn(1, G, cfg.data.obs_window_used * C, generator=g).to(dev)
    truth = torch.randn(1, G, P * C, generator=g)
    obs = torch.full_like(truth, float("nan"))
    obs[:, st] = truth[:, st]
    obs = obs.to(dev)
    plain = CapturedRollout(model, P, use_residual=False)
    assim = CapturedAssimilatedRollout(model, P, net, use_residual=False)
    t_plain = timed(lambda: plain(X), args.steps, args.warmup)
    t_assim = timed(lambda: assim(X, obs), args.steps, args.warmup)
    t_plain2 = timed(lambda: plain(X), args.steps, args.warmup)  # the plain rollout again: run-to-run spread
    ch = list(range(C))
    net.prepare(C, 1)
    xa = X[:, :, :C].contiguous()
    o1 = obs[:, :, :C]
    t_oi = timed(lambda: net.apply_(xa, o1), args.steps * 10, args.warmup)
    return {"a_grid_points": G, "a_roi_nodes": int(len(roi)), "a_stations": int(len(st)), "a_channels": len(ch),
            "a_ar_steps": P, "a_batch": 1, "a_captured": assim.graph_active and plain.graph_active,
            "a_rollout_ms": round(t_plain, 3), "a_rollout_repeat_ms": round(t_plain2, 3),
            "a_assim_rollout_ms": round(t_assim, 3), "a_assim_cost_ms": round(t_assim - min(t_plain, t_plain2), 3),
            "a_oi_apply_eager_ms": round(t_oi, 4)}


def part_b(args, dev, lats, lons, frac):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd.assimilation import OptimalInterpolation

    G, C = len(lats) * len(lons), 19
    rng = np.random.RandomState(42)
    st = np.sort(rng.choice(G, int(G * frac), replace=False))
    oi = OptimalInterpolation(lats, lons, SIGMA_B, SIGMA_O, L_M, dev)
    oi._setup()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.time()
    a.record()
    net = oi.prepare_network(st)
    b.record()
    torch.cuda.synchronize()
    t_factor_wall = time.time() - t0
    t_factor = a.elapsed_time(b)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, G, C, generator=g).to(dev)
    y = torch.full((1, G, C), float("nan"))
    y[:, st] = torch.randn(1, len(st), C, generator=g)
    y = y.to(dev)
    out = torch.empty_like(x)
    net.apply(x, y, out=out)
    t_apply = timed(lambda: net.apply(x, y, out=out), args.steps, args.warmup)
    chans, rhs, tmp, W = net._workspace(1, C)
    t_solve = timed(lambda: hip.oi_solve(net.fac.M, rhs, tmp, W), args.steps, args.warmup)
    t_an = timed(lambda: hip.oi_analysis(x, out, chans, None, oi._nodes, net.fac.stations, W, oi._sb2, oi._rl2,
                                         oi._th_cut, oi._a_cut), args.steps, args.warmup)
    m = len(st)
    k = f"b{int(round(frac * 100))}"
    return {f"{k}_stations": m, f"{k}_factor_ms": round(t_factor, 2), f"{k}_factor_wall_s": round(t_factor_wall, 3),
            f"{k}_apply_ms": round(t_apply, 4), f"{k}_solve_ms": round(t_solve, 4),
            f"{k}_analysis_ms": round(t_an, 4), f"{k}_pairs_per_s": float(f"{G * m / (t_an * 1e-3):.4g}"),
            f"{k}_factor_bytes": m * m * 8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parts", default="ab")
    args = ap.parse_args()
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "assim_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    lats = np.linspace(-90, 90, 256, endpoint=True)
    lons = np.linspace(0, 360, 512, endpoint=False)
    res = {"tool": "assim_bench", "sigma_b": SIGMA_B, "sigma_o": SIGMA_O, "L_m": L_M, "steps": args.steps,
           "warmup": args.warmup}
    if "a" in args.parts:
        res.update(part_a(args, dev, lats, lons))
    if "b" in args.parts:
        for frac in (0.01, 0.05):
            res.update(part_b(args, dev, lats, lons, frac))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
