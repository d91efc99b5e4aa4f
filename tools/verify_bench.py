"""Device-event timings of forecast scoring and regional blending on the HIP path (graphcast_lite_amd.verify).

(a) One sample's full `scripts/predict.py` metric set at 512 x 256, 19 channels, 4 steps: prediction and persistence,
    overall and per horizon, on the whole grid and on the DA box 50-60N x 83-98E (294 nodes), 20 objects.
    `ForecastVerifier.update` eager and captured in a hipGraph, the statistics call of the whole grid alone with its
    algorithmic bytes (truth + prediction + the distinct persistence columns, read once) and GB/s, and the same metric
    set done the reference's way (written here): the forecast, truth and input window copied to the host, then the
    per-column torch CPU loop of every object with 16 threads (wall time).
(b) `GlobalRegionalForecast` (64 x 32 GCN global model, 61 x 41 regional model on a pruned mesh, 19 channels):
    captured against eager.

    python tools/verify_bench.py [--steps K] [--warmup W] [--parts ab]

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
sys.path.insert(0, os.path.join(ROOT, "tests"))

BOX = (50.0, 60.0, 83.0, 98.0)


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


def host_update(C, excl, y, p):
    """One StreamingMetrics update the reference's way: per-column torch CPU reductions with a .item() each."""
    se_ch, acc_ch = np.zeros(C), np.zeros(C)
    for c in range(y.shape[1]):
        yt, yp = y[:, c], p[:, c]
        se_ch[c % C] += (yp - yt).pow(2).sum().item()
        ta, pa = yt - yt.mean(), yp - yp.mean()
        acc_ch[c % C] += ((ta * pa).sum() / (ta.norm() * pa.norm() + 1e-8)).item()
    keep = [c for c in range(y.shape[1]) if c % C not in excl]
    err = (p - y)[:, keep]
    return se_ch, acc_ch, err.pow(2).sum().item(), err.abs().sum().item()


def part_a(args, dev):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd import verify as V

    lats, lons = V.linspace_lats_lons(256, 512)
    G, C, P = 256 * 512, 19, 4
    K = C * P
    ridx = V.region_node_indices(*BOX, lats, lons)
    excl = [17, 18]
    g = torch.Generator().manual_seed(1)
    y = torch.randn(G, K, generator=g).to(dev)
    out = (y.cpu() + 0.3 * torch.randn(G, K, generator=g)).to(dev)
    X = torch.randn(G, 2 * C, generator=g).to(dev)
    base = V.Persistence(X, C)
    ver = V.ForecastVerifier(C, P, exclude_channels=excl, region_idxs=ridx, device=dev)
    t_eager = timed(lambda: ver.update(y, pred=out, base=base), args.steps, args.warmup)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ver.update(y, pred=out, base=base)
    t_graph = timed(graph.replay, args.steps, args.warmup)

    T3, P3, X3 = y.unsqueeze(0), out.unsqueeze(0), X.unsqueeze(0)
    stats = torch.empty(1, 2, K, 3, dtype=torch.float64, device=dev)
    cmap = base.column_map(K)
    t_stats = timed(lambda: hip.verify_colstats(T3, [(P3, None), (X3, cmap)], None, stats), args.steps * 5,
                    args.warmup)
    nbytes = G * K * 4 * 2 + G * C * 4

    # the reference's way (scripts/predict.py:574-600): host copies, then every object's per-column loop
    torch.set_num_threads(16)
    rows = torch.from_numpy(ridx)

    def host_set():
        yc, oc, xc = y.cpu(), out.cpu(), X.cpu()
        bl = xc[:, -C:].repeat(1, P)
        for pred in (oc, bl):
            host_update(C, excl, yc, pred)
            for p in range(P):
                host_update(C, excl, yc[:, p * C:(p + 1) * C], pred[:, p * C:(p + 1) * C])
            yr, pr = yc[rows], pred[rows]
            host_update(C, excl, yr, pr)
            for p in range(P):
                host_update(C, excl, yr[:, p * C:(p + 1) * C], pr[:, p * C:(p + 1) * C])
    host_set()
    reps = max(1, args.steps // 10)
    t0 = time.perf_counter()
    for _ in range(reps):
        host_set()
    t_host = (time.perf_counter() - t0) / reps * 1e3
    return {"a_grid_points": G, "a_channels": C, "a_ar_steps": P, "a_region_nodes": int(len(ridx)),
            "a_objects": len(ver._objects), "a_update_eager_ms": round(t_eager, 4),
            "a_update_captured_ms": round(t_graph, 4), "a_stats_ms": round(t_stats, 4), "a_stats_bytes": nbytes,
            "a_stats_GBps": round(nbytes / (t_stats * 1e-3) / 1e9, 1), "a_host_ref_ms": round(t_host, 1),
            "a_host_threads": torch.get_num_threads(), "a_speedup_vs_host": round(t_host / t_graph, 1)}


def part_b(args, dev):
    from test_verify import _global_config
    from graphcast_lite_amd import verify as V
    from graphcast_lite_amd.experiments import experiment
    from graphcast_lite_amd.models import WeatherPrediction

    C = 19
    gcfg = _global_config(C)
    torch.manual_seed(42)
    g_lats, g_lons = V.linspace_lats_lons(32, 64)
    gm = WeatherPrediction((g_lats.astype(np.float32), g_lons.astype(np.float32)), gcfg.graph, gcfg.pipeline,
                           gcfg.data, dev)
    rcfg = experiment("region_krsk_cds_19f", mesh_levels=[3, 5])
    rcfg.pipeline.processor.gcn.num_message_passing_steps = 2
    r_lats, r_lons = np.linspace(50, 60, 41).astype(np.float32), np.linspace(85, 100, 61).astype(np.float32)
    rm = WeatherPrediction((r_lats, r_lons), rcfg.graph, rcfg.pipeline, rcfg.data, dev,
                           region_bounds=(50.0, 60.0, 85.0, 100.0), mesh_buffer=15.0)
    g = torch.Generator().manual_seed(3)
    gX = torch.randn(1, 32 * 64, 2 * C, generator=g).to(dev)
    rX = torch.randn(1, 41 * 61, 2 * C, generator=g).to(dev)
    eager = V.GlobalRegionalForecast(gm, rm, (g_lats, g_lons), (r_lats, r_lons), taper_width=3, horizons=1)
    cap = V.CapturedGlobalRegionalForecast(gm, rm, (g_lats, g_lons), (r_lats, r_lons), taper_width=3, horizons=1)
    t_eager = timed(lambda: eager(gX, rX), args.steps, args.warmup)
    t_cap = timed(lambda: cap(gX, rX), args.steps, args.warmup)
    return {"b_global_grid": "64x32", "b_region_grid": "61x41", "b_channels": C, "b_captured": cap.graph_active,
            "b_eager_ms": round(t_eager, 4), "b_captured_ms": round(t_cap, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parts", default="ab")
    args = ap.parse_args()
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "verify_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    res = {"tool": "verify_bench", "steps": args.steps, "warmup": args.warmup}
    with torch.no_grad():
        if "a" in args.parts:
            res.update(part_a(args, dev))
        if "b" in args.parts:
            res.update(part_b(args, dev))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
