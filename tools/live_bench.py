"""Live forecast timing (graphcast_lite_amd.live; gcl_live_frame_pack, gcl_live_region_stats).

`wb2_512x256_19f_ar` model (131 072 nodes, 19 channels, obs_window 2), 4 AR steps, a 721 x 1440 source grid (0.25 deg,
latitudes descending) with 16 fields per cycle (tp absent, z_surf / lsm from the template), learned MOS, synthetic data.

  pack        one cycle into one window slot: from host arrays (arena assembled on the host, one upload, one launch;
              host clock around a synchronise), from device-resident fields (one concatenation, one launch; device
              events) and the kernel alone on a prepared arena (device events)
  forecast    `LiveForecaster.forecast` after its capture, fields on the host / on the device, against
              `predict.CapturedRollout` alone on the same window: the difference is ingest plus post-processing
  launches    kernels and copies of one eager forecast and of the eager rollout inside it (torch profiler)
  hindcast    `hindcast` of 8 anchors over 9 frames against `forecast` called 8 times, per anchor

    python tools/live_bench.py [--iters 20] [--out FILE]

Prints one JSON line (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time
from datetime import datetime, timedelta, timezone

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = 4
BBOX = (50.0, 62.0, 85.0, 100.0)
T0 = datetime(2024, 2, 28, 18, tzinfo=timezone.utc)


def timed(fn, iters, events, warmup=3):
    """Median / min / max ms of fn: device events, or a host clock around a synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        if events:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        else:
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t))
    return {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts), "iters": iters,
            "clock": "device events" if events else "host clock + synchronise"}


def device_activities(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if e.device_type.name != "CPU"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "live_bench needs a GPU"
    import bench
    from graphcast_lite_amd import hip, live, mos, predict

    dev = torch.device("cuda:0")
    cfg, model, (nlat, nlon) = bench.build_model("wb2_512x256_19f_ar", dev)
    model.eval()
    lats, lons = np.linspace(-90, 90, nlat), np.linspace(0, 360, nlon, endpoint=False)
    node_lat, node_lon = np.tile(lats, nlon).astype(np.float32), np.repeat(lons, nlat).astype(np.float32)
    G, names = node_lat.size, list(live.DEFAULT_VAR_ORDER)
    C = len(names)
    src_lat, src_lon = np.linspace(90, -90, 721), 0.25 * np.arange(1440)

    def fields(k):
        r = np.random.default_rng(k)
        return {n: (r.standard_normal((721, 1440)).astype(np.float32), src_lat, src_lon) for n in names
                if n not in ("tp", "z_surf", "lsm")}

    rng = np.random.default_rng(0)
    x_mean, x_std = np.zeros(C, np.float32), np.ones(C, np.float32)
    x_std[[names.index("msl"), names.index("sp")]] = 0.01
    y_mean, y_std = rng.normal(0, 5, C).astype(np.float32), rng.uniform(0.5, 6, C).astype(np.float32)
    y_mean[0] = 265.0
    statics = {"z_surf": rng.standard_normal(G).astype(np.float32), "lsm": (rng.random(G) < 0.3).astype(np.float32)}
    gm = np.load(os.path.join(ROOT, "tests", "golden", "mos_vectors.npz"))
    forest = mos.MOSForest(gm["forest_feature"], gm["forest_value"], gm["forest_left"], gm["forest_right"],
                           gm["forest_missing_left"], gm["forest_is_leaf"], gm["forest_roots"],
                           float(gm["forest_baseline"]))
    host = [fields(k) for k in range(3)]
    ondev = [{n: (torch.from_numpy(v).to(dev), la, lo) for n, (v, la, lo) in f.items()} for f in host]
    res = {"shape": {"G": G, "C": C, "obs": model.obs_window, "steps": STEPS, "source": [721, 1440],
                     "fields_per_cycle": len(host[0])}}

    t = time.perf_counter()
    live.point_tables(src_lat, src_lon, node_lat, node_lon)
    res["point_tables_first_call_s"] = time.perf_counter() - t
    packer = live.LiveFramePacker(names, node_lat, node_lon, x_mean, x_std, statics, dev)
    X = torch.empty(G, model.obs_window * C, device=dev)
    res["pack_host_fields"] = timed(lambda: packer.pack(host[0], X, [0]), args.iters, events=False)
    res["pack_device_fields"] = timed(lambda: packer.pack(ondev[0], X, [0]), 50, events=True)
    present = [n for n in names if n in host[0]]
    chan, pos, w, total = packer._plan(present, host[0])
    arena = packer._arena(present, ondev[0], total)
    res["pack_kernel"] = timed(lambda: hip.live_frame_pack(arena, packer._statics, chan, packer._div, pos, w, packer._mean,
                                                           packer._std, X, [0], X.stride(0), G, C), 200, events=True)
    res["pack_kernel_bytes"] = {"stored": G * C * 4, "tables": int(pos.numel() * 4 + w.numel() * 8),
                                "arena": int(arena.numel() * 4)}

    def forecaster(use_graph):
        return live.LiveForecaster(model, names, node_lat, node_lon, (x_mean, x_std, y_mean, y_std), statics, STEPS, True,
                                   learned_mos=forest, city_bbox=BBOX, use_graph=use_graph)

    six = timedelta(hours=6)
    cyc_host, cyc_dev = [(T0, host[0]), (T0 + six, host[1])], [(T0, ondev[0]), (T0 + six, ondev[1])]
    fc = forecaster(True)
    for _ in range(4):
        out = fc.forecast(cyc_host)
    assert fc.graph_active
    res["forecast_host_fields"] = timed(lambda: fc.forecast(cyc_host), args.iters, events=False)
    res["forecast_device_fields"] = timed(lambda: fc.forecast(cyc_dev), args.iters, events=True)
    X3 = out["input_normalized"].unsqueeze(0).contiguous()
    cr = predict.CapturedRollout(model, STEPS, use_residual=True)
    for _ in range(4):
        cr(X3)
    assert cr.graph_active
    res["captured_rollout"] = timed(lambda: cr(X3), args.iters, events=True)

    eager = forecaster(False)
    eager.forecast(cyc_dev)
    n_all = device_activities(lambda: eager.forecast(cyc_dev))
    n_roll = device_activities(lambda: predict.rollout(model, X3, STEPS, use_residual=True))
    res["launches"] = {"forecast_eager": n_all, "rollout_eager": n_roll, "ingest_and_post": n_all - n_roll}

    frames = [(T0 + k * six, ondev[k % 3]) for k in range(9)]
    anchors = list(range(1, 9))
    for _ in range(4):
        fc.hindcast(frames, anchors)

    def one_by_one():
        for a in anchors:
            fc.forecast(frames[a - 1:a + 1])

    h = timed(lambda: fc.hindcast(frames, anchors), 10, events=False)
    e = timed(one_by_one, 10, events=False)
    res["hindcast_B8"], res["forecast_x8"] = h, e
    res["per_anchor_ms"] = {"hindcast": h["median_ms"] / 8, "forecast_x8": e["median_ms"] / 8}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
