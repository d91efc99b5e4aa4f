"""WRF benchmark timing (graphcast_lite_amd.wrf; gcl_wrf_sample, gcl_wrf_scores, gcl_wrf_box_means).

The reference's sizes: a 96 x 84 WRF d03 grid (8064 points, synthetic curvilinear coordinates around Krasnoyarsk), the
`wb2_512x256_19f` series (32 steps, fp16, 19 channels) and forecasts of 131 072 nodes x 4 horizons x 19 channels in
batches of 8, synthetic data.

  sample      `gcl_wrf_sample`: 20 fields (4 variables x 5 steps) of the series onto the WRF points, one launch
  scores      `gcl_wrf_scores`: the 60 jobs of `compare_wrf_era5` (20 comparisons + each side's own mean), one call;
              and the 1408 jobs of one `WrfBenchmark.update` with `on_wrf_grid` (8 samples x 176 slots)
  box_means   `gcl_wrf_box_means`: one batch of 8 forecasts
  compare     `compare_wrf_era5` end to end (tables cached, WRF fields uploaded, one launch, one read-back; host clock)
  update      `WrfBenchmark.update` eager and `CapturedWrfBenchmark.update` replayed, with and without `on_wrf_grid`
  launches    kernels and copies of one eager update (torch profiler)

    python tools/wrf_bench.py [--iters 50] [--out FILE]

Prints one JSON line (and writes it to --out).
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

NAMES = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm", "t@850", "u@850", "v@850", "z@850", "q@850",
         "t@500", "u@500", "v@500", "z@500", "q@500"]
P_STEPS, B = 4, 8


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


def wrf_case(rng):
    """(fields, lat, lon, times, domain) like load_wrf_json: 25 hourly steps on a gently rotated 96 x 84 grid."""
    jj, ii = np.meshgrid(np.arange(84), np.arange(96))
    lon = (92.0 + 0.024 * jj + 0.002 * ii).astype(np.float32)
    lat = (55.4 + 0.0125 * ii - 0.001 * jj).astype(np.float32)
    times = ["2023-01-%02d_%02d:00:00" % (20 + h // 24, h % 24) for h in range(25)]
    fields = {"t2_K": 258 + 6 * rng.standard_normal((25, 96, 84)), "u10_ms": 3 * rng.standard_normal((25, 96, 84)),
              "v10_ms": 3 * rng.standard_normal((25, 96, 84)), "psfc_Pa": 98300 + 600 * rng.standard_normal((25, 96, 84))}
    fields = {k: v.astype(np.float32) for k, v in fields.items()}
    return fields, lat, lon, times, {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "wrf_bench needs a GPU"
    from graphcast_lite_amd import hip, wrf

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    case = wrf_case(rng)
    lons, lats = np.linspace(0, 360, 512, endpoint=False), np.linspace(-90, 90, 256)
    C, G = len(NAMES), 512 * 256
    series = torch.from_numpy((rng.standard_normal((32, 512, 256, C)) * 8).astype(np.float16)).to(dev)
    res = {"shape": {"wrf_points": 96 * 84, "series": list(series.shape), "G": G, "P": P_STEPS, "C": C, "B": B}}

    t = time.perf_counter()
    pos, w = wrf.wrf_point_tables(lons, lats, case[2], case[1])
    res["point_tables_first_call_s"] = time.perf_counter() - t
    src = hip.WrfSource(series, C, G, torch.from_numpy(np.array(pos)).to(dev), torch.from_numpy(np.array(w)).to(dev))
    offs = [(8 + h) * G * C + NAMES.index(n) for n in ("t2m", "10u", "10v", "sp") for h in range(5)]
    offs_d = torch.tensor(offs, dtype=torch.int64, device=dev)
    out = torch.empty(len(offs), 8064, dtype=torch.float64, device=dev)
    res["sample_20_fields"] = timed(lambda: hip.wrf_sample(src, offs, offs_d, out=out), args.iters, events=True)

    res["compare_wrf_era5"] = timed(lambda: wrf.compare_wrf_era5(case, series, lons, lats, NAMES), args.iters,
                                    events=False)
    pts = torch.from_numpy(np.stack([case[0][k][6 * h].reshape(-1) for k in wrf.VAR_MAP for h in range(5)])).to(dev)
    jobs, conv = [], []
    for a, (k, v) in enumerate(wrf.VAR_MAP.items()):
        kw = hip.WRF_POINT | (hip.WRF_CONVERT if v["era5_to_wrf"] != 1.0 else 0)
        for h in range(5):
            po, fo = (a * 5 + h) * 8064, offs[a * 5 + h]
            jobs += [(kw, po, hip.WRF_SRC0, fo, 0, 0), (kw, po, kw, po, 0, 0), (hip.WRF_SRC0, fo, hip.WRF_SRC0, fo, 0, 0)]
            conv += [(v["era5_to_wrf"], 0.0, 1.0, 0.0), (v["era5_to_wrf"], 0.0, v["era5_to_wrf"], 0.0), (1.0, 0.0, 1.0, 0.0)]
    jobs_d = torch.tensor(jobs, dtype=torch.int64, device=dev)
    conv_d = torch.tensor(conv, dtype=torch.float32, device=dev)
    stats = torch.empty(len(jobs), 6, dtype=torch.float64, device=dev)
    res["scores_60_jobs"] = timed(lambda: hip.wrf_scores(8064, jobs, conv, jobs_d, conv_d, src0=src, pts=pts.view(-1),
                                                         out=stats, validated=True), args.iters, events=True)

    mean = rng.normal(0, 5, C).astype(np.float32)
    std = rng.uniform(0.5, 6, C).astype(np.float32)
    pred = torch.randn(B, G, P_STEPS * C, device=dev)
    truth = pred + 0.1 * torch.randn_like(pred)
    offsets = list(range(3, 3 + B))
    wrf_means = {n: np.zeros(5, np.float32) for n in ("t2m", "10u", "10v", "sp")}

    def bench_of(cls, grid, **kw):
        return cls(mean, std, NAMES, lats, lons, P_STEPS, dev, wrf_means=wrf_means, wrf_times=case[3],
                   time_start="2023-01-18", wrf_fields=case, on_wrf_grid=grid, capacity=B, **kw)

    def one_update(b):
        b._count.zero_()
        b.n = 0
        b.update(pred, truth, offsets)

    plain = bench_of(wrf.WrfBenchmark, False)
    res["region_rows"] = int(plain.region_indices.size)
    state = torch.empty(B, P_STEPS * C, device=dev)
    res["box_means_B8"] = timed(lambda: hip.wrf_box_means(pred, plain._rows, G, plain._std, plain._mean, out=state,
                                                          validated=True), args.iters, events=True)
    for grid in (False, True):
        tag = "update_grid" if grid else "update"
        eager = bench_of(wrf.WrfBenchmark, grid)
        res[tag + "_eager"] = timed(lambda: one_update(eager), args.iters, events=False)
        res[tag + "_launches"] = device_activities(lambda: one_update(eager))
        cap = bench_of(wrf.CapturedWrfBenchmark, grid)
        for _ in range(4):
            one_update(cap)
        assert cap.graph_active, cap.launch_mode
        res[tag + "_captured"] = timed(lambda: one_update(cap), args.iters, events=False)
        if grid:
            jobs_b = eager._jobs(B, pred.stride(0), truth.stride(0))
            res["scores_update_jobs"] = len(jobs_b[0])
            srcs = [hip.WrfSource(x, x.stride(1), G, eager._pos, eager._w) for x in (pred, truth)]
            offs_t = torch.tensor(offsets, dtype=torch.int64, device=dev)
            res["scores_update_kernel"] = timed(
                lambda: hip.wrf_scores(8064, jobs_b[0], jobs_b[1], jobs_b[2], jobs_b[3], src0=srcs[0], src1=srcs[1],
                                       pts=eager._pts, slots=len(eager.slots), offsets=offs_t, target=eager.target,
                                       filled=eager._filled, accumulate=True, out=eager._stats, validated=True),
                args.iters, events=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
