"""Timings of the inference loop and of the regional scoring of a saved bundle (graphcast_lite_amd.predict / .verify).

(a) `predict_experiment` at the `baseline` shape (64 x 32 grid, 33 channels, GCN processor), AR 4, hipGraph on, over N
    synthetic samples that already sit on the device, for `--batch-size` 1 and 8: samples per second of the whole call
    (rollouts, scores, the warm-up and capture of its own graph, the final host read), host clock around a call that ends
    in a device-to-host copy.  The two batch sizes alternate, `--repeats` times each.
(b) The same with optimal interpolation on a 10 % station network over the whole grid (sigma_b 0.8, sigma_o 0.5,
    correlation length 1000 km), observations cut from the truth on the device.
(c) `gcl_region_interp_scores` for 200 samples x 4 horizons x 19 channels from 512 x 256 onto 61 x 41: device events
    around the launch pair (forecast, tables and regional series resident on the device), with and without the stored
    fields, its algorithmic bytes (the DISTINCT forecast rows the regional cells touch and the distinct steps of the
    fp16 series, each once, + the stored fields) and GB/s, and the host pooling of the [P, C, 11] sums.

    python tools/predict_bench.py [--samples N] [--repeats R] [--parts abc]

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


class DeviceSamples:
    def __init__(self, X, y):
        self.X, self.y = X, y

    def __len__(self):
        return self.X.shape[0]

    def batch(self, indices, out=None):
        return self.X[indices[0]:indices[-1] + 1], self.y[indices[0]:indices[-1] + 1]


def part_ab(args, dev, with_oi):
    from graphcast_lite_amd import predict as P
    from graphcast_lite_amd.assimilation import OptimalInterpolation, station_network
    from graphcast_lite_amd.experiments import GRID, experiment
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.verify import linspace_lats_lons

    cfg = experiment("baseline")
    nlat, nlon = GRID["baseline"]
    lats, lons = linspace_lats_lons(nlat, nlon)
    torch.manual_seed(42)
    model = WeatherPrediction((lats.astype(np.float32), lons.astype(np.float32)), cfg.graph, cfg.pipeline, cfg.data, dev)
    model = model.to(dev).eval()
    C, AR, G, N = cfg.data.num_features_used, 4, nlat * nlon, args.samples
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.randn(N, G, 2 * C, generator=g, device=dev)
    y = X[:, :, -C:].repeat(1, 1, AR) + 0.1 * torch.randn(N, G, AR * C, generator=g, device=dev)
    ds = DeviceSamples(X, y)
    kw = {}
    if with_oi:
        stations = station_network(np.arange(G), 0.1, 42)
        kw = dict(assim_method="oi", oi=OptimalInterpolation(lats, lons, 0.8, 0.5, 1.0e6, dev), station_rows=stations)
    quiet = lambda s="": None  # noqa: E731
    rates = {1: [], 8: []}
    for r in range(args.repeats + 1):  # round 0 warms the libraries up and is dropped
        for bs in (1, 8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run = P.predict_experiment(model, ds, C, AR, batch_size=bs, grid=(nlon, nlat), use_graph=True, device=dev,
                                       say=quiet, **kw)
            dt = time.perf_counter() - t0
            assert run.n_samples == N
            if r:
                rates[bs].append(N / dt)
    tag = "b_oi" if with_oi else "a"
    out = {f"{tag}_samples": N, f"{tag}_ar_steps": AR, f"{tag}_grid": f"{nlon}x{nlat}", f"{tag}_channels": C,
           f"{tag}_rmse": round(run.overall[0].rmse, 6)}
    if with_oi:
        out["b_oi_stations"] = int(len(stations))
    for bs in (1, 8):
        out[f"{tag}_bs{bs}_samples_per_s"] = [round(v, 1) for v in rates[bs]]
    return out


def region_bytes(cell, nlat, N, P, C, nr, n_feat, store):
    """Bytes the regional scoring needs: the distinct global rows under the regional cells (P * C floats each, per
    sample), the distinct steps of the fp16 series that consecutive samples share (N + P of them), the stored fields."""
    n00 = cell[:, 0].astype(np.int64) * nlat + cell[:, 1]
    rows = np.unique(np.concatenate([n00, n00 + 1, n00 + nlat, n00 + nlat + 1])).size
    return N * rows * P * C * 4 + (N + P) * nr * n_feat * 2 + (2 * N * P * nr * C * 4 if store else 0)


def part_c(args, dev):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd.verify import RegionBundleScores, regrid_tables

    N, P, C, NLG, NTG, NLR, NTR, NT = 200, 4, 19, 512, 256, 61, 41, 260
    cell, w = regrid_tables(np.linspace(-90, 90, NTG), np.linspace(0, 360, NLG, endpoint=False), np.linspace(50, 60, NTR),
                            np.linspace(85, 100, NLR))
    nr = cell.shape[0]
    g = torch.Generator(device=dev).manual_seed(2)
    pred = torch.randn(N, NLG * NTG, P * C, generator=g, device=dev)
    series = torch.randn(NT, nr, C, generator=g, device=dev).to(torch.float16)
    t0 = torch.arange(2, 2 + N, dtype=torch.int32, device=dev)
    mean = torch.zeros(C, dtype=torch.float64, device=dev)
    std = torch.ones(C, dtype=torch.float64, device=dev)
    cell_d, w_d = torch.from_numpy(cell).to(dev), torch.from_numpy(w).to(dev)
    sums = torch.empty(P, C, hip.REGION_NS, dtype=torch.float64, device=dev)
    vout = torch.empty(N, P, nr, C, device=dev)
    tout = torch.empty_like(vout)

    def timed(fn, steps=10, warmup=3):
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

    call = lambda v, t: hip.region_interp_scores(pred, NTG, cell_d, w_d, series, t0, 0, mean, std, P, C, sums, v, t)  # noqa: E731
    t_scores = timed(lambda: call(None, None))
    t_store = timed(lambda: call(vout, tout))
    t_h0 = time.perf_counter()
    res = RegionBundleScores(sums.cpu().numpy(), N, N, nr)
    o = res.overall
    for p in range(P):
        res.horizon(p)
        for c in range(C):
            res.channel(p, c)
    t_host = (time.perf_counter() - t_h0) * 1e3
    items = N * P * nr * C
    b_scores = region_bytes(cell, NTG, N, P, C, nr, C, store=False)
    b_store = region_bytes(cell, NTG, N, P, C, nr, C, store=True)
    return {"c_samples": N, "c_horizons": P, "c_channels": C, "c_global_grid": f"{NLG}x{NTG}", "c_region_grid": f"{NLR}x{NTR}",
            "c_values": items, "c_scores_ms": round(t_scores, 4), "c_scores_GBps": round(b_scores / (t_scores * 1e-3) / 1e9, 1),
            "c_scores_and_fields_ms": round(t_store, 4), "c_scores_and_fields_GBps": round(b_store / (t_store * 1e-3) / 1e9, 1),
            "c_host_pooling_ms": round(t_host, 2), "c_overall_rmse": round(o["rmse"], 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--parts", default="abc")
    args = ap.parse_args()
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "predict_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    res = {"tool": "predict_bench", "repeats": args.repeats}
    with torch.no_grad():
        if "a" in args.parts:
            res.update(part_ab(args, dev, with_oi=False))
        if "b" in args.parts:
            res.update(part_ab(args, dev, with_oi=True))
        if "c" in args.parts:
            res.update(part_c(args, dev))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
