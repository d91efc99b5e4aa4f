"""The two measurements of DESIGN.md 3.23, on one GPU, `baseline` configuration (64x32 grid, 33 features, B = 64).

    python tools/runner_bench.py [--batches 8] [--passes 7] [--samples 4096] [--epochs 10]

1. Validation pass over 8 HBM-resident batches: `train.Evaluator.evaluate` (fused, captured) against `train.test`
   (torch ops, `.item()` per score, a Python loop over the samples), same process, same batches, one pair of HIP events
   around a pass, median of the passes after two warm-up passes, two rounds that alternate the two (the better round
   is reported, both are kept).  Per batch, for each: the GPU kernels a profiler trace counts (the evaluator in eager
   mode: the graph replays the same kernels for one host launch) and the host synchronisations torch's sync debug mode
   reports.
2. Loader-inclusive epoch: `TrainStep` fed by `DeviceLoader(buffers=step.input_buffers)` over a synthetic legacy dataset
   of 4096 samples resident in HBM, shuffled; samples/s over whole epochs, next to the same step on one resident batch
   (what `bench.py` times).

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def count_syncs(fn):
    import torch

    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in seen)


def count_kernels(fn):
    """GPU kernels of one call, from a profiler trace; None when the profiler gives none on this build."""
    import torch

    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as e:  # noqa: BLE001
        print(f"profiler unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def pass_ms(fn, passes, warmup=2):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()

    import numpy as np
    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.data import DeviceLoader, WeatherDataset
    from graphcast_lite_amd.experiments import GRID, experiment
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.train import Evaluator, TrainStep, get_lat_weights, test

    dev = torch.device("cuda:0")
    torch.cuda.set_stream(torch.cuda.Stream(dev))  # as bench.py: replayed graphs on a created stream
    hip.lib()
    cfg = experiment("baseline")
    nlat, nlon = GRID["baseline"]
    torch.manual_seed(42)
    model = WeatherPrediction((np.linspace(-90, 90, nlat), np.linspace(0, 360, nlon, endpoint=False)), cfg.graph,
                              cfg.pipeline, cfg.data, dev)
    G, C, obs, B = model._num_grid_nodes, cfg.data.num_features_used, cfg.data.obs_window_used, a.batch
    lw = get_lat_weights(nlat, nlon, dev)
    out = {"config": "baseline", "B": B, "G": G, "C": C, "device": torch.cuda.get_device_name(0)}

    # ---- 1. validation pass -------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(a.batches):
        X = torch.randn(B, G, obs * C, generator=g)
        batches.append((X.to(dev), (X[..., -C:] + 0.1 * torch.randn(B, G, C, generator=g)).to(dev)))
    ev = Evaluator(model, lat_weights=lw)
    ev_eager = Evaluator(model, lat_weights=lw, use_graph=False)
    run_test = lambda: test(model, batches, None, dev, lw)  # noqa: E731
    run_ev = lambda: ev.evaluate(batches)  # noqa: E731
    want, got = run_test(), run_ev()
    out["scores_test"], out["scores_evaluator"] = list(want), list(got)
    one = batches[:1]
    val = {}
    paths = (("test", run_test, lambda: test(model, one, None, dev, lw)),
             ("evaluator", run_ev, lambda: ev_eager.update(*one[0])))
    rounds = {name: [] for name, _, _ in paths}
    for _ in range(2):  # two rounds that alternate the two: the spread between the rounds is the noise of the run
        for name, fn, _ in paths:
            rounds[name].append(pass_ms(fn, a.passes))
    for name, fn, single in paths:
        single()
        val[name] = {"ms_per_pass": min(r[0] for r in rounds[name]), "rounds_median_min_max": rounds[name],
                     "kernels_per_batch": count_kernels(single), "host_syncs_per_batch": count_syncs(single)}
    ev_eager.results()
    val["evaluator"]["launch_mode"] = ev.launch_mode
    val["evaluator"]["host_syncs_per_pass"] = count_syncs(run_ev)
    val["test"]["host_syncs_per_pass"] = count_syncs(run_test)
    val["speedup"] = val["test"]["ms_per_pass"] / val["evaluator"]["ms_per_pass"]
    out["validation"] = val

    # ---- 2. loader-inclusive epoch ------------------------------------------------------------------------------
    N = a.samples
    store_X = torch.randn(N, G, obs, C, device=dev)
    store_y = store_X[:, :, -1:, :] + 0.1 * torch.randn(N, G, 1, C, device=dev)
    ds = WeatherDataset(store_X, store_y.contiguous(), 0, N, obs, 1, C)
    step = TrainStep(model, lr=1e-3, lat_weights=lw)
    loader = DeviceLoader(ds, batch_size=B, shuffle=True, drop_last=True, buffers=step.input_buffers)

    def epoch():
        for i, (X, y) in enumerate(loader):
            step(X, y, 0.0, 0, i)

    epoch()  # warm-up: the capture, then batches written into the graph's buffers
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.epochs):
        epoch()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    nsteps = a.epochs * len(loader)
    X, y = ds.batch(list(range(B)))
    for _ in range(5):
        step(X, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(nsteps):
        step(X, y)
    torch.cuda.synchronize()
    dt_res = time.perf_counter() - t0
    out["epoch"] = {"samples": N, "steps": nsteps, "launch_mode": step.launch_mode,
                    "in_place": step.input_buffers() is not None,
                    "loader_samples_per_s": B * nsteps / dt, "resident_batch_samples_per_s": B * nsteps / dt_res,
                    "loader_cost_percent": 100.0 * (dt / dt_res - 1.0)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
