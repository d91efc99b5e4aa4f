"""Time of the downscaler kernels (csrc/downscale.hip) at the reference's shapes: a 512 x 256 x 19 global series cropped
onto the 61 x 41 regional grid of the box (50, 60, 83, 98), archives resident on the GPU.

    python tools/downscale_bench.py [--reps R] [--warmup W] [--chain N] [--frames T]
    python tools/downscale_bench.py --reference-script PATH/build_downscaler_dataset.py [--reference-frames N]

Prints one JSON line.  Timing: the calls are 17 - 70 us each, so a timed window is a train of N calls back to back
(captured in a graph once, replayed between one pair of HIP events: milliseconds of device work, no host in it) and the
figure is the window over N; the median of R trains after W warm-up calls, in two alternating rounds whose spread is the
noise of the run.  The median of R single calls between their own events is printed next to it (`*_single_us_*`): the
difference is what events and a lone launch add at this size.  Bytes are the algorithm's: output bytes plus the DISTINCT
source bytes a call needs (coarse: the cropped global nodes of every frame, not the whole frame; pred: the ROI nodes of
every sample; batch: obs + 1 fp16 frames in, float32 planes out; pair_mse: two fp16 frames per listed frame).  The
working sets here are tens of megabytes - inside the 256 MiB Infinity Cache - so the rates are cache-resident rates and
the yardstick printed next to them is a device copy of the same size, not the HBM peak.

The second form needs no GPU: it writes the same synthetic pair with N frames to a temporary directory, runs the given
builder script on it by runpy and prints its wall time, for the host comparison (scaled linearly to T by the reader).
"""
import argparse
import contextlib
import io
import json
import os
import runpy
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LON, N_LAT, C = 512, 256, 19
ROI = (50.0, 60.0, 83.0, 98.0)


def axes():
    g_lats, g_lons = np.linspace(-90, 90, N_LAT), np.linspace(0, 360, N_LON, endpoint=False)
    r_lats, r_lons = np.linspace(50.0, 60.0, 41), np.linspace(83.0, 98.0, 61)
    return g_lats, g_lons, r_lats, r_lons


def run_reference(script, frames):
    g_lats, g_lons, r_lats, r_lons = axes()
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as tmp:
        for name, lats, lons in (("global", g_lats, g_lons), ("region", r_lats, r_lons)):
            d = os.path.join(tmp, name)
            os.makedirs(d)
            rng.standard_normal((frames, len(lons), len(lats), C), dtype=np.float32).astype(np.float16).tofile(
                os.path.join(d, "data.npy"))
            with open(os.path.join(d, "dataset_info.json"), "w") as fh:
                json.dump({"n_time": frames, "n_lon": len(lons), "n_lat": len(lats), "n_feat": C}, fh)
            np.savez(os.path.join(d, "coords.npz"), latitude=lats, longitude=lons)
            np.savez(os.path.join(d, "scalers.npz"), mean=np.zeros(C, np.float32), std=np.ones(C, np.float32), n=np.int64(1))
            with open(os.path.join(d, "variables.json"), "w") as fh:
                json.dump([f"v{c}" for c in range(C)], fh)
        argv = sys.argv
        sys.argv = [script, "--global-dir", os.path.join(tmp, "global"), "--region-dir", os.path.join(tmp, "region"),
                    "--roi", *[str(v) for v in ROI], "--out-dir", os.path.join(tmp, "out")]
        try:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(script, run_name="__main__")
            wall = time.perf_counter() - t0
        finally:
            sys.argv = argv
    print(json.dumps({"tool": "downscale_bench", "mode": "reference builder on the host", "frames": frames,
                      "wall_s": round(wall, 3), "s_per_frame": round(wall / frames, 4)}))


def timed(fn, reps, warmup, chain):
    """us per call, twice: (median, min, max) over `reps` trains of `chain` calls each, captured in a graph once and
    replayed between one pair of events, and the median over `reps` single calls between their own events.  The first is
    the figure: a train runs for milliseconds, so neither the events nor the host's enqueue rate has a share in it.  The
    second shows what a lone launch of this size costs."""
    import torch

    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(chain):
            fn(k)
    graph.replay()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        graph.replay()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / chain for a, b in ev)
    for k, (a, b) in enumerate(ev):
        a.record()
        fn(k)
        b.record()
    torch.cuda.synchronize()
    single = statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)
    return statistics.median(us), us[0], us[-1], single


def copy_gbs(nbytes, dev):
    """A device copy moving `nbytes` in all (half read, half written): the yardstick of a working set of that size."""
    import torch

    a = torch.empty(max(nbytes // 2, 1 << 16), dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    med = timed(lambda k: b.copy_(a), 10, 3, 50)[0]
    return 2.0 * a.numel() / (med * 1e-6) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chain", type=int, default=200, help="calls of one timed train")
    ap.add_argument("--frames", type=int, default=512, help="frames of the global series and of the archives")
    ap.add_argument("--reference-script", default=None)
    ap.add_argument("--reference-frames", type=int, default=20)
    args = ap.parse_args()
    if args.reference_script:
        return run_reference(args.reference_script, args.reference_frames)

    import torch

    from graphcast_lite_amd import downscale as D
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "downscale_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    T, FPL, B_PRED, B_BATCH, OBS = args.frames, 256, 8, 32, 2
    g_lats, g_lons, r_lats, r_lons = axes()
    la0, la1, lo0, lo1 = D.roi_crop(g_lats, g_lons, ROI)
    P = len(r_lats) * len(r_lons)
    gen = torch.Generator(device=dev).manual_seed(0)
    series = torch.randn(T, N_LON, N_LAT, C, generator=gen, device=dev).half()
    pos, w = D.device_tables(*D.coarse_tables(g_lats, g_lons, r_lats, r_lons, ROI), dev)
    arch = [torch.empty(T, len(r_lons), len(r_lats), C, dtype=torch.float16, device=dev) for _ in range(2)]
    fine = torch.randn(T, len(r_lons), len(r_lats), C, generator=gen, device=dev).half()
    nt = min(FPL, T)

    lat_g, lon_g = np.meshgrid(g_lats, g_lons, indexing="ij")
    ppos, pw = D.prediction_tables(lat_g.ravel().astype(np.float32), lon_g.ravel().astype(np.float32), ROI, r_lats, r_lons,
                                   flat_grid=False)
    roi_nodes = len(np.unique(ppos))
    ppos, pw = D.device_tables(*D._lon_first(ppos, pw, len(r_lats), len(r_lons)), dev)
    pred = torch.randn(B_PRED, N_LON * N_LAT, C, generator=gen, device=dev)
    last = torch.randn(B_PRED, N_LON * N_LAT, OBS * C, generator=gen, device=dev)[:, :, C:]
    mean, std = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dests = [torch.arange(B_PRED, dtype=torch.int64, device=dev) + B_PRED * g for g in range(max(1, T // B_PRED))]

    ts = [torch.randint(OBS - 1, T, (B_BATCH,), generator=gen, device=dev) for _ in range(8)]
    static = torch.randn(len(r_lons), len(r_lats), 2, generator=gen, device=dev)
    outs = [(torch.empty(B_BATCH, OBS * C + 2, len(r_lats), len(r_lons), device=dev),
             torch.empty(B_BATCH, C, len(r_lats), len(r_lons), device=dev)) for _ in range(2)]
    flip = torch.randint(0, 2, (B_BATCH,), generator=gen, device=dev).int()
    neg = torch.zeros(C, dtype=torch.int32, device=dev)
    neg[1] = 1
    noise = torch.randn(B_BATCH, OBS * C, len(r_lats), len(r_lons), generator=gen, device=dev)
    all_t = torch.arange(T, dtype=torch.int64, device=dev)
    stats = torch.empty(C, 2, dtype=torch.float64, device=dev)

    frame = P * C * 2  # bytes of one fp16 frame of the fine grid
    crop = (la1 - la0) * (lo1 - lo0) * C * 2
    runs = {
        "coarse": (lambda k: hip.downscale_coarse(series, pos, w, 0, nt, arch[k % 2], 0), nt * (frame + crop)),
        "fine_copy": (lambda k: hip.downscale_coarse(fine, None, None, 0, nt, arch[k % 2], 0), nt * 2 * frame),
        "pred": (lambda k: hip.downscale_pred(pred, ppos, pw, std, mean, dests[k % len(dests)], arch[k % 2], last3=last),
                 B_PRED * (frame + roi_nodes * C * 4 * 2)),
        "batch": (lambda k: hip.downscale_batch(arch[0], fine, ts[k % 8], OBS, mean, std, static=static, out=outs[k % 2]),
                  B_BATCH * ((OBS + 1) * frame + (OBS * C + 2 + C) * P * 4) + P * 2 * 4),
        "batch_flip_noise": (lambda k: hip.downscale_batch(arch[0], fine, ts[k % 8], OBS, mean, std, static=static, flip=flip,
                                                           neg=neg, noise=noise, sigma=0.05, out=outs[k % 2]),
                             B_BATCH * ((OBS + 1) * frame + (OBS * C + 2 + C) * P * 4 + OBS * C * P * 4) + P * 2 * 4),
        "pair_mse": (lambda k: hip.downscale_pair_mse(arch[0], fine, all_t, mean, std, out=stats), T * 2 * frame),
    }
    arch[0].copy_(fine)
    res = {"tool": "downscale_bench", "device": torch.cuda.get_device_name(0), "global": f"{N_LON}x{N_LAT}x{C}",
           "fine": f"{len(r_lons)}x{len(r_lats)}", "crop": f"{lo1 - lo0}x{la1 - la0}", "frames": T,
           "frames_per_launch": nt, "pred_batch": B_PRED, "batch": B_BATCH, "obs": OBS, "reps": args.reps,
           "warmup": args.warmup, "chain": args.chain}
    for rnd in range(2):
        for name, (fn, nbytes) in runs.items():
            med, lo, hi, single = timed(fn, args.reps, args.warmup, args.chain)
            res[f"{name}_us_r{rnd}"] = med
            res[f"{name}_min_max_us_r{rnd}"] = [round(lo, 2), round(hi, 2)]
            res[f"{name}_single_us_r{rnd}"] = single
            res[f"{name}_bytes"] = nbytes
            res[f"{name}_gbs_r{rnd}"] = nbytes / med / 1e3
    for name, (_, nbytes) in runs.items():
        res[f"{name}_copy_same_size_gbs"] = copy_gbs(nbytes, dev)
    t0 = time.perf_counter()
    pairs_T = T
    for a in range(0, pairs_T, FPL):
        hip.downscale_coarse(series, pos, w, a, min(FPL, pairs_T - a), arch[0], a)
        hip.downscale_coarse(fine, None, None, a, min(FPL, pairs_T - a), arch[1], a)
    torch.cuda.synchronize()
    res["build_pairs_wall_s"] = time.perf_counter() - t0
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
