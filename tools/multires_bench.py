"""ms per `MultiresChunkDataset.batch` at the real size (512 x 256 global, 61 x 41 regional box 50-60N x 83-98E,
19 features, obs 2 + pred 1, B = 8) in merge and in interpolate mode, next to the yardstick: `gcl_window_pack` on a
pre-merged flat series of the same N_total (what a user has after running the reference's builder), and to the same
kernel on the regular global grid.  Synthetic series, written to a temporary directory and uploaded once.

    python tools/multires_bench.py [--reps R] [--warmup W] [--frames T]

Prints one JSON line.  Timing: HIP events around every launch, the median of R launches after W warm-up launches; every
launch reads windows that no recent launch touched (the starts rotate through the series) into one of two output
buffers, so the 256 MiB Infinity Cache does not serve the reads.  Bytes: the algorithm's fp16 frames in (2 bytes per
value of each of the obs + pred frames) plus the fp32 windows out.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROI = (50.0, 60.0, 83.0, 98.0)
C, OBS, PRED, B = 19, 2, 1, 8


def write_dataset(path, T, lats, lons, rng):
    os.makedirs(path)
    n = T * len(lons) * len(lats) * C
    mm = np.memmap(os.path.join(path, "data.npy"), dtype=np.float16, mode="w+", shape=(n,))
    for a in range(0, n, 1 << 24):
        mm[a:a + (1 << 24)] = rng.standard_normal(min(1 << 24, n - a), dtype=np.float32).astype(np.float16)
    mm.flush()
    del mm
    with open(os.path.join(path, "dataset_info.json"), "w") as fh:
        json.dump({"time_start": "", "time_end": "", "n_time": T, "n_lon": len(lons), "n_lat": len(lats), "n_feat": C}, fh)
    np.savez(os.path.join(path, "coords.npz"), latitude=lats, longitude=lons)
    np.savez(os.path.join(path, "scalers.npz"), mean=np.zeros(C, np.float32), std=np.ones(C, np.float32))
    with open(os.path.join(path, "variables.json"), "w") as fh:
        json.dump([f"v{c}" for c in range(C)], fh)
    return path


def timed(fn, reps, warmup):
    """Median and spread (ms) of single launches: fn(k) enqueues launch k."""
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k, (a, b) in enumerate(ev):
        a.record()
        fn(warmup + k)
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return statistics.median(ms), ms[0], ms[-1]


def copy_ceiling_gbs(dev):
    """The stream-copy ceiling of this box as bench.py measures it: a 256 MiB device-to-device copy, read + write."""
    a = torch.empty(64 << 20, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    return 2.0 * a.numel() * 4 * 10 / (e0.elapsed_time(e1) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--frames", type=int, default=96)
    args = ap.parse_args()

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.multires import MultiresChunkDataset

    assert torch.cuda.is_available(), "multires_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    T = args.frames
    g_lats, g_lons = np.linspace(-90, 90, 256), np.linspace(0, 360, 512, endpoint=False)
    r_lats, r_lons = ROI[0] + 0.25 * np.arange(41), ROI[2] + 0.25 * np.arange(61)
    rng = np.random.default_rng(0)
    span = B * (OBS + PRED)
    groups = (T - (OBS + PRED)) // span + 1  # disjoint groups of B windows
    assert groups >= 3, "--frames too small to rotate the windows"
    with tempfile.TemporaryDirectory() as d:
        gdir = write_dataset(os.path.join(d, "global"), T, g_lats, g_lons, rng)
        rdir = write_dataset(os.path.join(d, "region"), T, r_lats, r_lons, rng)
        kw = dict(obs_window=OBS, pred_steps=PRED, split="all", device=dev)
        merge = MultiresChunkDataset(gdir, rdir, ROI, mode="merge", **kw)
        interp = MultiresChunkDataset(gdir, os.path.join(rdir, "coords.npz"), ROI, mode="interpolate", **kw)
    N = merge.n_nodes
    # the yardstick's input: the merged series as the reference's builder would have stored it, (T, N, C) fp16
    flat = torch.empty(T, N, C, dtype=torch.float16, device=dev)
    for t in range(0, T, 8):
        t0 = torch.arange(t, min(t + 8, T), dtype=torch.int64, device=dev)
        merge.windows(t0, 1, 0, C, zscore=False, out=(flat[t:t + t0.numel()], None), out_f16=True)
    starts = [torch.arange(0, span, OBS + PRED, dtype=torch.int64, device=dev) + g * span for g in range(groups)]

    def buffers(G):
        return [(torch.empty(B, G, OBS * C, device=dev), torch.empty(B, G, PRED * C, device=dev)) for _ in range(2)]

    bufs_n, bufs_g = buffers(N), buffers(512 * 256)
    runs = {
        "merge": lambda k: merge.windows(starts[k % groups], OBS, PRED, C, out=bufs_n[k % 2]),
        "interpolate": lambda k: interp.windows(starts[k % groups], OBS, PRED, C, out=bufs_n[k % 2]),
        "window_pack_flat": lambda k: hip.window_pack(flat, starts[k % groups], merge.mean, merge.std, C, OBS, PRED,
                                                      out=bufs_n[k % 2]),
        "window_pack_grid": lambda k: hip.window_pack(merge.series, starts[k % groups], merge.mean, merge.std, C, OBS,
                                                      PRED, out=bufs_g[k % 2]),
    }
    # the same windows from the three paths that serve the flat node set
    ref = hip.window_pack(flat, starts[1], merge.mean, merge.std, C, OBS, PRED)
    got = merge.windows(starts[1], OBS, PRED, C)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])

    res = {"tool": "multires_bench", "device": torch.cuda.get_device_name(0), "global": "512x256", "regional": "61x41",
           "features": C, "obs": OBS, "pred": PRED, "batch": B, "frames": T, "nodes": N,
           "n_global_kept": merge.n_global_kept, "n_regional": merge.n_regional, "reps": args.reps,
           "warmup": args.warmup}
    for rnd in range(2):  # two alternating rounds: the spread between them is the noise of the box
        for name, fn in runs.items():
            G = 512 * 256 if name == "window_pack_grid" else N
            nbytes = B * (OBS + PRED) * G * C * (2 + 4)
            med, lo, hi = timed(fn, args.reps, args.warmup)
            res[f"{name}_ms_r{rnd}"] = med
            res[f"{name}_min_max_ms_r{rnd}"] = [round(lo, 4), round(hi, 4)]
            res[f"{name}_gbps_r{rnd}"] = nbytes / med / 1e6
            res[f"{name}_bytes"] = nbytes
    res["copy_ceiling_gbs"] = copy_ceiling_gbs(dev)
    for name in runs:
        res[f"{name}_frac_of_copy_ceiling"] = max(res[f"{name}_gbps_r0"], res[f"{name}_gbps_r1"]) / res["copy_ceiling_gbs"]
    for name in ("merge", "interpolate"):
        res[f"{name}_over_flat"] = min(res[f"{name}_ms_r0"], res[f"{name}_ms_r1"]) / min(
            res["window_pack_flat_ms_r0"], res["window_pack_flat_ms_r1"])
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
