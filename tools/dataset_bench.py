"""Time of the dataset kernels (csrc/dataset.hip) at the real block size: 512 x 256 points, 19 channels, 500 time steps
(one `time_chunk` of the reference's builder), sources and series resident on the GPU.

    python tools/dataset_bench.py [--reps R] [--warmup W] [--steps NT] [--numpy-steps N]

Prints one JSON line.  Timing: HIP events around every call, the median of R calls after W warm-up calls; a call moves
gigabytes, far beyond the 256 MiB Infinity Cache, and alternates between two destination series.  Bytes are the
algorithm's: float32 planes in, fp16 rows out (pack: 4 + 2 bytes per value; sums only: 4; stats: 2; widen: 2 in and
2 * 23 / 19 out).  The yardsticks: the box's stream-copy ceiling as bench.py measures it, and `gcl_window_pack` on the
same series.  For the record, the reference's numpy path (a strided 2-byte write per channel into a memmap, two passes
for the sums) for a block of --numpy-steps steps on this machine's CPUs.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_LON, N_LAT, C = 512, 256, 19
P = N_LON * N_LAT
PEAK_GBS = 8000.0  # HBM3E peak of one MI355X


def timed(fn, reps, warmup):
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


def numpy_block(nt, rng):
    """The reference's host path for one block of nt steps: per channel scale, cast, strided memmap write, two sums."""
    planes = [rng.standard_normal((nt, N_LON, N_LAT), dtype=np.float32) for _ in range(C)]
    with tempfile.TemporaryDirectory() as d:
        fp = np.memmap(os.path.join(d, "data.npy"), dtype=np.float16, mode="w+", shape=(nt, N_LON, N_LAT, C))
        s, q = np.zeros(C), np.zeros(C)
        t0 = time.perf_counter()
        for j, arr in enumerate(planes):
            if j % 4 == 3:
                arr = arr * 0.01
            fp[:, :, :, j] = arr.astype(np.float16)
            s[j] = arr.sum(dtype=np.float64)
            q[j] = (arr * arr).sum(dtype=np.float64)
        fp.flush()
        build_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        for j in range(C):  # the statistics pass over the memmap (resume, repair, add_time_features)
            arr = np.nan_to_num(fp[:, :, :, j].astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
            s[j] = arr.sum(dtype=np.float64)
            q[j] = (arr * arr).sum(dtype=np.float64)
        stats_s = time.perf_counter() - t0
        del fp
    return build_s, stats_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--numpy-steps", type=int, default=100)
    args = ap.parse_args()

    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "dataset_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    nt = args.steps
    gen = torch.Generator(device=dev).manual_seed(0)
    planes = [torch.randn(nt, P, generator=gen, device=dev) * (1 + j) for j in range(C)]
    scales = [0.01 if j % 4 == 3 else 1.0 for j in range(C)]
    series = [torch.empty(nt, N_LON, N_LAT, C, dtype=torch.float16, device=dev) for _ in range(2)]
    wide = torch.empty(nt, N_LON, N_LAT, C + 4, dtype=torch.float16, device=dev)
    extra = torch.randn(nt, 4, generator=gen, device=dev).half()
    s, q = (torch.zeros(C, dtype=torch.float64, device=dev) for _ in range(2))
    mean, m2 = (torch.zeros(C, dtype=torch.float64, device=dev) for _ in range(2))
    n = torch.zeros(1, dtype=torch.int64, device=dev)
    chans = list(range(C))
    stat_out = hip.dataset_stats(series[0], 0, 1)
    B, OBS, PRED = 8, 2, 1
    t0s = [torch.arange(0, B * 3, 3, dtype=torch.int64, device=dev) + g * B * 3 for g in range((nt - 3) // (B * 3))]
    zmean, zstd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    wbuf = [(torch.empty(B, P, OBS * C, device=dev), torch.empty(B, P, PRED * C, device=dev)) for _ in range(2)]

    vals = nt * P * C
    runs = {
        "pack": (lambda k: hip.dataset_pack(planes, chans, scales, nt, series[k % 2], 0, s, q), vals * 6),
        "pack_sums_only": (lambda k: hip.dataset_pack(planes, chans, scales, nt, None, 0, s, q, grid=(N_LON, N_LAT, C)),
                           vals * 4),
        "pack_3_channels": (lambda k: hip.dataset_pack(planes[:3], [3, 5, 7], [0.01, 0.01, 0.1], nt, series[k % 2], 0, s, q),
                            nt * P * 3 * 6),
        "stats": (lambda k: hip.dataset_stats(series[k % 2], 0, nt, 3, out=stat_out), vals * 2),
        "widen": (lambda k: hip.dataset_widen(series[k % 2], extra, out=wide), vals * 2 + nt * P * (C + 4) * 2),
        "welford": (lambda k: hip.dataset_welford(mean, m2, n, s, q, nt * P), 0),
        "window_pack": (lambda k: hip.window_pack(series[0], t0s[k % len(t0s)], zmean, zstd, C, OBS, PRED, out=wbuf[k % 2]),
                        B * (OBS + PRED) * P * C * 6),
    }
    res = {"tool": "dataset_bench", "device": torch.cuda.get_device_name(0), "grid": f"{N_LON}x{N_LAT}", "channels": C,
           "steps": nt, "reps": args.reps, "warmup": args.warmup, "peak_gbs": PEAK_GBS}
    for rnd in range(2):  # two alternating rounds: the spread between them is the noise of the box
        for name, (fn, nbytes) in runs.items():
            med, lo, hi = timed(fn, args.reps, args.warmup)
            res[f"{name}_us_r{rnd}"] = med * 1e3
            res[f"{name}_min_max_us_r{rnd}"] = [round(lo * 1e3, 1), round(hi * 1e3, 1)]
            if nbytes:
                res[f"{name}_bytes"] = nbytes
                res[f"{name}_tbs_r{rnd}"] = nbytes / med / 1e9
    res["copy_ceiling_gbs"] = copy_ceiling_gbs(dev)
    for name, (_, nbytes) in runs.items():
        if nbytes:
            best = max(res[f"{name}_tbs_r0"], res[f"{name}_tbs_r1"])
            res[f"{name}_share_of_peak"] = best * 1e3 / PEAK_GBS
            res[f"{name}_frac_of_copy_ceiling"] = best * 1e3 / res["copy_ceiling_gbs"]
    # what a build from host arrays pays instead: the upload of one block's float32 planes (pageable memory)
    host = torch.randn(min(nt, 50), P).numpy()
    t0 = time.perf_counter()
    for _ in range(3):
        torch.from_numpy(host).to(dev)
    torch.cuda.synchronize()
    res["upload_gbs_pageable"] = 3 * host.nbytes / (time.perf_counter() - t0) / 1e9
    if args.numpy_steps > 0:
        torch.set_num_threads(16)
        b, st = numpy_block(args.numpy_steps, np.random.default_rng(0))
        res["numpy_steps"] = args.numpy_steps
        res["numpy_build_block_s"], res["numpy_stats_block_s"] = b, st
        res["numpy_build_s_per_500_steps"] = b * 500 / args.numpy_steps
        res["numpy_stats_s_per_500_steps"] = st * 500 / args.numpy_steps
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
