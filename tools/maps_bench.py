"""Device-event timings of the per-grid-point error maps (graphcast_lite_amd.verify.MetricMaps, csrc/maps.hip).

Shape: 512 x 256 grid, 19 channels in physical units (de-normalised, unit-converted), batches of 8 samples, 1 and 4
lead times; all four sums, the three sums without ACC, and RMSE only.  Per configuration:
  accumulate   `gcl_maps_accumulate` alone (column statistics precomputed), median of per-launch device events, its
               algorithmic bytes (both sample tensors read once, the state read and written once), TB/s and the
               fraction of 8 TB/s
  colstats     `gcl_maps_colstats` alone (two launches), same bytes for the samples
  update       `MetricMaps.update` eager and `CapturedMetricMaps.update` replayed (the replay copies both inputs into
               the graph's buffers first, as capture.Captured does)
The inputs rotate over several buffers so that no launch finds its samples in the 256 MB last-level cache.  The state
does not rotate: one lead's 80 MB (20 MB with RMSE only) may partly survive in that cache from one launch to the next,
so the TB/s figure is algorithmic, an upper view of the HBM rate; device events around one launch also include the
launch gap - the kernel trace of the same tool gives the kernel time proper.
For context (part h): the reference's way at the same shape with leads = 1 - both tensors copied to the host and
stacked, then de-normalisation, unit conversion and the four statistics of every channel with torch on 16 CPU threads
(wall time).

    python tools/maps_bench.py [--steps K] [--warmup W] [--parts duh] [--leads 1,4] [--sums all,noacc,rmse]
                               [--out profiles/maps_bench.json]

Parts: d the two entry points alone, u `update` eager and replayed, h the host's way.  A counter run takes
`--parts d` with one lead count and one set of sums, so that every launch of a kernel it sees is the same work.

Prints one JSON line and writes it to --out.
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

NAMES = ["t2m", "10u", "10v", "msl", "tp", "z@500", "z@850", "t@500", "t@850", "q@500", "q@850", "u@500", "u@850",
         "v@500", "v@850", "sp", "tcc", "lsm", "orog"]
N_LON, N_LAT, B = 512, 256, 8
PEAK_TBPS = 8.0
SUMS = {"all": ("rmse", "mae", "bias", "acc"), "noacc": ("rmse", "mae", "bias"), "rmse": ("rmse",)}


def median_ms(fn, steps, warmup):
    """Median of per-call device-event times."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(warmup + i)
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def scalers(C):
    rng = np.random.RandomState(7)
    return (rng.randn(C) * 100.0).astype(np.float64), (0.5 + 10.0 * rng.rand(C)).astype(np.float64)


def device_config(args, dev, leads, stats):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd import verify as V

    G, C = N_LON * N_LAT, len(NAMES)
    K = leads * C
    y_mean, y_scale = scalers(C)
    nbuf = max(2, int(np.ceil(600e6 / (2 * B * G * K * 4))))
    g = torch.Generator(device=dev).manual_seed(leads)
    bufs = []
    for _ in range(nbuf):
        t = torch.randn(B, G, K, generator=g, device=dev)
        bufs.append((t, t + 0.3 * torch.randn(B, G, K, generator=g, device=dev)))
    kw = dict(leads=leads, stats=stats, var_order=NAMES, y_mean=y_mean, y_scale=y_scale)
    mm = V.MetricMaps(C, G, device=dev, **kw)
    mm.update(*bufs[0])
    cs = mm._scratch.get(B)
    sample_bytes = 2 * B * G * K * 4
    state_bytes = 2 * mm._state.numel() * 8

    def acc(i):
        t, p = bufs[i % nbuf]
        hip.maps_accumulate(t, p, None, None, mm._conv, mm._flags, cs, mm._sums, C, mm._state, mm._count)
    t_acc = median_ms(acc, args.steps, args.warmup)
    res = {"accumulate_ms": round(t_acc, 4), "accumulate_bytes": sample_bytes + state_bytes,
           "accumulate_TBps": round((sample_bytes + state_bytes) / (t_acc * 1e-3) / 1e12, 3)}
    res["accumulate_frac_of_8TBps"] = round(res["accumulate_TBps"] / PEAK_TBPS, 3)
    if cs is not None:
        def col(i):
            t, p = bufs[i % nbuf]
            hip.maps_colstats(t, p, None, None, mm._conv, mm._flags, cs)
        t_col = median_ms(col, args.steps, args.warmup)
        res.update(colstats_ms=round(t_col, 4), colstats_bytes=sample_bytes,
                   colstats_TBps=round(sample_bytes / (t_col * 1e-3) / 1e12, 3))
    if "u" in args.parts:
        res["update_eager_ms"] = round(median_ms(lambda i: mm.update(*bufs[i % nbuf]), args.steps, args.warmup), 4)
        cap = V.CapturedMetricMaps(C, G, device=dev, **kw)
        res["update_replayed_ms"] = round(median_ms(lambda i: cap.update(*bufs[i % nbuf]), args.steps,
                                                    max(args.warmup, 4)), 4)
        res["update_launch_mode"] = cap.launch_mode
    t0 = time.perf_counter()
    n = mm.n
    for s in stats:
        mm.maps(s)
    torch.cuda.synchronize()
    res["n_and_maps_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    res["n"] = n
    return res


def host_reference(args, dev):
    """The reference's path at leads = 1, written here for all channels at once: every sample copied to the host and
    stacked, de-normalised, converted channel by channel, then the four per-node statistics over the sample axis."""
    from graphcast_lite_amd import verify as V

    torch.set_num_threads(16)
    G, C = N_LON * N_LAT, len(NAMES)
    y_mean, y_scale = (torch.from_numpy(a).float() for a in scalers(C))
    units = [V.unit_label(name) for name in NAMES]
    factor = torch.tensor([u[1] for u in units], dtype=torch.float32)
    offset = torch.tensor([u[2] for u in units], dtype=torch.float32)
    geopotential = [c for c, u in enumerate(units) if u[3] == "z_to_m"]
    g = torch.Generator(device=dev).manual_seed(1)
    t = torch.randn(B, G, C, generator=g, device=dev)
    p = t + 0.3 * torch.randn(B, G, C, generator=g, device=dev)

    def physical(x):
        x = x * y_scale + y_mean
        x[..., geopotential] /= 9.80665
        return x * factor + offset

    def anomalies(x):  # every sample's field, centred and scaled by its own spread
        spread, centre = torch.std_mean(x, dim=1, keepdim=True)
        return (x - centre) / (spread + 1e-8)

    def run():
        fields = [torch.stack([x[b].cpu() for b in range(B)]) for x in (p, t)]
        t_copied = time.perf_counter()
        P, T = (physical(f) for f in fields)
        diff = P - T
        maps = {"rmse": diff.square().mean(0).sqrt(), "mae": diff.abs().mean(0), "bias": diff.mean(0),
                "acc": (anomalies(P) * anomalies(T)).mean(0)}
        assert all(m.shape == (G, C) for m in maps.values())
        return t_copied
    run()
    reps = max(1, args.steps // 10)
    copy_ms, total_ms = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t1 = run()
        t2 = time.perf_counter()
        copy_ms.append((t1 - t0) * 1e3)
        total_ms.append((t2 - t0) * 1e3)
    return {"host_copy_and_stack_ms": round(float(np.median(copy_ms)), 1),
            "host_total_ms": round(float(np.median(total_ms)), 1), "host_threads": torch.get_num_threads()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="duh")
    ap.add_argument("--leads", default="1,4", help="lead counts of parts d and u")
    ap.add_argument("--sums", default="all,noacc,rmse", help="sets of sums of parts d and u")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maps_bench.json"))
    args = ap.parse_args()
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "maps_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    res = {"tool": "maps_bench", "steps": args.steps, "warmup": args.warmup, "grid": f"{N_LON}x{N_LAT}",
           "channels": len(NAMES), "batch": B}
    with torch.no_grad():
        if "d" in args.parts or "u" in args.parts:
            for leads in (int(v) for v in args.leads.split(",")):
                for tag in args.sums.split(","):
                    res[f"leads{leads}_{tag}"] = device_config(args, dev, leads, SUMS[tag])
                    torch.cuda.empty_cache()
        if "h" in args.parts:
            res["host_reference_leads1"] = host_reference(args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
