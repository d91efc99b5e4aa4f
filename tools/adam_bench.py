"""Adam update timing over the flat parameter buckets of real models (graphcast_lite_amd.train.FusedAdam).

    python tools/adam_bench.py [--iters 30] [--reps 20] [--out profiles/adam_bench.json]

Prints one JSON line.  Buckets: `baseline`, `wb2_512x256_19f_ar_v2` (one group, every parameter trainable) and the
same InteractionNet-256 x 12 model as `experiments/multires_nores_freeze6` trains it: two groups (processor at
lr x 0.1), processor frozen and unfrozen.  Per bucket and entry point (`gcl_adam_step_groups`, `gcl_adam_step`, and
`gcl_adam_step_dev` while the library still exports it): the device-event median of one update (`reps` back-to-back
updates between two events, `iters` samples) and the algorithmic bytes, 28 B per active bucket element (p, g, m, v
read; p, m, v written).  Parameter shapes do not depend on the grid, so the models are built on a small one.
Per-kernel medians come from a `rocprofv3 --kernel-trace --stats` run of this tool (profiles/adam_kernel_stats.csv).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_device(fn, iters, reps):
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    return float(np.median(ts))


def model(name, dev):
    import torch

    from graphcast_lite_amd.experiments import experiment
    from graphcast_lite_amd.models import WeatherPrediction

    cfg = experiment(name, [1, 2])
    torch.manual_seed(0)
    lats, lons = np.linspace(-90, 90, 32, endpoint=True), np.linspace(0, 360, 64, endpoint=False)
    return WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev)


def two_groups(m, lr=1e-4, factor=0.1):
    proc = list(m.processor.parameters())
    ids = {id(p) for p in proc}
    return [{"params": [p for p in m.parameters() if id(p) not in ids], "lr": lr}, {"params": proc, "lr": lr * factor}]


def bench_bucket(opt, iters, reps):
    import torch

    from graphcast_lite_amd import hip

    flat = opt.flat
    flat.grad.copy_(1e-3 * torch.randn_like(flat.grad))
    opt.sync()
    active = sum((p.numel() + 63) // 64 * 64 for p in flat.params if p.requires_grad)
    b1, b2 = opt.betas
    out = {"bucket_elems": flat.numel, "params": len(flat.params), "active_elems": active,
           "algorithmic_bytes": 28 * active}

    def grouped():
        hip.adam_step_groups(flat.flat, flat.grad, opt.m, opt.v, flat.chunk_param, opt.active_dev, opt.lr_dev,
                             opt.step_dev, opt.bc_dev, b1, b2, opt.eps, opt.wd)

    def one_counter():
        hip.adam_step(flat.flat, flat.grad, opt.m, opt.v, opt.lr, b1, b2, opt.eps, opt.wd, 10)

    out["groups_ms"] = time_device(grouped, iters, reps)
    out["groups_tbs"] = out["algorithmic_bytes"] / out["groups_ms"] / 1e9
    if active == flat.numel:  # the single-counter kernels update every element: compared on whole buckets only
        out["adam_step_ms"] = time_device(one_counter, iters, reps)
        if hasattr(hip, "adam_step_dev") and hasattr(hip.lib(), "gcl_adam_step_dev"):
            step_dev = torch.zeros(1, dtype=torch.int32, device=flat.flat.device)
            bc_dev = torch.zeros(2, dtype=torch.float32, device=flat.flat.device)

            def dev_counter():
                hip.adam_step_dev(flat.flat, flat.grad, opt.m, opt.v, opt.lr, b1, b2, opt.eps, opt.wd, step_dev, bc_dev)

            out["adam_step_dev_ms"] = time_device(dev_counter, iters, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.train import FlatParams, FusedAdam

    dev = torch.device("cuda:0")
    hip.lib()
    res = {}
    for name in ("baseline", "wb2_512x256_19f_ar_v2"):
        m = model(name, dev)
        res[name] = bench_bucket(FusedAdam(FlatParams(m), lr=1e-4), args.iters, args.reps)
    m = model("wb2_512x256_19f_ar_v2", dev)
    groups = two_groups(m)
    for p in m.processor.parameters():
        p.requires_grad = False
    opt = FusedAdam(FlatParams(m, groups), param_groups=groups)
    res["freeze6_frozen"] = bench_bucket(opt, args.iters, args.reps)
    for p in m.processor.parameters():
        p.requires_grad = True
    res["freeze6_unfrozen"] = bench_bucket(opt, args.iters, args.reps)
    line = {"metric": "Adam update over the flat bucket, device-event median per update", "unit": "ms",
            "reps_per_sample": args.reps, "samples": args.iters, "buckets": res,
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
