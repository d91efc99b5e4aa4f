"""Time of the WeatherUNetV2 forward on the HIP path (`graphcast_lite_amd.unet_v2`, csrc/unet_v2.hip + csrc/unet.hip) at
the workload's shape - H x W = 41 x 61, 40 input channels, 19 output channels, base_filters 64, 4 heads, 4 modes - for B
in {1, 8}, next to torch's own float32 forward of the functional restatement (tests/helpers/unet_v2_case.py) of the same
state dict on the same GPU: what a user has without this path.

    python tools/bench_unet_v2.py [--reps R] [--warmup W] [--steps N] [--batches 1,8] [--out FILE]

Inputs and weights are synthetic (seeded).  Prints one JSON line (and writes it to --out).  Per batch size:
  hip_eager_us / hip_graph_us / torch_eager_us / torch_graph_us   one forward: a window of N forwards between one pair
      of HIP events over N, [median, min, max] of R windows after W warm-up forwards; `graph`: the forward captured in a
      hipGraph and replayed (the device alone); the versions alternate in two rounds (r0, r1): their spread is the noise;
  launches   per entry of `launch_plan` (one launch; `.tail` is two), replayed alone in a graph of N calls: us
      [median, min, max]; launches_sum_us is the sum of the medians, sum_us_<kind> the same per kind of launch;
  check      max |hip - torch| / max |torch| of the two outputs, before any timing.
Every step runs under the caller's time limit; one process."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, IN, OUT, BASE, HEADS, MODES = 41, 61, 40, 19, 64, 4, 4
KINDS = ("conv.0", "conv.3", "gn1_stats", "gn2_stats", "gn1_gelu", "skip", "tail", "attn", "spectral", "out_conv")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="forwards (or launches) of one timed window")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import unet_v2_case as VC
    from bench_unet import graph_windows, windows

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    assert torch.cuda.is_available(), "bench_unet_v2 needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    model = VC.randomise_(WeatherUNetV2(IN, OUT, BASE, HEADS, MODES), 0).eval().to(dev)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    res = {"tool": "bench_unet_v2", "device": torch.cuda.get_device_name(0), "shape": [IN, OUT, BASE, HEADS, MODES, H, W],
           "reps": args.reps, "warmup": args.warmup, "steps": args.steps, "params": model.num_params,
           "launches_per_forward": model.LAUNCHES}

    def write():
        if args.out:  # (after every batch size: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    for B in [int(b) for b in args.batches.split(",")]:
        x = torch.randn(B, IN, H, W, generator=torch.Generator(device=dev).manual_seed(B), device=dev)
        with torch.no_grad():
            y_hip, y_ref = model(x), VC.functional_unet_v2(sd, x, HEADS, MODES)
        r = {"check_max_diff_over_max": float((y_hip - y_ref).abs().max() / y_ref.abs().max())}

        def ours():
            return model(x)

        def yardstick():
            with torch.no_grad():
                return VC.functional_unet_v2(sd, x, HEADS, MODES)

        for rnd in range(2):
            for name, fn in (("hip", ours), ("torch", yardstick)):
                r[f"{name}_eager_us_r{rnd}"] = windows(fn, args.reps, args.warmup, args.steps)
            for name, fn in (("hip", ours), ("torch", yardstick)):
                us, why = graph_windows(fn, args.reps, args.warmup, min(args.steps, 10))
                r[f"{name}_graph_us_r{rnd}"] = us
                if why:
                    r[f"{name}_graph_not_measured"] = why
        y = torch.empty(B, OUT, H, W, device=dev)
        rows = []
        for name, launch in model.launch_plan(x, y):
            us, why = graph_windows(launch, args.reps, args.warmup, args.steps)
            row = {"name": name, "us": us}
            if us is None:
                row["not_measured"] = why
            rows.append(row)
        r["launches"] = rows
        r["launches_sum_us"] = round(sum(l["us"][0] for l in rows if l["us"]), 2)
        for kind in KINDS:
            sel = [l["us"][0] for l in rows if l["us"] and (l["name"].endswith("." + kind) or l["name"].startswith(kind))]
            r[f"sum_us_{kind}"] = round(sum(sel), 2)
        res[f"B{B}"] = r
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
