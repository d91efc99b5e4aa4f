"""Time of the WeatherUNet forward on the HIP path (`graphcast_lite_amd.unet`, csrc/unet.hip) at the workload's shape -
H x W = 41 x 61, 40 input channels, 19 output channels, base_filters 64 - for B in {1, 8, 32}, next to a float32
`torch.nn.functional` forward of the same state dict on the same GPU: what a user has without this path.

    python tools/bench_unet.py [--reps R] [--warmup W] [--steps N] [--batches 1,8,32] [--out FILE]

Inputs and weights are synthetic (seeded).  Prints one JSON line (and writes it to --out).  Per batch size:
  hip_eager_us / hip_graph_us / torch_eager_us / torch_graph_us   one forward: a window of N forwards between one pair
      of HIP events over N, [median, min, max] of R windows after W warm-up forwards; `graph`: the forward captured in a
      hipGraph and replayed (the device alone); the versions alternate in two rounds (r0, r1): their spread is the noise;
  layers   per launch, replayed alone in a graph of N launches: us, achieved GFLOP/s (2 * 9 * Cin * Cout * H * W * B over
      the time), and floor_share = the time of a launch that has next to nothing to do (the same kernel on one pixel and
      four channels) over the launch's time - 1.0 means the launch is bound by launching;
  check    max |hip - torch| / max |torch| of the two outputs, before any timing.
Every step runs under the caller's time limit; one process.

    python tools/bench_unet.py --train [--reps R] [--warmup W] [--steps N] [--batches 1,32] [--out FILE]

times one training step - the forward in training mode plus the backward of `unet.TrainableUNet` (csrc/unet_train.hip) -
at the same shape, next to the same step on torch's own convolutions (the functional network with `training=True` and
`torch.autograd.grad` for the 44 parameters).  Per batch size:
  hip_step_eager_us / hip_step_graph_us / torch_step_eager_us   one step, windows as above (the torch step eagerly only: its backward is not captured);
  launches   per entry-point call of the step (a call is one to three kernels), replayed alone in a graph of N calls:
      us and, for the convolutions, GFLOP/s; launches_sum_us is their sum;
  check      the largest max |hip - torch| / max |torch| over y and the 44 gradients, before any timing (torch-ROCm's own
      backward is the less accurate side of this figure: see --accuracy).

    python tools/bench_unet.py --accuracy [--batches 1,2] [--out FILE]

runs one training step at the same shape four ways - `TrainableUNet`, torch on the same GPU, torch float32 on the CPU,
torch float64 on the CPU - and reports E(t) = max |t - t64| / max |t64| of y and of each of the 44 gradients for the
first three against the fourth, with the ranges over the gradients."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, IN, OUT, BASE = 41, 61, 40, 19, 64
BLOCKS = ("inc.net", "down1.net.1.net", "down2.net.1.net", "down3.net.1.net", "up1.conv.net", "up2.conv.net", "up3.conv.net")


def randomise_(model, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif t.dim() == 1:
                t.copy_(0.75 + 0.5 * torch.rand(t.shape, generator=g) if name.endswith("weight")
                        else 0.2 * torch.randn(t.shape, generator=g))
            else:
                t.copy_(torch.randn(t.shape, generator=g) * (1.5 / (t.shape[1] * t.shape[2] * t.shape[3]) ** 0.5))
    return model


def torch_forward(sd, x):
    """model.py:87-98 as torch.nn.functional calls in float32: the yardstick."""
    import torch
    import torch.nn.functional as F

    def dc(p, x):
        for c, n in ((0, 1), (3, 4)):
            x = F.conv2d(x, sd[f"{p}.{c}.weight"], padding=1)
            x = F.gelu(F.batch_norm(x, sd[f"{p}.{n}.running_mean"], sd[f"{p}.{n}.running_var"], sd[f"{p}.{n}.weight"],
                                    sd[f"{p}.{n}.bias"], training=False, eps=1e-5))
        return x

    def up(p, x, skip):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = skip.shape[2] - x.shape[2], skip.shape[3] - x.shape[3]
        if dh > 0 or dw > 0:
            x = F.pad(x, [0, dw, 0, dh])
        return dc(p, torch.cat([skip, x], dim=1))

    x1 = dc(BLOCKS[0], x)
    x2 = dc(BLOCKS[1], F.max_pool2d(x1, 2))
    x3 = dc(BLOCKS[2], F.max_pool2d(x2, 2))
    x4 = dc(BLOCKS[3], F.max_pool2d(x3, 2))
    u = up(BLOCKS[6], up(BLOCKS[5], up(BLOCKS[4], x4, x3), x2), x1)
    return F.conv2d(u, sd["out_conv.weight"], sd["out_conv.bias"])


def torch_train_step(params, buffers, x, g):
    """The training forward (BatchNorm on batch statistics, the running buffers updated) and the 44 gradients."""
    import torch
    import torch.nn.functional as F

    def dc(p, x):
        for c, n in ((0, 1), (3, 4)):
            x = F.conv2d(x, params[f"{p}.{c}.weight"], padding=1)
            x = F.gelu(F.batch_norm(x, buffers[f"{p}.{n}.running_mean"], buffers[f"{p}.{n}.running_var"],
                                    params[f"{p}.{n}.weight"], params[f"{p}.{n}.bias"], training=True, momentum=0.1, eps=1e-5))
        return x

    def up(p, x, skip):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = skip.shape[2] - x.shape[2], skip.shape[3] - x.shape[3]
        if dh > 0 or dw > 0:
            x = F.pad(x, [0, dw, 0, dh])
        return dc(p, torch.cat([skip, x], dim=1))

    x1 = dc(BLOCKS[0], x)
    x2 = dc(BLOCKS[1], F.max_pool2d(x1, 2))
    x3 = dc(BLOCKS[2], F.max_pool2d(x2, 2))
    x4 = dc(BLOCKS[3], F.max_pool2d(x3, 2))
    u = up(BLOCKS[6], up(BLOCKS[5], up(BLOCKS[4], x4, x3), x2), x1)
    y = F.conv2d(u, params["out_conv.weight"], params["out_conv.bias"])
    return y, torch.autograd.grad(y, list(params.values()), g)


def windows(step, reps, warmup, steps):
    import torch

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        for _ in range(steps):
            step()
        b.record()
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 / steps for a, b in ev)
    return [round(statistics.median(us), 2), round(us[0], 2), round(us[-1], 2)]


def graph_windows(step, reps, warmup, steps):
    """`steps` calls captured once and replayed; us per call, or (None, reason) when the capture fails."""
    import torch

    try:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 3)):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(steps):
                step()
        return [round(v / steps, 2) for v in windows(graph.replay, reps, 2, 1)], None
    except Exception as e:  # noqa: BLE001  (reported, never hidden)
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {str(e)[:200]}"


def layer_shapes():
    """(name, Cin, Cout, H, W) of the 15 launches."""
    f = BASE
    lv = [(H, W)]
    for _ in range(3):
        lv.append((lv[-1][0] // 2, lv[-1][1] // 2))
    rows = [("inc.0", IN, f, 0), ("inc.3", f, f, 0), ("down1.0", f, 2 * f, 1), ("down1.3", 2 * f, 2 * f, 1),
            ("down2.0", 2 * f, 4 * f, 2), ("down2.3", 4 * f, 4 * f, 2), ("down3.0", 4 * f, 8 * f, 3),
            ("down3.3", 8 * f, 8 * f, 3), ("up1.0", 12 * f, 4 * f, 2), ("up1.3", 4 * f, 4 * f, 2),
            ("up2.0", 6 * f, 2 * f, 1), ("up2.3", 2 * f, 2 * f, 1), ("up3.0", 3 * f, f, 0), ("up3.3", f, f, 0)]
    return [(n, ci, co, *lv[k], 9) for n, ci, co, k in rows] + [("out_conv", f, OUT, H, W, 1)]


def train_main(args):
    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet import TrainableUNet

    assert torch.cuda.is_available(), "bench_unet needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    model = randomise_(TrainableUNet(IN, OUT, BASE), 0).to(dev).train()
    shapes = {n: (ci, co, h, w, t) for n, ci, co, h, w, t in layer_shapes()}
    res = {"tool": "bench_unet --train", "device": torch.cuda.get_device_name(0), "shape": [IN, OUT, BASE, H, W],
           "reps": args.reps, "warmup": args.warmup, "steps": args.steps, "params": model.num_params,
           "gflop_per_sample_fwd": round(sum(2 * t * ci * co * h * w for _, ci, co, h, w, t in layer_shapes()) / 1e9, 3)}

    def write():
        if args.out:  # (after every batch size: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    for B in [int(b) for b in args.batches.split(",")]:
        x = torch.randn(B, IN, H, W, generator=torch.Generator(device=dev).manual_seed(B), device=dev)
        g = torch.randn(B, OUT, H, W, generator=torch.Generator(device=dev).manual_seed(B + 100), device=dev)
        names = [n for n, _ in model.named_parameters()]
        tparams = {n: p.detach().clone().requires_grad_(True) for n, p in model.named_parameters()}
        tbufs = {n: b.detach().clone() for n, b in model.named_buffers() if b.is_floating_point()}
        y_ref, g_ref = torch_train_step(tparams, tbufs, x, g)
        model.zero_grad()
        y_hip = model(x)
        y_hip.backward(g)
        named = dict(model.named_parameters())
        worst = float((y_hip.detach() - y_ref.detach()).abs().max() / y_ref.detach().abs().max())
        for n, gr in zip(names, g_ref):
            worst = max(worst, float((named[n].grad - gr).abs().max() / gr.abs().max()))
        r = {"check_max_diff_over_max": worst}
        ws = model._train_workspace(B, H, W, dev)
        y = torch.empty(B, OUT, H, W, device=dev)
        plan = model.train_launch_plan(x, y, ws) + model.backward_launch_plan(x, g, ws)

        def ours():
            for _, launch in plan:
                launch()

        def yardstick():
            return torch_train_step(tparams, tbufs, x, g)

        for rnd in range(2):
            for name, fn in (("hip", ours), ("torch", yardstick)):
                r[f"{name}_step_eager_us_r{rnd}"] = windows(fn, args.reps, args.warmup, args.steps)
        # (the torch step is timed eagerly only: this tool does not capture autograd's backward in a hipGraph)
        us, why = graph_windows(ours, args.reps, args.warmup, min(args.steps, 5))
        r["hip_step_graph_us"] = us
        if why:
            r["hip_step_graph_not_measured"] = why
        ours()  # (a failed capture may have left the workspace half written)
        rows = []
        for name, launch in plan:
            us, why = graph_windows(launch, args.reps, args.warmup, args.steps)
            row = {"name": name, "us": us}
            base = name.split(".bn_")[0].rsplit(".wgrad", 1)[0].rsplit(".dgrad", 1)[0]
            if us is not None and base in shapes and (name == base or name.endswith((".wgrad", ".dgrad"))):
                ci, co, h, w, t = shapes[base]
                row["gflops"] = round(2 * t * ci * co * h * w * B / us[0] / 1e3, 1)
            if us is None:
                row["not_measured"] = why
            rows.append(row)
        r["launches"] = rows
        r["launches_sum_us"] = round(sum(l["us"][0] for l in rows if l["us"]), 2)
        for kind in ("fwd", "bn_stats", "bn_gelu", "bn_gelu_bwd", "wgrad", "dgrad", "upsample_bwd", "pool_bwd", "out"):
            sel = [l["us"][0] for l in rows if l["us"] and (
                l["name"].endswith("." + kind) or (kind == "fwd" and l["name"] in shapes and l["name"] != "out_conv")
                or (kind == "out" and l["name"].startswith("out_conv")))]
            r[f"sum_us_{kind}"] = round(sum(sel), 2)
        res[f"B{B}"] = r
        write()
    print(json.dumps(res))


def accuracy_main(args):
    """One training step at the workload's shape against the same step in float64 on the CPU."""
    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet import TrainableUNet

    assert torch.cuda.is_available(), "bench_unet needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")

    def E(t, t64):
        t, t64 = t.detach().double().cpu(), t64.detach().double().cpu()
        return float((t - t64).abs().max() / t64.abs().max())

    res = {"tool": "bench_unet --accuracy", "device": torch.cuda.get_device_name(0), "shape": [IN, OUT, BASE, H, W],
           "rule": "E(t) = max |t - t64| / max |t64| per tensor, t64: the float64 step on the CPU"}
    for B in [int(b) for b in args.batches.split(",")]:
        model = randomise_(TrainableUNet(IN, OUT, BASE), 0)
        names = [n for n, _ in model.named_parameters()]
        gen = torch.Generator().manual_seed(B)
        x, g = torch.randn(B, IN, H, W, generator=gen), torch.randn(B, OUT, H, W, generator=gen)

        def step(dtype, device):
            params = {n: p.detach().to(device=device, dtype=dtype).clone().requires_grad_(True)
                      for n, p in model.named_parameters()}
            bufs = {n: b.detach().to(device=device, dtype=dtype).clone() for n, b in model.named_buffers()
                    if b.is_floating_point()}
            y, grads = torch_train_step(params, bufs, x.to(device=device, dtype=dtype), g.to(device=device, dtype=dtype))
            return [y] + list(grads)

        t64, t32, tgpu = step(torch.float64, "cpu"), step(torch.float32, "cpu"), step(torch.float32, dev)
        model = model.to(dev).train()
        y = model(x.to(dev))
        y.backward(g.to(dev))
        ours = [y] + [p.grad for p in model.parameters()]
        rows = [{"tensor": n, "hip": E(a, r), "torch_gpu": E(b, r), "torch_cpu32": E(c, r)}
                for n, a, b, c, r in zip(["y"] + names, ours, tgpu, t32, t64)]
        grads = rows[1:]
        res[f"B{B}"] = {"tensors": rows,
                        "grad_hip": [min(r["hip"] for r in grads), max(r["hip"] for r in grads)],
                        "grad_torch_gpu": [min(r["torch_gpu"] for r in grads), max(r["torch_gpu"] for r in grads)],
                        "grad_torch_cpu32": [min(r["torch_cpu32"] for r in grads), max(r["torch_cpu32"] for r in grads)],
                        "grad_hip_over_cpu32_max": max(r["hip"] / max(r["torch_cpu32"], 1e-300) for r in grads)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true", help="time one training step (forward + backward) instead")
    ap.add_argument("--accuracy", action="store_true",
                    help="per-tensor error of one training step against the float64 step on the CPU instead")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20, help="forwards (or launches) of one timed window")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.accuracy:
        if args.batches == "1,8,32":
            args.batches = "1,2"
        return accuracy_main(args)
    if args.train:
        if args.batches == "1,8,32":
            args.batches = "1,32"
        return train_main(args)

    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet import WeatherUNet

    assert torch.cuda.is_available(), "bench_unet needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    model = randomise_(WeatherUNet(IN, OUT, BASE), 0).eval().to(dev)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    res = {"tool": "bench_unet", "device": torch.cuda.get_device_name(0), "shape": [IN, OUT, BASE, H, W],
           "reps": args.reps, "warmup": args.warmup, "steps": args.steps, "params": model.num_params,
           "gflop_per_sample": round(sum(2 * t * ci * co * h * w for _, ci, co, h, w, t in layer_shapes()) / 1e9, 3)}

    # the launch-bound floor: the conv kernel with next to nothing to do
    tiny_x = torch.zeros(1, 1, 1, 4, device=dev)
    tiny_y = torch.zeros(1, 1, 1, 4, device=dev)
    tiny_w = hip.unet_pack_weights(torch.zeros(4, 4, 3, 3, device=dev))
    tiny_src = hip.unet_src(hip.UNET_ROWS, tiny_x)
    floor, why = graph_windows(lambda: hip.unet_conv3x3(tiny_src, tiny_w, None, 1e-5, tiny_y, 4), args.reps, args.warmup, 50)
    res["launch_floor_us"] = floor
    if why:
        res["launch_floor_not_measured"] = why

    for B in [int(b) for b in args.batches.split(",")]:
        x = torch.randn(B, IN, H, W, generator=torch.Generator(device=dev).manual_seed(B), device=dev)
        with torch.no_grad():
            y_hip, y_ref = model(x), torch_forward(sd, x)
        r = {"check_max_diff_over_max": float((y_hip - y_ref).abs().max() / y_ref.abs().max())}

        def ours():
            return model(x)

        def yardstick():
            with torch.no_grad():
                return torch_forward(sd, x)

        for rnd in range(2):
            for name, fn in (("hip", ours), ("torch", yardstick)):
                r[f"{name}_eager_us_r{rnd}"] = windows(fn, args.reps, args.warmup, args.steps)
            for name, fn in (("hip", ours), ("torch", yardstick)):
                us, why = graph_windows(fn, args.reps, args.warmup, min(args.steps, 10))
                r[f"{name}_graph_us_r{rnd}"] = us
                if why:
                    r[f"{name}_graph_not_measured"] = why
        y = torch.empty(B, OUT, H, W, device=dev)
        layers = []
        for (name, launch), (_, ci, co, h, w, taps) in zip(model.launch_plan(x, y), layer_shapes()):
            us, why = graph_windows(launch, args.reps, args.warmup, args.steps)
            row = {"name": name, "Cin": ci, "Cout": co, "H": h, "W": w, "us": us}
            if us is not None:
                row["gflops"] = round(2 * taps * ci * co * h * w * B / us[0] / 1e3, 1)
                if floor is not None:
                    row["floor_share"] = round(floor[0] / us[0], 3)
            else:
                row["not_measured"] = why
            layers.append(row)
        r["layers"] = layers
        r["layers_sum_us"] = round(sum(l["us"][0] for l in layers if l["us"]), 2)
        res[f"B{B}"] = r
        if args.out:  # (after every batch size: a run that is cut short leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
