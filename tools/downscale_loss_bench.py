"""Time of the downscaler's objective (csrc/downscale_loss.hip through `downscale.downscaler_loss`), forward and
backward, at (B, C, H, W) = (32, 19, 41, 61) - the default ROI on the 0.25 degree grid - with the mask of two static
channels, residual and both weights on (0.1 / 0.05), next to the same objective written as plain torch ops (the
expression of scripts/train_downscaler.py:189-246: about twenty elementwise ops, two rfft2 and autograd) on the same GPU.

    python tools/downscale_loss_bench.py [--reps R] [--warmup W] [--steps N]

Prints one JSON line.  A timed window is N steps (loss, then backward into `out`) between one pair of HIP events, the
host enqueueing as it would in training; the figure is the window over N, the median of R windows after W warm-up
steps, in two rounds that alternate the two versions: the spread between the rounds is the noise of the run.  Our
steps captured in a graph and replayed (`ours_graph_us`) leave the host out: what the device alone needs for them (a
failed capture is reported as not measured; the torch version is not captured).  If torch has no rfft2 on this device, that is said and both versions are
timed without the spectral term.  Before timing, the two versions' loss and gradient are compared.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, C, H, W, OBS, NS = 32, 19, 41, 61, 2, 2
STATIC = (7, 8)
SW, GW = 0.1, 0.05


def torch_objective(out, Y, X, mask, sw, gw):
    """The objective as torch ops: the yardstick."""
    import torch

    m = mask.view(1, -1, 1, 1)
    o = X[:, (OBS - 1) * C:OBS * C] + out
    loss = ((o - Y) ** 2 * m).mean()
    if sw > 0:
        p, t = torch.fft.rfft2(o * m, norm="ortho").abs(), torch.fft.rfft2(Y * m, norm="ortho").abs()
        loss = loss + sw * (p - t).abs().mean()
    if gw > 0:
        e = o - Y
        dy, dx = e[:, :, 1:] - e[:, :, :-1], e[:, :, :, 1:] - e[:, :, :, :-1]
        loss = loss + gw * ((dy ** 2 * m).mean() + (dx ** 2 * m).mean())
    return loss


def windows(step, reps, warmup, steps):
    """us per step: (median, min, max) over `reps` windows of `steps` eager steps between one pair of events."""
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
    """The same steps captured once and replayed; None (and the reason) when the capture fails."""
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
        return windows(graph.replay, reps, 2, 1), None
    except Exception as e:  # noqa: BLE001  (reported, never hidden)
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {str(e)[:200]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100, help="steps of one timed window")
    args = ap.parse_args()

    import torch

    from graphcast_lite_amd import downscale as D
    from graphcast_lite_amd import hip

    assert torch.cuda.is_available(), "downscale_loss_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(B, OBS * C + NS, H, W, generator=gen, device=dev)
    Y = torch.randn(B, C, H, W, generator=gen, device=dev)
    out = (0.3 * torch.randn(B, C, H, W, generator=gen, device=dev)).requires_grad_(True)
    mask = torch.ones(C, device=dev)
    mask[list(STATIC)] = 0.0
    sw = SW
    note = None
    try:
        torch.fft.rfft2(Y[:1, :1], norm="ortho")
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        sw, note = 0.0, f"torch has no rfft2 here ({type(e).__name__}): both versions timed without the spectral term"

    def ours():
        out.grad = None
        D.downscaler_loss(out, Y, X=X, obs_window=OBS, residual=True, channel_mask=mask, spectral_weight=sw,
                          gradient_weight=GW).backward()

    def yardstick():
        out.grad = None
        torch_objective(out, Y, X, mask, sw, GW).backward()

    ours()
    g_ours, l_ours = out.grad.clone(), D.downscaler_loss(out, Y, X=X, obs_window=OBS, residual=True, channel_mask=mask,
                                                         spectral_weight=sw, gradient_weight=GW).item()
    yardstick()
    g_ref, l_ref = out.grad.clone(), torch_objective(out, Y, X, mask, sw, GW).item()
    res = {"tool": "downscale_loss_bench", "device": torch.cuda.get_device_name(0), "shape": [B, C, H, W],
           "spectral_weight": sw, "gradient_weight": GW, "residual": True, "masked_channels": list(STATIC),
           "reps": args.reps, "warmup": args.warmup, "steps": args.steps, "note": note,
           "loss_ours": l_ours, "loss_torch": l_ref,
           "grad_max_abs_diff_over_max": float((g_ours - g_ref).abs().max() / g_ref.abs().max())}
    for rnd in range(2):
        for name, fn in (("ours", ours), ("torch", yardstick)):
            res[f"{name}_eager_us_med_min_max_r{rnd}"] = windows(fn, args.reps, args.warmup, args.steps)
    chain = min(args.steps, 20)
    us, why = graph_windows(ours, args.reps, args.warmup, chain)
    res["ours_graph_us_med_min_max"] = None if us is None else [round(v / chain, 2) for v in us]
    if why:
        res["ours_graph_not_measured"] = why
    print(json.dumps(res))


if __name__ == "__main__":
    main()
