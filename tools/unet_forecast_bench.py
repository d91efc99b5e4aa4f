"""Samples per second of the regional U-Net forecaster's inference loop (`graphcast_lite_amd.unet_predict.GridForecaster`,
csrc/unet_forecast.hip) at the shapes of the reference's regional experiments, on synthetic data:

    v1   experiments/unet_region_krsk_23f:   H x W = 41 x 61, C = 23, obs 2, pred 4, base_filters 96, WeatherUNet
    v2   experiments/unet_v2_region_krsk:    H x W = 41 x 61, C = 23, obs 4, pred 4, base_filters 64, WeatherUNetV2 (4 heads, 4 modes)
    both: static channels [7, 8], forcing channels [19 .. 22], four autoregressive steps

    python tools/unet_forecast_bench.py [--samples N] [--reps R] [--archs v1,v2] [--out FILE]

Per architecture, four configurations, each timed as N samples between a device synchronise before and after (host clock),
R times, the configurations alternating inside a repetition; [median, min, max] samples/s:
  b8_graph, b1_graph   GridForecaster with batches of 8 / 1 replayed from a hipGraph;
  b8_eager             the same launches made eagerly;
  b8_torch_glue        the same network (the HIP module) and batch with the loop's glue written in plain torch device ops -
                       indexing the series, torch.cat for the shift, the per-channel sums - and no host round trip: what a
                       user could write around the module without the new kernels.  (The parent commit has no way to run
                       this loop at all; the reference's own loop goes through the host once per step and sample.)
`check` compares the accumulators of b8_graph and b8_torch_glue (largest relative difference of the squared-error sums).
`kernels`: gcl_grid_window_pack and gcl_grid_forecast_step alone at B = 8, replayed from a graph of 50 calls: us per call,
the bytes the call must move (computed from the shapes), that over the time, and the share of the 6.3 TB/s HBM rate - at
this size the tensors sit in the Infinity Cache and the calls are bound by their launches, which is what the figures show.
`network_us`: one forward at B = 8 replayed from a graph, for the share of a step the new kernels take.
Prints one JSON line (and writes it to --out).  One process; needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, C, PRED, AR = 41, 61, 23, 4, 4
STATIC, FORCING = [7, 8], [19, 20, 21, 22]
ARCHS = {"v1": dict(obs=2, base=96), "v2": dict(obs=4, base=64, heads=4, modes=4)}
HBM = 6.3e12  # bytes / s achievable (a float4 copy)
DEV = "cuda:0"


def make_model(arch, seed=0):
    import torch

    from graphcast_lite_amd.unet import WeatherUNet
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    a = ARCHS[arch]
    torch.manual_seed(seed)
    m = WeatherUNet(a["obs"] * C, C, a["base"]) if arch == "v1" else WeatherUNetV2(a["obs"] * C, C, a["base"], a["heads"], a["modes"])
    with torch.no_grad():
        m.out_conv.weight.mul_(0.1)  # a forecast near persistence: finite through four steps with untrained weights
    return m.to(DEV).eval()


def make_dataset(obs, n_samples, seed=1):
    import torch

    from graphcast_lite_amd.data import TimeseriesChunkDataset
    from graphcast_lite_amd.unet_predict import Grid2DDataset

    g = torch.Generator(device=DEV).manual_seed(seed)
    T = n_samples + obs + PRED - 1
    series = torch.randn(T, W, H, C, generator=g, device=DEV).to(torch.float16)
    mean = 0.1 * torch.randn(C, generator=g, device=DEV)
    std = 0.8 + 0.4 * torch.rand(C, generator=g, device=DEV)
    return Grid2DDataset(TimeseriesChunkDataset.from_series(series, mean, std, obs, PRED, split="all", n_features=C))


class TorchGlue:
    """The loop of GridForecaster with its glue in torch device ops (float64 sums, no host read until `state`)."""

    def __init__(self, model, ds, batch_size):
        import torch

        self.model, self.ds, self.B = model, ds, batch_size
        raw = ds.ds
        self.obs = raw.obs_window
        self.series, self.mean, self.std = raw.chunks[0], raw.mean.view(1, C, 1, 1), raw.std.view(1, C, 1, 1)
        self.state = torch.zeros(AR, C, 5, dtype=torch.float64, device=DEV)
        self.acc_count = torch.zeros(AR, C, dtype=torch.int64, device=DEV)
        self.frames = torch.arange(self.obs + PRED, device=DEV)

    def frame(self, window, k):  # [B, W, H, C] fp16 -> normalised planar [B, C, H, W]
        return (window[:, k].float().permute(0, 3, 2, 1) - self.mean) / self.std

    def update(self, indices):
        import torch

        t0 = torch.tensor([t for _, t in self.ds.window_starts(indices)], device=DEV)
        window = self.series[t0[:, None] + self.frames[None, :]][..., :C]
        cur = torch.cat([self.frame(window, k) for k in range(self.obs)], dim=1).contiguous()
        base = cur[:, (self.obs - 1) * C:]
        for s in range(AR):
            out = self.model(cur, residual_from=((self.obs - 1) * C, self.obs * C))
            g = self.frame(window, self.obs + s)
            out[:, STATIC] = cur[:, (self.obs - 1) * C:][:, STATIC]
            out[:, FORCING] = g[:, FORCING]
            pp, gp, bp = out * self.std + self.mean, g * self.std + self.mean, base * self.std + self.mean
            sums = [((pp - gp) ** 2), ((bp - gp) ** 2), ((out - g) ** 2), ((base - g) ** 2)]
            self.state[s, :, :4] += torch.stack([x.double().sum((0, 2, 3)) for x in sums], dim=1)
            p, t = out.double(), g.double()
            p, t = p - p.mean((2, 3), keepdim=True), t - t.mean((2, 3), keepdim=True)
            pn, tn = (p * p).sum((2, 3)).sqrt(), (t * t).sum((2, 3)).sqrt()
            ok = (pn > 1e-8) & (tn > 1e-8)
            corr = torch.where(ok, (p * t).sum((2, 3)) / (pn * tn), torch.zeros_like(pn))
            self.state[s, :, 4] += corr.sum(0)
            self.acc_count[s] += ok.sum(0)
            cur = torch.cat([cur[:, C:], out], dim=1)


def timed(run, n_samples):
    import torch

    torch.cuda.synchronize()
    t = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return n_samples / (time.perf_counter() - t)


def graph_us(fn, calls=50, reps=7):
    """us per call of fn(i), i = 0 .. calls, replayed from one hipGraph (the device alone)."""
    import torch

    for i in range(2):
        fn(i)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(calls):
            fn(i)
    graph.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / calls)
    return [statistics.median(times), min(times), max(times)]


def kernel_figures(model, ds, B=8):
    import torch

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet_predict import channel_kinds

    raw = ds.ds
    obs, series = raw.obs_window, raw.chunks[0]
    t0 = torch.arange(B, device=DEV)
    X = [torch.empty(B, obs * C, H, W, device=DEV) for _ in range(2)]
    out = torch.randn(B, C, H, W, device=DEV)
    kind = channel_kinds(C, STATIC, FORCING).to(DEV)
    state = torch.zeros(AR, C, 5, dtype=torch.float64, device=DEV)
    acc_count = torch.zeros(AR, C, dtype=torch.int64, device=DEV)
    count = torch.zeros(AR, dtype=torch.int64, device=DEV)
    ws = torch.empty(int(hip.lib().gcl_grid_forecast_step_ws_bytes(B, H, W, C)) // 8, dtype=torch.float64, device=DEV)
    plane, frame = 4 * B * C * H * W, 2 * B * H * W * C  # bytes of one planar frame, of one series frame (Ct = C here)
    figures = {}
    for name, nbytes, fn in (
            ("grid_window_pack", obs * (frame + plane),
             lambda i: hip.grid_window_pack(series, t0, raw.mean, raw.std, obs, out=X[0])),
            # pass 1 reads out, frames 1 .. obs-1 of X and two series frames, writes X_next; pass 2 reads out' and one frame
            ("grid_forecast_step", plane * (1 + (obs - 1) + obs + 1) + 3 * frame,
             lambda i: hip.grid_forecast_step(out, X[i % 2], series, t0, kind, raw.mean, raw.std, i % AR, X[1 - i % 2], state,
                                              acc_count, count, ws=ws))):
        us = graph_us(fn)
        figures[name] = {"us": us, "bytes": nbytes, "GB_per_s": nbytes / us[0] / 1e3, "share_of_hbm": nbytes / (us[0] * 1e-6) / HBM}
    hip.grid_window_pack(series, t0, raw.mean, raw.std, obs, out=X[0])
    figures["network_us"] = graph_us(lambda i: model(X[0], residual_from=((obs - 1) * C, obs * C)), calls=10)
    return figures


def bench_arch(arch, n_samples, reps):
    import torch

    from graphcast_lite_amd.unet_predict import GridForecaster

    model = make_model(arch)
    ds = make_dataset(ARCHS[arch]["obs"], n_samples)

    def forecaster(bs, graph):
        return GridForecaster(model, ds, STATIC, FORCING, AR, batch_size=bs, use_graph=graph)

    runners = {"b8_graph": forecaster(8, True), "b1_graph": forecaster(1, True), "b8_eager": forecaster(8, False),
               "b8_torch_glue": TorchGlue(model, ds, 8)}

    def run(name, n):
        r, bs = runners[name], 1 if name == "b1_graph" else 8
        for first in range(0, n, bs):
            r.update(range(first, min(first + bs, n)))

    for name in runners:  # warm-up: packs, workspaces, the graph captures
        run(name, 32)
    torch.cuda.synchronize()
    assert runners["b8_graph"].graph_active and runners["b1_graph"].graph_active
    a, b = runners["b8_graph"].state[:, :, :4], runners["b8_torch_glue"].state[:, :, :4]
    dyn = [c for c in range(C) if c not in STATIC + FORCING]
    check = float(((a - b).abs() / b.abs())[:, dyn].max())
    rates = {name: [] for name in runners}
    for _ in range(reps):
        for name in runners:
            rates[name].append(timed(lambda: run(name, n_samples), n_samples))
    res = {name: [statistics.median(v), min(v), max(v)] for name, v in rates.items()}
    res["check"] = check
    res["kernels"] = kernel_figures(model, ds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--archs", default="v1,v2")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("unet_forecast_bench needs a GPU: a CPU run measures nothing")
    res = {"shape": {"H": H, "W": W, "C": C, "pred": PRED, "ar": AR, "static": STATIC, "forcing": FORCING, "archs": ARCHS},
           "samples": args.samples, "reps": args.reps, "unit": "samples/s [median, min, max]"}
    for arch in args.archs.split(","):
        res[arch] = bench_arch(arch, args.samples, args.reps)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
