"""Device ms per sample of `pipeline.FullPipelineEvaluator.update` with every variant on, next to its stages run
separately (multires window + rollout, the three learned-MOS calls, station observations + OI, and the glue kernels of
csrc/pipeline.hip), at the script's shape: 512 x 256 global, 61 x 41 regional box, 19 features, 19 stations, AR 4.

The model is a stand-in (half the difference of the two input frames), so the rollout figure is the window pack and
the AR glue only - the point of the record is the glue between the stages, not the forecaster.  The forest is a random
one of the shipped bundle's size (500 trees of depth 5).  Synthetic series.

    python tools/pipeline_bench.py [--reps R] [--warmup W]

Prints one JSON line.  Timing: HIP events around each repetition, the median of R after W warm-ups.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from multires_bench import ROI, write_dataset  # noqa: E402

VAR_ORDER = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm", "t@850", "u@850", "v@850", "z@850",
             "q@850", "t@500", "u@500", "v@500", "z@500", "q@500"]
AR, T = 4, 16


class DiffModel(torch.nn.Module):
    obs_window = 2

    def forward(self, X, attention_threshold=0.0, **kw):
        C = X.shape[-1] // 2
        return 0.5 * (X[..., C:] - X[..., :C])


def random_forest(rng, trees=500, depth=5):
    from graphcast_lite_amd.mos import MOSForest

    per = 2 ** (depth + 1) - 1
    n = trees * per
    local = np.arange(per)
    leaf = np.tile(local >= 2 ** depth - 1, trees)
    base = np.repeat(np.arange(trees) * per, per)
    left, right = base + np.tile(2 * local + 1, trees), base + np.tile(2 * local + 2, trees)
    feature = rng.integers(0, 20, n)
    value = np.where(leaf, rng.normal(0, 0.01, n), rng.normal(0, 10, n))
    return MOSForest(np.where(leaf, 0, feature), value, np.where(leaf, 0, left), np.where(leaf, 0, right),
                     rng.integers(0, 2, n), leaf, np.arange(trees) * per, 0.0)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.assimilation import OptimalInterpolation
    from graphcast_lite_amd.multires import MultiresChunkDataset
    from graphcast_lite_amd.pipeline import FullPipelineEvaluator
    from graphcast_lite_amd.predict import rollout

    assert torch.cuda.is_available(), "pipeline_bench needs a GPU"
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    g_lats, g_lons = np.linspace(-90, 90, 256), np.linspace(0, 360, 512, endpoint=False)
    r_lats, r_lons = ROI[0] + 0.25 * np.arange(41), ROI[2] + 0.25 * np.arange(61)
    stations = [{"lat": float(a), "lon": float(o), "elev": float(e)} for a, o, e in
                zip(rng.uniform(53.5, 58, 19), rng.uniform(89, 96, 19), rng.uniform(90, 480, 19))]
    with tempfile.TemporaryDirectory() as d:
        gdir = write_dataset(os.path.join(d, "global"), T, g_lats, g_lons, rng)
        rdir = write_dataset(os.path.join(d, "region"), T, r_lats, r_lons, rng)
        ds = MultiresChunkDataset(gdir, rdir, ROI, mode="merge", obs_window=2, pred_steps=AR, split="all", device=dev,
                                  quantize=False)
    oi = OptimalInterpolation(r_lats, r_lons, 1.5, 0.5, 100_000.0, dev)
    ev = FullPipelineEvaluator(DiffModel(), ds, None, VAR_ORDER, np.zeros(19, np.float32), np.ones(19, np.float32),
                               stations, AR, np.float64(250.0), mos=random_forest(rng), oi=oi, use_residual=True)
    C, V = 19, len(ev.variants)
    t0 = torch.tensor([3], dtype=torch.int64, device=dev)
    X, _ = ds.windows(t0, 2, 0, C)
    out = rollout(ev.model, X, AR, use_residual=True)
    phys, _ = hip.window_pack(ev.rs, t0 + 1, ev._zeros, ev._ones, C, 1 + AR, 0)
    truth = [phys[0, :, (1 + h) * C:(2 + h) * C] for h in range(AR)]
    as3 = lambda t: t.view(ev.G, 1, C)  # noqa: E731
    buf = ev._buf

    def stage_rollout():
        x, _ = ds.windows(t0, 2, 0, C)
        rollout(ev.model, x, AR, use_residual=True)

    def stage_mos():
        for h in range(AR):
            ev._mos_stn.apply(as3(buf[0]), ev._tfeat[h], out=as3(buf[2]))
            ev._mos_stn.apply(as3(buf[1]), ev._tfeat[h], out=as3(buf[3]))
            ev._mos_idw.apply(as3(buf[1]), ev._tfeat[h], out=as3(buf[4]))

    def stage_oi():
        for h in range(AR):
            hip.pipeline_station_obs(truth[h], ev._sim, out=ev._obs)
            ev._oi_net.apply(buf[4], ev._obs, out=buf[5])

    def stage_glue():
        hip.window_pack(ev.rs, t0 + 1, ev._zeros, ev._ones, C, 1 + AR, 0)
        for h in range(AR):
            hip.pipeline_roi_phys(out[0, :, h * C:(h + 1) * C], None, None, ev.n_kept, ev.G, ev.mean, ev.std, ev.t_idx,
                                  ev.z_idx, ev.lapse_elev, ev.lapse_f64, buf[0], buf[1])
            hip.pipeline_sqerr(buf, truth[h], ev._score, h, ev._acc_grid[:V - 1], ev._acc_stn[:V - 1])
            hip.pipeline_sqerr(phys[:, :, :C], truth[h], ev._score, h, ev._acc_grid[V - 1:], ev._acc_stn[V - 1:])

    res = {"tool": "pipeline_bench", "device": torch.cuda.get_device_name(0), "nodes": ds.n_nodes, "regional": ev.G,
           "features": C, "stations": len(stations), "ar": AR, "variants": V, "reps": args.reps, "warmup": args.warmup}
    res["evaluator_ms_per_sample"] = timed(lambda: ev.update([3]), args.reps, args.warmup)
    for name, fn in (("rollout", stage_rollout), ("mos_x3", stage_mos), ("oi", stage_oi), ("glue", stage_glue)):
        res[f"{name}_ms"] = timed(fn, args.reps, args.warmup)
    res["stages_sum_ms"] = sum(res[f"{k}_ms"] for k in ("rollout", "mos_x3", "oi", "glue"))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
