"""ms per dual-mesh regional training step (src/dual_mesh.py + scripts/train_dual_mesh.py) at the
`experiments/dual_mesh_krsk` shape: the full step (frozen global forward + regional module) and the reference's cached
mode (`precompute_global` once per sample, then `forward_cached` steps), eager and hipGraph-captured.

Shape: the krsk global model (InteractionNet processor, 12 steps, latent 256, mesh levels [4, 6], 19 features,
2 observation steps) on a synthetic flat grid - a 1-degree global grid whose points inside the ROI box are replaced by a
0.25-degree patch of 41 x 61 points - and the driver's regional module: level-7 regional mesh with a 2-degree buffer
(467 nodes), 4 shared processor steps, cross_k 3, hidden 256, batch 1.

    python tools/dual_mesh_bench.py [--steps K] [--warmup W]

Prints one JSON line.  Timing: HIP events around K steps after W warm-up steps, one sync at the end.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from roi_bench import krsk_config, timed  # noqa: E402

ROI = (50.0, 60.0, 83.0, 98.0)


def flat_grid():
    lat_c, lon_c = np.meshgrid(np.arange(-90.0, 90.5, 1.0), np.arange(0.0, 360.0, 1.0), indexing="ij")
    lat_c, lon_c = lat_c.ravel(), lon_c.ravel()
    inside = (lat_c >= ROI[0]) & (lat_c <= ROI[1]) & (lon_c >= ROI[2]) & (lon_c <= ROI[3])
    lat_f, lon_f = np.meshgrid(ROI[0] + 0.25 * np.arange(41), ROI[2] + 0.25 * np.arange(61), indexing="ij")
    lats = np.concatenate([lat_c[~inside], lat_f.ravel()]).astype(np.float32)
    lons = np.concatenate([lon_c[~inside], lon_f.ravel()]).astype(np.float32)
    return lats, lons


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.dual_mesh import DualMeshCachedStep, DualMeshModel
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.train import TrainStep

    assert torch.cuda.is_available(), "dual_mesh_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    cfg = krsk_config()
    lats, lons = flat_grid()
    t0 = time.time()
    torch.manual_seed(42)
    gm = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev, flat_grid=True)
    dm = DualMeshModel(gm, ROI, lats, lons, dev, reg_mesh_level=7, reg_mesh_buffer=2.0, reg_processor_steps=4,
                       cross_k=3, hidden_dim=256)
    setup_s = time.time() - t0
    G, Fe = gm._num_grid_nodes, cfg.data.num_features_used
    g = torch.Generator().manual_seed(1234)
    X = torch.randn(1, G, 2 * Fe, generator=g).to(dev)
    y = torch.randn(1, G, Fe, generator=g).to(dev)
    mask = dm.roi_mask
    mask3 = mask.view(1, -1, 1).float()

    def glob():
        with torch.no_grad():
            gm.forward_with_latents(X)

    res = {"tool": "dual_mesh_bench", "grid_points": G, "mesh_nodes": gm._num_mesh_nodes, "n_roi": dm.n_roi_grid,
           "n_reg_mesh": dm.n_reg_mesh, "reg_edges": int(dm.reg_processing_edges.shape[1]),
           "cross_edges_used": int(dm.cross_edge_index.shape[1] // 2), "hidden": 256, "processor_steps": 4,
           "cross_k": 3, "batch": 1,
           "regional_params": sum(p.numel() for n, p in dm.named_parameters() if not n.startswith("global_model.")),
           "steps": args.steps, "warmup": args.warmup, "setup_s": round(setup_s, 1)}
    res["global_fwd_ms"] = timed(glob, args.steps, args.warmup)
    for mode, use_graph in (("eager", False), ("captured", True)):
        step = TrainStep(dm, lr=1e-3, spatial_mask=mask3, use_residual=False, use_graph=use_graph)
        res[f"full_{mode}_step_ms"] = timed(lambda: step(X, y), args.steps, args.warmup)
        if use_graph:
            assert step.graph_active, step.launch_mode
    res["global_share_full_captured"] = res["global_fwd_ms"] / res["full_captured_step_ms"]

    cache = {}

    def pre():
        cache.update(dm.precompute_global(X))  # ends in the device-to-host copies (a sync)

    res["precompute_ms_per_sample"] = timed(pre, args.steps, args.warmup)
    keys = ("global_pred_roi", "roi_grid_latent", "cross_sender_feat")
    raw, y_roi = X[0][mask], y[0][mask]
    cdev = [cache[k].to(dev) for k in keys]
    for mode, use_graph in (("eager", False), ("captured", True)):
        cs = DualMeshCachedStep(dm, lr=1e-3, use_residual=True, use_graph=use_graph)
        res[f"cached_{mode}_step_ms"] = timed(lambda: cs(raw, *cdev, y_roi), args.steps, args.warmup)
        if use_graph:
            assert cs.graph_active, cs.launch_mode
    res["peak_hbm_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
