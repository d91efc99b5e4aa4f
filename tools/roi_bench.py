"""ms per ROI residual training step (src/roi_residual.py + scripts/train_roi_residual.py:112-116) at the
`experiments/roi_residual_krsk` shape, eager and hipGraph-captured, and how much of it is the frozen global forward.

Shape: the config's global model (InteractionNet processor, 12 steps, latent 256, mesh levels [4, 6], 19 features,
2 observation steps) on a synthetic flat grid - a 1-degree global grid whose points inside the ROI box are replaced by a
0.25-degree patch of 61 x 41 points - and the driver's default head: hidden 256, 6 processor steps, k = 8, batch 1.

    python tools/roi_bench.py [--steps K] [--warmup W]

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

ROI = (50.0, 65.0, 85.0, 95.0)


def krsk_config():
    from graphcast_lite_amd.config import ExperimentConfig

    return ExperimentConfig(**{
        "graph": {"grid2mesh_edge_creation": "radius", "mesh2grid_edge_creation": "contained",
                  "grid2mesh_radius_query": 0.6, "mesh_levels": [4, 6]},
        "pipeline": {
            "encoder": {"mlp": {"mlp_hidden_dims": [256, 256], "output_dim": 256, "use_layer_norm": True,
                                "layer_norm_mode": "node"},
                        "gcn": {"layer_type": "conv_gcn", "hidden_dims": [256, 256], "output_dim": 256,
                                "activation": "swish"}},
            "processor": {"gcn": {"layer_type": "interaction_net", "output_dim": 256, "activation": "swish",
                                  "use_layer_norm": True, "num_message_passing_steps": 12, "edge_feature_dim": 4}},
            "decoder": {"mlp": {"mlp_hidden_dims": [256, 128], "output_dim": 128, "use_layer_norm": False},
                        "gcn": {"layer_type": "conv_gcn", "hidden_dims": [128, 128], "output_dim": 19,
                                "activation": "swish"}},
        },
        "data": {"dataset_name": "multires", "num_features_used": 19, "obs_window_used": 2, "pred_window_used": 1,
                 "want_feats_flattened": True},
    })


def flat_grid():
    lat_c, lon_c = np.meshgrid(np.arange(-90.0, 90.5, 1.0), np.arange(0.0, 360.0, 1.0), indexing="ij")
    lat_c, lon_c = lat_c.ravel(), lon_c.ravel()
    inside = (lat_c >= ROI[0]) & (lat_c <= ROI[1]) & (lon_c >= ROI[2]) & (lon_c <= ROI[3])
    lat_f, lon_f = np.meshgrid(ROI[0] + 0.25 * np.arange(61), ROI[2] + 0.25 * np.arange(41), indexing="ij")
    lats = np.concatenate([lat_c[~inside], lat_f.ravel()]).astype(np.float32)
    lons = np.concatenate([lon_c[~inside], lon_f.ravel()]).astype(np.float32)
    return lats, lons


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.roi_residual import ROIResidualModel
    from graphcast_lite_amd.train import TrainStep

    assert torch.cuda.is_available(), "roi_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    cfg = krsk_config()
    lats, lons = flat_grid()
    t0 = time.time()
    torch.manual_seed(42)
    gm = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev, flat_grid=True)
    roi = ROIResidualModel(gm, ROI, lats, lons, dev, hidden_dim=256, processor_steps=6, roi_k=8)
    setup_s = time.time() - t0
    G, Fe = gm._num_grid_nodes, cfg.data.num_features_used
    g = torch.Generator().manual_seed(1234)
    X = torch.randn(1, G, 2 * Fe, generator=g).to(dev)
    y = torch.randn(1, G, Fe, generator=g).to(dev)
    mask3 = roi.roi_mask.view(1, -1, 1).float()

    def glob():
        with torch.no_grad():
            gm.forward_with_latents(X)

    res = {"tool": "roi_bench", "grid_points": G, "mesh_nodes": gm._num_mesh_nodes, "n_roi": roi.n_roi_grid,
           "roi_edges": int(roi.roi_edge_index.shape[1]), "hidden": 256, "processor_steps": 6, "k": 8, "batch": 1,
           "head_params": sum(p.numel() for n, p in roi.named_parameters() if not n.startswith("global_model.")),
           "steps": args.steps, "warmup": args.warmup, "setup_s": round(setup_s, 1)}
    res["global_fwd_ms"] = timed(glob, args.steps, args.warmup)
    for mode, use_graph in (("eager", False), ("captured", True)):
        step = TrainStep(roi, lr=1e-3, spatial_mask=mask3, use_residual=False, use_graph=use_graph)
        res[f"{mode}_step_ms"] = timed(lambda: step(X, y), args.steps, args.warmup)
        if use_graph:
            assert step.graph_active, step.launch_mode
    res["global_share_captured"] = res["global_fwd_ms"] / res["captured_step_ms"]
    res["peak_hbm_gib"] = torch.cuda.max_memory_allocated() / 2 ** 30
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
