"""A cached training epoch of the dual-mesh regional model at the `experiments/dual_mesh_krsk` shape of
tools/dual_mesh_bench.py, two ways in one call, alternating:

  parent  `DualMeshCachedStep` fed `precompute_global`'s CPU dictionaries step by step (three uploads a step)
  cache   `DualMeshCacheStep` over a `GlobalOutputCache` (a device slot index a step)

and `eval_dual` (one lock-step pass) against two separate rollouts scored with `weighted_mse_loss`.

    python tools/regional_train_bench.py [--samples N] [--rounds R] [--out profiles/regional_train_bench.json]

Per path: the epoch's wall time per sample (host clock around the epoch, one sync at its end) for every round, the
median and the spread (max - min over the rounds); host-to-device bytes per step; cache bytes per sample.  The first
epoch of each path (warm-up and capture) is not counted.  Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dual_mesh_bench import ROI, flat_grid  # noqa: E402
from roi_bench import krsk_config  # noqa: E402

KEYS = ("global_pred_roi", "roi_grid_latent", "cross_sender_feat")


def build(dev):
    from graphcast_lite_amd.dual_mesh import DualMeshModel
    from graphcast_lite_amd.models import WeatherPrediction

    cfg = krsk_config()
    lats, lons = flat_grid()
    torch.manual_seed(42)
    gm = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev, flat_grid=True)
    return cfg, DualMeshModel(gm, ROI, lats, lons, dev, reg_mesh_level=7, reg_mesh_buffer=2.0, reg_processor_steps=4,
                              cross_k=3, hidden_dim=256)


def stats(per_sample_ms):
    return {"rounds_ms": [round(v, 4) for v in per_sample_ms], "median_ms": round(statistics.median(per_sample_ms), 4),
            "spread_ms": round(max(per_sample_ms) - min(per_sample_ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regional_train_bench.json"))
    args = ap.parse_args()

    from graphcast_lite_amd import hip
    from graphcast_lite_amd.dual_mesh import DualMeshCachedStep
    from graphcast_lite_amd.regional_train import DualMeshCacheStep, GlobalOutputCache, eval_dual
    from graphcast_lite_amd.train import weighted_mse_loss

    assert torch.cuda.is_available(), "regional_train_bench needs a GPU"
    hip.lib()
    dev = torch.device("cuda:0")
    cfg, m_parent = build(dev)
    _, m_cache = build(dev)  # the same seed: a twin, so that both paths train the same thing
    G, Fe, N = m_parent.global_model._num_grid_nodes, cfg.data.num_features_used, args.samples
    g = torch.Generator().manual_seed(1234)
    data = [(torch.randn(1, G, 2 * Fe, generator=g), torch.randn(1, G, 2 * Fe, generator=g)) for _ in range(N)]
    mask = m_parent.roi_mask

    # parent: precompute_global's CPU dictionaries; the window and the target come from the loader on the device
    fed = []
    for X, y in data:
        Xd = X.to(dev)
        fed.append((Xd[0][mask], m_parent.precompute_global(Xd), y.to(dev)[0][mask][:, :Fe].contiguous()))
    h2d_parent = sum(v.numel() * v.element_size() for v in fed[0][1].values())
    cache = GlobalOutputCache.build(m_cache, data, "train", log=lambda s: None)
    s_parent = DualMeshCachedStep(m_parent, lr=5e-4, use_residual=True, use_graph=True)
    s_cache = DualMeshCacheStep(m_cache, cache, lr=5e-4, use_residual=True, use_graph=True)
    order = torch.arange(N, dtype=torch.int64, device=dev)

    def epoch_parent():
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for raw, c, y_roi in fed:
            total += s_parent(raw, *(c[k] for k in KEYS), y_roi)
        return total.item() / N

    def epoch_cache():
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for i in range(N):
            total += s_cache(order[i:i + 1])
        return total.item() / N

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / N, loss

    l_parent, l_cache = clock(epoch_parent)[1], clock(epoch_cache)[1]  # warm-up and capture
    assert s_parent.graph_active and s_cache.graph_active, (s_parent.launch_mode, s_cache.launch_mode)
    t_parent, t_cache = [], []
    for _ in range(args.rounds):  # alternating, so that drift hits both alike
        t_parent.append(clock(epoch_parent)[0])
        t_cache.append(clock(epoch_cache)[0])
    res = {"tool": "regional_train_bench", "samples": N, "rounds": args.rounds, "n_roi": m_parent.n_roi_grid,
           "half_E": cache.rec.half_E, "grid_points": G,
           "first_epoch_loss": {"parent": l_parent, "cache": l_cache},
           "parent": dict(stats(t_parent), h2d_bytes_per_step=h2d_parent),
           "cache": dict(stats(t_cache), h2d_bytes_per_step=0, slot_bytes_per_step=8,
                         cache_bytes_per_sample=cache.rec.nbytes)}
    res["speedup_median"] = round(res["parent"]["median_ms"] / res["cache"]["median_ms"], 3)
    res["accepted"] = res["cache"]["median_ms"] <= res["parent"]["median_ms"] + res["parent"]["spread_ms"]

    # eval_dual (two AR steps) against two separate rollouts + weighted_mse_loss
    val = data[:max(N // 2, 1)]
    mask3 = mask.view(1, -1, 1).float()

    def separate():
        from graphcast_lite_amd.predict import rollout

        tot = [0.0, 0.0]
        with torch.no_grad():
            for X, y in val:
                Xd, yd = X.to(dev), y.to(dev)
                for q, model in enumerate((m_cache, m_cache.global_model)):
                    outs = rollout(model, Xd, 2, y=yd, use_residual=True)
                    tot[q] += weighted_mse_loss(outs, yd, spatial_mask=mask3).item()
        return tot[0] / len(val), 1.0 - tot[0] / tot[1]

    def lockstep():
        return eval_dual(m_cache, val, dev, use_residual=True, current_ar_steps=2)

    for fn in (separate, lockstep):
        fn()
    te_sep, te_lock, got = [], [], None
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        want = separate()
        torch.cuda.synchronize()
        te_sep.append((time.perf_counter() - t0) * 1e3 / len(val))
        t0 = time.perf_counter()
        got = lockstep()
        torch.cuda.synchronize()
        te_lock.append((time.perf_counter() - t0) * 1e3 / len(val))
    res["eval_dual"] = {"batches": len(val), "ar_steps": 2, "separate_rollouts": stats(te_sep), "lockstep": stats(te_lock),
                        "loss": {"separate": want[0], "lockstep": got[0]}, "skill": {"separate": want[1], "lockstep": got[1]}}
    res["peak_hbm_gib"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
