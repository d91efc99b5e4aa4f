"""Generate the downscaler data-layer fixtures by RUNNING the reference's own `scripts/build_downscaler_dataset.py`
(by runpy, with its command line), `crop_and_upsample_roi` of `scripts/generate_gnn_predictions.py`, and
`DownscalerDataset` / `compute_metrics` of `scripts/train_downscaler.py` on the CPU.

Run from the repo root, only where the reference checkout (`make_golden.REF`) and scipy exist (never on the GPU box):

    python tests/golden/make_downscale_golden.py

The inputs come from tests/helpers/downscale_case.py (global 24 x 12, regional 9 x 7, box (15, 46, 60, 120), 5
variables, 12 frames).  The seed is the first for which at least one coarse value differs between the direct float64 ->
binary16 rounding and the rounding through float32.  Output (data only - arrays and recorded JSON text, no reference
source text): tests/golden/downscale_vectors.npz
  seed, g_data, r_data             the two fp16 series
  coarse, fine                     coarse.npy / fine.npy as the builder wrote them
  static_fine, sc_mean, sc_std, sc_n, lat32, lon32   static_fine.npy, scalers.npz and coords.npz arrays
  info, variables                  dataset_info.json / variables.json text (the *_source strings are downscale_case's)
  n_two_step                       how many coarse values the rounding through float32 would change
  grid_lats, grid_lons, flat_data  the multires node set (build_multires_coords) and the reference's interpolate-mode
                                   data.npy on it: the GNN's data set
  crop_in, crop_out                a float32 (G, C) field and crop_and_upsample_roi of it (flat grid)
  gnn_<res|abs>_<subsample>        gnn_pred.npy as the main() of generate_gnn_predictions.py writes it (run by its
                                   command line; the loaders of its experiment directory are replaced so that they
                                   hand it tests/helpers/diff_stub.py and the flat data set), gnn_*_count: the count
                                   it reports
  len_<split>                      DownscalerDataset lengths (obs 2)
  X<i>, Y<i>                       its items i of the "all" split (obs 2, statics); o3_X1, o3_Y1: obs 3, no statics;
                                   gnn_X4: item 4 with use_gnn_input over gnn_res_1
  rmse_coarse_all, rmse_coarse_train   the baseline column of compute_metrics, one batch holding the whole split
"""
import contextlib
import importlib.util
import io
import json
import os
import re
import runpy
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402  (where the reference checkout lives, placeholder modules)
import downscale_case as DC  # noqa: E402
import multires_case as MC  # noqa: E402
from diff_stub import DiffStub  # noqa: E402

REF = make_golden.REF


def _load(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_builder(gdir, rdir, odir):
    argv = sys.argv
    sys.argv = ["build_downscaler_dataset.py", "--global-dir", gdir, "--region-dir", rdir, "--roi",
                *[str(v) for v in DC.ROI], "--out-dir", odir, "--static-channels", *[str(c) for c in DC.STATIC]]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            runpy.run_path(os.path.join(REF, "scripts", "build_downscaler_dataset.py"), run_name="__main__")
    finally:
        sys.argv = argv


def choose_seed(tmp):
    """The first seed whose coarse archive holds a value that two-step rounding would change; the float64 restatement
    over the host tables must reproduce the reference's bytes."""
    from graphcast_lite_amd.downscale import coarse_tables, roi_crop

    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    la0, la1, lo0, lo1 = roi_crop(g_lats, g_lons, DC.ROI)
    assert la1 - la0 >= 2 and lo1 - lo0 >= 2, "the crop needs at least 2 nodes per axis"
    pos, w = coarse_tables(g_lats, g_lons, r_lats, r_lons, DC.ROI)
    print(f"crop {lo1 - lo0} x {la1 - la0}, weights in [{w.min():.2f}, {w.max():.2f}]")
    for seed in range(1, 100):
        g_data, r_data = DC.pair(seed)
        acc = DC.restate_coarse(g_data, pos, w)
        n_two = int(np.count_nonzero(acc.astype(np.float16) != acc.astype(np.float32).astype(np.float16)))
        if n_two >= 1:
            break
    else:
        raise SystemExit("no seed separates the two roundings")
    root = os.path.join(tmp, f"seed{seed}")
    gdir, rdir = DC.write_pair(root, g_data, r_data)
    odir = os.path.join(root, "out")
    run_builder(gdir, rdir, odir)
    shape = (DC.T, len(r_lons), len(r_lats), DC.C)
    coarse = np.fromfile(os.path.join(odir, "coarse.npy"), dtype=np.float16).reshape(shape)
    assert coarse.tobytes() == acc.astype(np.float16).reshape(shape).tobytes(), "the restatement misses the reference"
    return seed, n_two, g_data, r_data, gdir, rdir, odir, coarse


def gnn_dataset(tmp, gdir, rdir):
    """The flat multires data set of the GNN (the reference's interpolate mode) with its own scalers."""
    import argparse

    B = _load("_ref_build_multires", "scripts", "build_multires_dataset.py")
    E = _load("_ref_eval_pipeline", "scripts", "evaluate_full_pipeline.py")
    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    mc = E.build_multires_coords(g_lats, g_lons, r_lats, r_lons, DC.ROI)
    odir = os.path.join(tmp, "flat")
    with contextlib.redirect_stdout(io.StringIO()):
        B.build_interpolate_mode(argparse.Namespace(global_dir=gdir, roi=list(DC.ROI), out_dir=odir,
                                                    region_coords=os.path.join(rdir, "coords.npz")))
    mean, std = DC.gnn_scalers()
    np.savez(os.path.join(odir, "scalers.npz"), mean=mean, std=std)
    flat = np.fromfile(os.path.join(odir, "data.npy"), dtype=np.float16).reshape(DC.T, len(mc[0]), DC.C)
    return odir, mc[0], mc[1], flat


def run_generator(G, ds_cls, flat_dir, grid_lats, grid_lons, pairs_dir, use_residual, subsample):
    """The reference's own main() of generate_gnn_predictions.py, by its command line.  What it loads from an experiment
    directory is handed to it instead: the stub as the model, an empty checkpoint, a configuration of the three fields
    it reads, and the three splits of the flat data set with the node coordinates as their metadata.  The loop, the
    crop, the denormalisation and the memmap are the reference's, untouched.  Returns gnn_pred.npy and the count its
    last line reports."""
    from types import SimpleNamespace

    exp = os.path.join(pairs_dir, "experiment")
    os.makedirs(exp, exist_ok=True)
    torch.save({}, os.path.join(exp, "best_model.pth"))
    cfg = SimpleNamespace(data=SimpleNamespace(obs_window_used=DC.OBS, num_features_used=DC.C), data_dir=flat_dir,
                          use_residual=use_residual)

    def datasets(data_path, obs_window, pred_steps, n_features):
        sets = [ds_cls(data_path, obs_window=obs_window, pred_steps=pred_steps, split=sp) for sp in ("train", "val", "test_only")]
        return (*sets, SimpleNamespace(flat_grid=True, cordinates=(grid_lats, grid_lons)))

    G.load_from_json_file = lambda path: {}
    G.ExperimentConfig = lambda **kw: cfg
    G.load_chunked_datasets = datasets
    G.load_model_from_experiment_config = lambda *a, **kw: DiffStub(DC.OBS, DC.C)
    argv, text = sys.argv, io.StringIO()
    sys.argv = ["generate_gnn_predictions.py", exp, "--downscaler-data", pairs_dir, "--roi", *[str(v) for v in DC.ROI],
                "--subsample", str(subsample), "--device", "cpu"]
    try:
        with contextlib.redirect_stdout(text):
            G.main()
    finally:
        sys.argv = argv
    count = int(re.search(r"Generated (\d+) GNN predictions", text.getvalue()).group(1))
    with open(os.path.join(pairs_dir, "dataset_info.json")) as fh:
        info = json.load(fh)
    shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
    return np.fromfile(os.path.join(pairs_dir, "gnn_pred.npy"), dtype=np.float16).reshape(shape), count


class LastFrame(torch.nn.Module):
    """The model compute_metrics is driven with: its baseline column does not depend on it."""

    def forward(self, X):
        return X[:, :DC.C]


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    warnings.filterwarnings("ignore")
    make_golden._placeholders()
    sys.path.insert(0, REF)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        seed, n_two, g_data, r_data, gdir, rdir, odir, coarse = choose_seed(tmp)
        shape = coarse.shape
        out.update(seed=np.int64(seed), n_two_step=np.int64(n_two), g_data=g_data, r_data=r_data, coarse=coarse)
        out["fine"] = np.fromfile(os.path.join(odir, "fine.npy"), dtype=np.float16).reshape(shape)
        out["static_fine"] = np.load(os.path.join(odir, "static_fine.npy"))
        sc = np.load(os.path.join(odir, "scalers.npz"))
        out["sc_mean"], out["sc_std"], out["sc_n"] = sc["mean"], sc["std"], sc["n"]
        co = np.load(os.path.join(odir, "coords.npz"))
        out["lat32"], out["lon32"] = co["latitude"], co["longitude"]
        with open(os.path.join(odir, "dataset_info.json")) as fh:
            info = json.load(fh)
        info["global_source"], info["region_source"] = DC.GLOBAL_SOURCE, DC.REGION_SOURCE
        out["info"] = np.array(json.dumps(info))
        with open(os.path.join(odir, "variables.json")) as fh:
            out["variables"] = np.array(fh.read())

        G = _load("_ref_gen_gnn", "scripts", "generate_gnn_predictions.py")
        from src.data.dataloader_chunked import TimeseriesChunkDataset

        flat_dir, grid_lats, grid_lons, flat = gnn_dataset(tmp, gdir, rdir)
        out["grid_lats"], out["grid_lons"], out["flat_data"] = grid_lats, grid_lons, flat
        t_lats, t_lons = out["lat32"].astype(np.float64), out["lon32"].astype(np.float64)
        rng = np.random.default_rng(77)
        out["crop_in"] = rng.standard_normal((len(grid_lats), DC.C)).astype(np.float32)
        out["crop_out"] = G.crop_and_upsample_roi(out["crop_in"], grid_lats, grid_lons, DC.ROI, t_lats, t_lons,
                                                  flat_grid=True)
        assert out["crop_out"].dtype == np.float32 and out["crop_out"].shape == (len(t_lats), len(t_lons), DC.C)
        for tag, res in (("res", True), ("abs", False)):
            for sub in (1, 2):
                arr, cnt = run_generator(G, TimeseriesChunkDataset, flat_dir, grid_lats, grid_lons, odir, res, sub)
                assert arr.shape == shape
                out[f"gnn_{tag}_{sub}"], out[f"gnn_{tag}_{sub}_count"] = arr, np.int64(cnt)
        assert out["gnn_res_1_count"] > out["gnn_res_2_count"] > 0
        assert np.any(out["gnn_res_1"] != out["gnn_abs_1"])

        out["gnn_res_1"].tofile(os.path.join(odir, "gnn_pred.npy"))
        TD = _load("_ref_train_downscaler", "scripts", "train_downscaler.py")
        with contextlib.redirect_stdout(io.StringIO()):
            for split in DC.SPLITS:
                ds = TD.DownscalerDataset(odir, obs_window=DC.OBS, split=split)
                out[f"len_{split}"] = np.int64(len(ds))
                if split in ("all", "train"):
                    loader = torch.utils.data.DataLoader(ds, batch_size=len(ds), shuffle=False)
                    _, rmse_coarse, _ = TD.compute_metrics(LastFrame(), loader, "cpu", None, False, DC.C,
                                                           torch.from_numpy(ds.std))
                    assert rmse_coarse.dtype == np.float32
                    out[f"rmse_coarse_{split}"] = rmse_coarse
            for i in DC.SAMPLES:
                X, Y = ds[i]
                out[f"X{i}"], out[f"Y{i}"] = X.numpy(), Y.numpy()
            X, Y = TD.DownscalerDataset(odir, obs_window=3, split="all", static_context=False)[1]
            out["o3_X1"], out["o3_Y1"] = X.numpy(), Y.numpy()
            out["gnn_X4"] = TD.DownscalerDataset(odir, obs_window=DC.OBS, split="all", use_gnn_input=True)[4][0].numpy()
    np.savez_compressed(DC.GOLDEN, **out)
    print(f"wrote {DC.GOLDEN} ({os.path.getsize(DC.GOLDEN) / 1e3:.1f} kB, {len(out)} arrays); seed {seed}, "
          f"{n_two} of {coarse.size} coarse values separate the roundings")


if __name__ == "__main__":
    main()
