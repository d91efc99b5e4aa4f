"""The data layer of the U-Net downscaler cascade: everything that feeds the network, from the fp16 series in HBM.

The reference prepares this on the host in hours: `scripts/build_downscaler_dataset.py` builds the (coarse, fine) pairs
with one scipy `RegularGridInterpolator` per frame and channel, `scripts/generate_gnn_predictions.py` runs the frozen
GNN one sample at a time with 19 interpolators per sample, and `DownscalerDataset` / `compute_metrics` of
`scripts/train_downscaler.py` pack batches and score the coarse baseline from memmaps.  Here the point tables are
built once on the host (`verify.find_cells` / `verify.regrid_tables`, the same corner order and weights as scipy's)
and the arithmetic runs in `csrc/downscale.hip`: `gcl_downscale_coarse`, `gcl_downscale_pred`, `gcl_downscale_batch`
and `gcl_downscale_pair_mse`.  The objective, the scores and the training loop (`downscale_train.py`, kernels in
`csrc/downscale_loss.hip`) are re-exported from here.  The U-Net's inference is `unet.py`; the loop around it that
`scripts/predict_cascade.py` runs - GNN, crop and upsample, U-Net, scores against the fine truth - is `CascadeRefiner`
and `predict_cascade` at the end of this module (`gcl_cascade_pack`, `gcl_cascade_scores` of `csrc/unet.hip`).
"""
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured
from .data import _upload_fp16
from .downscale_train import (DownscalerMetrics, compute_metrics, downscaler_loss, downscaler_results,  # noqa: F401
                              fit_downscaler, gradient_loss, iter_batches, masked_mse_loss, metrics_table,
                              spectral_loss, train_epoch, validate)
from .interp_tables import TableCache, device_tables
from .verify import regrid_tables, regrid_tables_latlon

# ======================================================================================================================
# Host tables (once per geometry)
# ======================================================================================================================
_TABLES = TableCache()


def roi_crop(g_lats, g_lons, roi, buffer: float = 1.0):
    """`build_downscaler_dataset.py:96-98`: (lat0, lat1, lon0, lon1), the index ranges [lat0, lat1) / [lon0, lon1) of
    the global axes inside the box widened by `buffer` degrees."""
    lat_min, lat_max, lon_min, lon_max = roi
    g_lats, g_lons = np.asarray(g_lats, dtype=np.float64), np.asarray(g_lons, dtype=np.float64)
    lat_idx = np.where((g_lats >= lat_min - buffer) & (g_lats <= lat_max + buffer))[0]
    lon_idx = np.where((g_lons >= lon_min - buffer) & (g_lons <= lon_max + buffer))[0]
    if len(lat_idx) < 2 or len(lon_idx) < 2:
        raise ValueError(f"roi_crop: the box {tuple(roi)} holds {len(lon_idx)} x {len(lat_idx)} global points; the "
                         "interpolation needs at least 2 per axis")
    return int(lat_idx[0]), int(lat_idx[-1]) + 1, int(lon_idx[0]), int(lon_idx[-1]) + 1


def coarse_tables(g_lats, g_lons, r_lats, r_lons, roi, buffer: float = 1.0):
    """(pos int32 [P, 4], w float64 [P, 4]) of `build_downscaler_dataset.py:137-157`: the fine points in the order of
    the lon-first storage (p = j * n_lat_fine + i) on the cropped global grid, corners and weights as
    `verify.regrid_tables` forms them (scipy's interpolator over (lons, lats); a fine point outside the crop is
    extrapolated), positions `lon * n_lat + lat` in the FULL global frame.  Cached; the arrays are read-only."""
    g_lats, g_lons = np.asarray(g_lats, dtype=np.float64), np.asarray(g_lons, dtype=np.float64)
    r_lats, r_lons = np.asarray(r_lats, dtype=np.float64), np.asarray(r_lons, dtype=np.float64)
    roi = tuple(float(v) for v in roi)

    def make():
        la0, la1, lo0, lo1 = roi_crop(g_lats, g_lons, roi, buffer)
        cell, w = regrid_tables(g_lats[la0:la1], g_lons[lo0:lo1], r_lats, r_lons)
        lo, la = cell[:, 0].astype(np.int64) + lo0, cell[:, 1].astype(np.int64) + la0
        n_lat = len(g_lats)
        pos = np.stack([lo * n_lat + la, lo * n_lat + la + 1, (lo + 1) * n_lat + la, (lo + 1) * n_lat + la + 1], axis=1)
        assert pos.min() >= 0 and pos.max() < n_lat * len(g_lons) < 2 ** 31
        return np.ascontiguousarray(pos.astype(np.int32)), np.ascontiguousarray(w)

    key = TableCache.array_key
    return _TABLES.get(("coarse", key(g_lats), key(g_lons), key(r_lats), key(r_lons), roi, float(buffer)), make)


def prediction_tables(grid_lats, grid_lons, roi, target_lats, target_lons, flat_grid: bool = True):
    """(pos int32 [P, 4], w float64 [P, 4]) of `generate_gnn_predictions.py:49-111`: the targets in the order of the
    reference's result (p = i * n_lon + j, latitude-major) on the ROI nodes of the prediction, corners and weights as
    `verify.regrid_tables_latlon` forms them (scipy's interpolator over (lats, lons)), positions = node rows.

    flat_grid: the nodes whose coordinates lie in the box, laid on their unique(lat) x unique(lon) grid (a node listed
    twice: the later row).  A grid with holes raises ValueError; the reference fills holes with a per-channel nanmean,
    which is not provided (its multires and regular node sets leave none).
    not flat_grid: the box widened by 1 degree on a regular grid whose nodes are read as lat * n_lon + lon, the order
    every loader here produces (the reference's reshape at :94 reads lon * n_lat + lat and calls itself approximate)."""
    grid_lats, grid_lons = np.asarray(grid_lats), np.asarray(grid_lons)
    t_lats, t_lons = np.asarray(target_lats, dtype=np.float64), np.asarray(target_lons, dtype=np.float64)
    roi = tuple(float(v) for v in roi)
    if grid_lats.shape != grid_lons.shape or grid_lats.ndim != 1:
        raise ValueError("prediction_tables: grid_lats and grid_lons are one coordinate per node")

    def make():
        lat_min, lat_max, lon_min, lon_max = roi
        if flat_grid:
            mask = (grid_lats >= lat_min) & (grid_lats <= lat_max) & (grid_lons >= lon_min) & (grid_lons <= lon_max)
            rows = np.nonzero(mask)[0]
            u_lats, li = np.unique(grid_lats[rows], return_inverse=True)
            u_lons, lo = np.unique(grid_lons[rows], return_inverse=True)
            node = np.full((len(u_lats), len(u_lons)), -1, dtype=np.int64)
            node[li, lo] = rows  # (ascending rows: a repeated cell keeps the later one)
            holes = int((node < 0).sum())
            if holes:
                raise ValueError(f"prediction_tables: the ROI nodes leave {holes} of the {node.size} cells of their "
                                 f"{len(u_lats)} x {len(u_lons)} grid empty; the nanmean hole fill is not provided")
        else:
            all_lats, all_lons = np.unique(grid_lats), np.unique(grid_lons)
            if len(all_lats) * len(all_lons) != len(grid_lats):
                raise ValueError(f"prediction_tables: {len(grid_lats)} nodes are no {len(all_lats)} x {len(all_lons)} grid")
            u_lats = np.unique(grid_lats[(grid_lats >= lat_min - 1) & (grid_lats <= lat_max + 1)])
            u_lons = np.unique(grid_lons[(grid_lons >= lon_min - 1) & (grid_lons <= lon_max + 1)])
            node = (np.searchsorted(all_lats, u_lats)[:, None].astype(np.int64) * len(all_lons)
                    + np.searchsorted(all_lons, u_lons)[None, :])
        if len(u_lats) < 2 or len(u_lons) < 2:
            raise ValueError(f"prediction_tables: the box {roi} holds {len(u_lats)} x {len(u_lons)} nodes; the "
                             "interpolation needs at least 2 per axis")
        cell, w = regrid_tables_latlon(u_lats, u_lons, t_lats, t_lons)
        la, lo = cell[:, 0].astype(np.int64), cell[:, 1].astype(np.int64)
        pos = np.stack([node[la, lo], node[la, lo + 1], node[la + 1, lo], node[la + 1, lo + 1]], axis=1)
        assert pos.min() >= 0 and pos.max() < len(grid_lats) < 2 ** 31
        return np.ascontiguousarray(pos.astype(np.int32)), np.ascontiguousarray(w)

    key = TableCache.array_key
    return _TABLES.get(("pred", key(grid_lats), key(grid_lons), roi, key(t_lats), key(t_lons), bool(flat_grid)), make)


def _lon_first(pos, w, n_lat: int, n_lon: int):
    """A latitude-major table in the order of the lon-first storage (p = j * n_lat + i)."""
    order = np.arange(n_lat * n_lon).reshape(n_lat, n_lon).T.reshape(-1)
    return np.ascontiguousarray(pos[order]), np.ascontiguousarray(w[order])


# ======================================================================================================================
# The pairs
# ======================================================================================================================
def _open_source(src, device):
    """(series fp16 on the device, info, lats f64, lons f64, scalers {mean, std, n}, variables, label)."""
    if isinstance(src, (str, os.PathLike)):
        d = os.fspath(src)
        with open(os.path.join(d, "dataset_info.json")) as fh:
            info = json.load(fh)
        c = np.load(os.path.join(d, "coords.npz"))
        shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
        series = _upload_fp16(np.memmap(os.path.join(d, "data.npy"), dtype=np.float16, mode="r", shape=shape), device)
        sc = np.load(os.path.join(d, "scalers.npz"))
        scalers = {k: sc[k] for k in sc.files}
        with open(os.path.join(d, "variables.json")) as fh:
            variables = json.load(fh)
        return series, info, c["latitude"].astype(np.float64), c["longitude"].astype(np.float64), scalers, variables, d
    series, info, coords, scalers, variables = src
    if not (series.is_cuda and series.dtype == torch.float16 and series.is_contiguous() and series.dim() == 4):
        raise TypeError("a downscaler source is a directory or (series, info, coords, scalers, variables) with a "
                        "contiguous float16 GPU series (T, lon, lat, C)")
    lats, lons = coords
    return (series, dict(info), np.asarray(lats).astype(np.float64), np.asarray(lons).astype(np.float64), dict(scalers),
            variables, "")


class DownscalerPairs:
    """The (coarse, fine) archives on the device with what the reference keeps next to them.  coarse / fine (and
    gnn_pred, once `GnnPredictionArchive` has made it): fp16 (T, n_lon, n_lat, C); static_fine float32 (n_lon, n_lat,
    Ns) or None; scalers: the global source's arrays as they were; lats / lons: the regional axes in float64."""

    def __init__(self, coarse, fine, static_fine, scalers, lats, lons, info, variables, gnn_pred=None):
        self.coarse, self.fine, self.static_fine, self.gnn_pred = coarse, fine, static_fine, gnn_pred
        self.scalers, self.lats, self.lons, self.info, self.variables = scalers, lats, lons, info, variables

    mean = property(lambda self: self.scalers["mean"])
    std = property(lambda self: self.scalers["std"])
    n = property(lambda self: self.scalers.get("n"))
    device = property(lambda self: self.coarse.device)

    def save(self, out_dir: str) -> str:
        """The reference's seven files: raw coarse.npy / fine.npy, static_fine.npy, scalers.npz, dataset_info.json,
        variables.json and coords.npz (and raw gnn_pred.npy when the archive exists)."""
        os.makedirs(out_dir, exist_ok=True)
        self.coarse.cpu().numpy().tofile(os.path.join(out_dir, "coarse.npy"))
        self.fine.cpu().numpy().tofile(os.path.join(out_dir, "fine.npy"))
        if self.static_fine is not None:
            np.save(os.path.join(out_dir, "static_fine.npy"), self.static_fine.cpu().numpy())
        np.savez(os.path.join(out_dir, "scalers.npz"), **self.scalers)
        with open(os.path.join(out_dir, "dataset_info.json"), "w") as fh:
            json.dump(self.info, fh, indent=2)
        with open(os.path.join(out_dir, "variables.json"), "w") as fh:
            json.dump(self.variables, fh, indent=2)
        np.savez(os.path.join(out_dir, "coords.npz"), latitude=self.lats.astype(np.float32),
                 longitude=self.lons.astype(np.float32))
        if self.gnn_pred is not None:
            self.gnn_pred.cpu().numpy().tofile(os.path.join(out_dir, "gnn_pred.npy"))
        return out_dir

    @classmethod
    def load(cls, data_dir: str, device="cuda:0") -> "DownscalerPairs":
        with open(os.path.join(data_dir, "dataset_info.json")) as fh:
            info = json.load(fh)
        shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
        up = lambda name: _upload_fp16(np.memmap(os.path.join(data_dir, name), dtype=np.float16, mode="r",  # noqa: E731
                                                 shape=shape), device)
        sc = np.load(os.path.join(data_dir, "scalers.npz"))
        c = np.load(os.path.join(data_dir, "coords.npz"))
        static = None
        if os.path.exists(os.path.join(data_dir, "static_fine.npy")):
            static = torch.from_numpy(np.load(os.path.join(data_dir, "static_fine.npy"))).to(device)
        variables = None
        if os.path.exists(os.path.join(data_dir, "variables.json")):
            with open(os.path.join(data_dir, "variables.json")) as fh:
                variables = json.load(fh)
        gnn = up("gnn_pred.npy") if os.path.exists(os.path.join(data_dir, "gnn_pred.npy")) else None
        return cls(up("coarse.npy"), up("fine.npy"), static, {k: sc[k] for k in sc.files},
                   c["latitude"].astype(np.float64), c["longitude"].astype(np.float64), info, variables, gnn)


def build_downscaler_dataset(global_src, region_src, roi, static_channels: Sequence[int] = (7, 8),
                             frames_per_launch: int = 256, device="cuda:0", global_source: Optional[str] = None,
                             region_source: Optional[str] = None) -> DownscalerPairs:
    """`scripts/build_downscaler_dataset.py` on the device.  The sources are dataset directories or (series, info,
    (lats, lons), scalers, variables) with the fp16 series already in HBM.  coarse: the global series cropped to the
    box (+ 1 degree) and interpolated bilinearly onto the regional grid, `frames_per_launch` frames per
    `gcl_downscale_coarse` launch; fine: the regional frames as they are.  global_source / region_source: the strings
    dataset_info.json records (default: the directories given)."""
    g_series, g_info, g_lats, g_lons, g_scalers, g_vars, g_label = _open_source(global_src, device)
    r_series, r_info, r_lats, r_lons, _, _, r_label = _open_source(region_src, device)
    T, C = min(int(g_series.shape[0]), int(r_series.shape[0])), int(g_series.shape[3])
    if C != r_series.shape[3]:
        raise ValueError(f"Feature mismatch: global={C}, region={r_series.shape[3]}")
    if tuple(g_series.shape[1:3]) != (len(g_lons), len(g_lats)) or tuple(r_series.shape[1:3]) != (len(r_lons), len(r_lats)):
        raise ValueError("build_downscaler_dataset: a series does not lie on its axes (lon, lat)")
    if T < 1 or frames_per_launch < 1:
        raise ValueError(f"build_downscaler_dataset: {T} common frames, {frames_per_launch} frames per launch")
    n_lon_f, n_lat_f = len(r_lons), len(r_lats)
    pos, w = device_tables(*coarse_tables(g_lats, g_lons, r_lats, r_lons, roi), g_series.device)
    coarse = torch.empty(T, n_lon_f, n_lat_f, C, dtype=torch.float16, device=g_series.device)
    fine = torch.empty_like(coarse)
    for t0 in range(0, T, frames_per_launch):
        nt = min(frames_per_launch, T - t0)
        hip.downscale_coarse(g_series, pos, w, t0, nt, coarse, t0)
        hip.downscale_coarse(r_series, None, None, t0, nt, fine, t0)
    static_ch = [int(c) for c in static_channels]
    static = r_series[0].float()[:, :, static_ch].contiguous() if static_ch else None
    info = {
        "n_time": T, "n_lon": n_lon_f, "n_lat": n_lat_f, "n_feat": C, "roi": [float(v) for v in roi],
        "global_source": g_label if global_source is None else str(global_source),
        "region_source": r_label if region_source is None else str(region_source),
        "coarse_file": "coarse.npy", "fine_file": "fine.npy", "static_channels": static_ch,
    }
    scalers = {k: g_scalers[k] for k in ("mean", "std", "n")}
    return DownscalerPairs(coarse, fine, static, scalers, r_lats, r_lons, info, g_vars)


# ======================================================================================================================
# GNN predictions on the fine grid
# ======================================================================================================================
def crop_and_upsample_roi(pred_flat, grid_lats, grid_lons, roi, target_lats, target_lons, flat_grid: bool = True):
    """`generate_gnn_predictions.py:49-111` on the device: pred_flat float32 (G, C) -> float32 (n_lat, n_lon, C), the
    float64 interpolation of the ROI nodes rounded once (see `prediction_tables` for the node sets it takes)."""
    if pred_flat.dim() != 2 or pred_flat.shape[0] != len(grid_lats):
        raise ValueError(f"crop_and_upsample_roi: a prediction of shape {tuple(pred_flat.shape)} for {len(grid_lats)} nodes")
    tables = prediction_tables(grid_lats, grid_lons, roi, target_lats, target_lons, flat_grid)  # (host: may raise)
    if not (pred_flat.is_cuda and pred_flat.dtype == torch.float32):
        raise RuntimeError("crop_and_upsample_roi needs a float32 (G, C) GPU tensor (there is no CPU fallback)")
    if pred_flat.stride(1) != 1:
        pred_flat = pred_flat.contiguous()
    G, C = pred_flat.shape
    pos, w = device_tables(*tables, pred_flat.device)
    src = hip.WrfSource(pred_flat, pred_flat.stride(0), G, pos, w)
    out64 = hip.wrf_sample(src, list(range(C)))  # [C, P], P latitude-major
    return out64.to(torch.float32).t().reshape(len(target_lats), len(target_lons), C).contiguous()


class GnnPredictionArchive:
    """`generate_gnn_predictions.py:213-255` in one `gcl_downscale_pred` launch per batch: the model's output (plus
    the last observed frame with use_residual) on the ROI nodes, interpolated to the fine grid, denormalised with the
    GNN's scalers and stored as fp16 in `pairs.gnn_pred[t_pred]` (zero where nothing was predicted, as the memmap)."""

    def __init__(self, model, pairs: DownscalerPairs, grid_lats, grid_lons, roi, mean, std, obs: int, C: int,
                 flat_grid: bool = True, use_residual: bool = False):
        self.model, self.pairs, self.obs, self.C, self.use_residual = model, pairs, int(obs), int(C), bool(use_residual)
        if pairs.coarse.shape[3] != self.C:
            raise ValueError(f"GnnPredictionArchive: {self.C} features for an archive of {pairs.coarse.shape[3]}")
        dev = pairs.device
        n_lon, n_lat = pairs.coarse.shape[1:3]
        self.n_nodes = len(grid_lats)
        # (the targets are the axes as coords.npz holds them: float32, widened - what the reference's script reads)
        t_lats, t_lons = (np.asarray(a).astype(np.float32).astype(np.float64) for a in (pairs.lats, pairs.lons))
        pos, w = prediction_tables(grid_lats, grid_lons, roi, t_lats, t_lons, flat_grid)
        self.pos, self.w = device_tables(*_lon_first(pos, w, n_lat, n_lon), dev)
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)[:self.C].copy()).to(dev)  # noqa: E731
        self.mean, self.std = f32(mean), f32(std)
        if pairs.gnn_pred is None:
            pairs.gnn_pred = torch.zeros_like(pairs.coarse)

    def update(self, X, t_pred):
        """X float32 [B, G, obs * C] on the device; t_pred: the destination frames (int64 [B] on the device, or host
        ints); a frame outside the archive is skipped."""
        B, G, F = X.shape
        if G != self.n_nodes or F != self.obs * self.C:
            raise ValueError(f"GnnPredictionArchive: a batch of {tuple(X.shape)} for {self.n_nodes} nodes, "
                             f"{self.obs} x {self.C} features")
        if not isinstance(t_pred, torch.Tensor):
            t_pred = torch.tensor([int(t) for t in t_pred], dtype=torch.int64).to(X.device)
        with torch.no_grad():
            pred = self.model(X=X, attention_threshold=0.0)
        if pred.dim() == 2:
            pred = pred.unsqueeze(0)
        if pred.stride(2) != 1:
            pred = pred.contiguous()
        last = X[:, :, (self.obs - 1) * self.C:] if self.use_residual else None
        hip.downscale_pred(pred.detach(), self.pos, self.w, self.std, self.mean, t_pred, self.pairs.gnn_pred, last3=last)
        return self.pairs.gnn_pred

    def save(self, out_dir: str) -> str:
        path = os.path.join(out_dir, "gnn_pred.npy")
        self.pairs.gnn_pred.cpu().numpy().tofile(path)
        return path


class CapturedGnnPredictions(GnnPredictionArchive, Captured):
    """`GnnPredictionArchive` with model and `gcl_downscale_pred` replayed from one hipGraph per batch shape."""

    def __init__(self, *args, use_graph: bool = True, required: bool = False, **kw):
        GnnPredictionArchive.__init__(self, *args, **kw)
        Captured.__init__(self, use_graph=use_graph, required=required)

    def _work(self, X, t_pred):
        return GnnPredictionArchive.update(self, X, t_pred)

    def update(self, X, t_pred):
        if not isinstance(t_pred, torch.Tensor):
            t_pred = torch.tensor([int(t) for t in t_pred], dtype=torch.int64).to(X.device)
        return self._run(X, t_pred)


def generate_gnn_predictions(model, datasets, pairs: DownscalerPairs, grid_lats, grid_lons, roi, mean, std, obs: int,
                             C: int, flat_grid: bool = True, use_residual: bool = False, subsample: int = 1,
                             batch_size: int = 8, archive: Optional[GnnPredictionArchive] = None) -> int:
    """The loop of `generate_gnn_predictions.py:208-255` over `batch()`-style data sets (train, val, test): every
    `subsample`-th sample i of a set goes to frame t_pred = local_t + obs of its `_sample_indices` entry (chunk-local,
    as the reference takes it), else obs + i.  Returns how many predictions landed inside the archive."""
    if archive is None:
        archive = GnnPredictionArchive(model, pairs, grid_lats, grid_lons, roi, mean, std, obs, C, flat_grid, use_residual)
    T, total = int(pairs.coarse.shape[0]), 0
    for ds in datasets:
        picks = list(range(0, len(ds), max(1, int(subsample))))
        si = getattr(ds, "_sample_indices", None)
        t_pred = [si[i][1] + obs if si is not None and i < len(si) else obs + i for i in picks]
        for a in range(0, len(picks), batch_size):
            X, _ = ds.batch(picks[a:a + batch_size])
            archive.update(X, t_pred[a:a + batch_size])
        total += sum(1 for t in t_pred if t < T)
    return total


# ======================================================================================================================
# Batches and the coarse baseline
# ======================================================================================================================
class DownscalerDataset:
    """`DownscalerDataset` of `scripts/train_downscaler.py:49-183` over archives on the device.  `ds[i]` returns
    (X [obs * C + Ns, H, W], Y [C, H, W]) float32 like the reference's `__getitem__` without its random draws;
    `ds.batch(indices, flip, noise)` a whole batch from one `gcl_downscale_batch` launch, the caller supplying the
    draws: flip one truth value per sample (used when augment_flip holds for this split), noise standard normals
    [B, obs * C, H, W] scaled by input_noise (train split only)."""

    def __init__(self, pairs_or_dir, obs_window: int = 2, split: str = "train", static_context: bool = True,
                 use_gnn_input: bool = False, augment_flip: bool = False, input_noise: float = 0.0,
                 wind_u_channels: Sequence[int] = (), device="cuda:0"):
        pairs = pairs_or_dir if isinstance(pairs_or_dir, DownscalerPairs) else DownscalerPairs.load(pairs_or_dir, device)
        self.pairs, self.obs_window, self.split = pairs, int(obs_window), split
        self.T, self.n_lon, self.n_lat, self.C = (int(v) for v in pairs.coarse.shape)
        self.static_channels = pairs.info.get("static_channels", [])
        self.augment_flip = augment_flip and split == "train"
        self.input_noise = float(input_noise) if split == "train" else 0.0
        self.wind_u_channels = tuple(int(c) for c in wind_u_channels)
        if use_gnn_input:
            if pairs.gnn_pred is None:
                raise FileNotFoundError("gnn_pred is missing: run generate_gnn_predictions first.")
            self.coarse = pairs.gnn_pred
        else:
            self.coarse = pairs.coarse
        self.fine = pairs.fine
        dev = self.coarse.device
        self.mean_np, self.std_np = pairs.mean.astype(np.float32), pairs.std.astype(np.float32)
        if len(self.mean_np) != self.C or len(self.std_np) != self.C:
            raise ValueError(f"DownscalerDataset: scalers of {len(self.mean_np)} channels for {self.C}")
        self.mean, self.std = torch.from_numpy(self.mean_np.copy()).to(dev), torch.from_numpy(self.std_np.copy()).to(dev)
        self.static_fine = pairs.static_fine.float().contiguous() if static_context and pairs.static_fine is not None else None
        neg = np.zeros(self.C, dtype=np.int32)
        neg[list(self.wind_u_channels)] = 1
        self._neg = torch.from_numpy(neg).to(dev)

        valid_indices = list(range(self.obs_window - 1, self.T))  # chronological, :111-125
        n = len(valid_indices)
        n_test = int(n * 0.2)
        n_val = n_test // 2
        n_train = n - n_test
        if split == "train":
            self.indices = valid_indices[:n_train]
        elif split == "val":
            self.indices = valid_indices[n_train:n_train + n_val]
        elif split == "test":
            self.indices = valid_indices[n_train + n_val:]
        else:
            self.indices = valid_indices

    def __len__(self):
        return len(self.indices)

    def frames(self, indices) -> torch.Tensor:
        """The archive frames t of the samples, int64 on the device."""
        return torch.tensor([self.indices[int(i)] for i in indices], dtype=torch.int64).to(self.coarse.device)

    def batch(self, indices, flip=None, noise=None, out=None):
        t = self.frames(indices)
        dev = t.device
        fl = None
        if flip is not None and self.augment_flip:
            fl = torch.as_tensor(flip).to(device=dev, dtype=torch.int32).contiguous()
        if noise is not None and self.input_noise <= 0:
            noise = None
        return hip.downscale_batch(self.coarse, self.fine, t, self.obs_window, self.mean, self.std, static=self.static_fine,
                                   flip=fl, neg=self._neg if fl is not None else None, noise=noise,
                                   sigma=self.input_noise, out=out)

    def __getitem__(self, idx):
        X, Y = self.batch([idx])
        return X[0], Y[0]


def coarse_baseline(ds: DownscalerDataset, channel_names: Optional[Sequence[str]] = None):
    """The `rmse_coarse` column of `compute_metrics` (`train_downscaler.py:288-305`) over every sample of `ds`: per
    channel sqrt(sum d^2 / n) * std in physical units, d the normalised difference of the last input frame and the
    target, from one `gcl_downscale_pair_mse` launch (the reference averages per-batch means, which is the same number
    when its batches are equal in size).  float64 [C], or {name: value} with channel_names."""
    if len(ds) == 0:
        raise ValueError("coarse_baseline: the data set is empty")
    stats = hip.downscale_pair_mse(ds.coarse, ds.fine, ds.frames(range(len(ds))), ds.mean, ds.std).cpu().numpy()
    rmse = np.sqrt(stats[:, 1] / stats[:, 0]) * ds.std_np.astype(np.float64)
    if channel_names is None:
        return rmse
    if len(channel_names) != len(rmse):
        raise ValueError(f"coarse_baseline: {len(channel_names)} names for {len(rmse)} channels")
    return {name: float(v) for name, v in zip(channel_names, rmse)}


# ======================================================================================================================
# The cascade: GNN -> crop and upsample -> U-Net, scored against the fine truth (scripts/predict_cascade.py)
# ======================================================================================================================
class CascadeRefiner:
    """The per-step refinement and scores of `predict_cascade.py:338-372` for B samples at a time.

    `refine(coarse)`: coarse float32 [B, H, W, C] in the GNN's normalised space (the ROI output on the fine grid) ->
    (cascade_out [B, C, H, W], coarse_phys [B, H, W, C]): `gcl_cascade_pack`, then the network (`unet.WeatherUNet`, with
    the x_last add fused when `residual`).  `score(step, cascade_out, coarse_phys, t_fine, t_persist)` adds the step's
    per-channel mean squared errors of GNN, cascade and persistence into the float64 device state (`gcl_cascade_scores`);
    `results()` is the one host read."""

    def __init__(self, unet, pairs_or_dir, gnn_mean, gnn_std, obs_window: int = 2, residual: bool = False,
                 ar_steps: int = 4, device="cuda:0"):
        pairs = pairs_or_dir if isinstance(pairs_or_dir, DownscalerPairs) else DownscalerPairs.load(pairs_or_dir, device)
        self.unet, self.pairs, self.obs_window, self.residual = unet, pairs, int(obs_window), bool(residual)
        self.T, self.W, self.H, self.C = (int(v) for v in pairs.fine.shape)
        dev = pairs.device
        f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)[:self.C].copy()).to(dev)  # noqa: E731
        self.gnn_mean, self.gnn_std, self.ds_mean, self.ds_std = f32(gnn_mean), f32(gnn_std), f32(pairs.mean), f32(pairs.std)
        for v in (self.gnn_mean, self.gnn_std, self.ds_mean, self.ds_std):
            if v.numel() != self.C:
                raise ValueError(f"CascadeRefiner: scalers of {v.numel()} channels for {self.C}")
        self.static_fine = pairs.static_fine.float().contiguous() if pairs.static_fine is not None else None
        ns = 0 if self.static_fine is None else int(self.static_fine.shape[2])
        want = self.obs_window * self.C + ns
        if getattr(unet, "in_channels", want) != want or getattr(unet, "out_channels", self.C) != self.C:
            raise ValueError(f"CascadeRefiner: the network maps {unet.in_channels} to {unet.out_channels} channels, the "
                             f"cascade feeds {want} and scores {self.C}")
        self.reset(ar_steps)

    def reset(self, ar_steps: int):
        dev = self.pairs.device
        self.state = torch.zeros(int(ar_steps), self.C, 3, dtype=torch.float64, device=dev)
        self.count = torch.zeros(int(ar_steps), dtype=torch.int64, device=dev)

    def refine(self, coarse):
        if coarse.dim() != 4 or tuple(coarse.shape[1:]) != (self.H, self.W, self.C):
            raise ValueError(f"CascadeRefiner: coarse [B, {self.H}, {self.W}, {self.C}] expected, got {tuple(coarse.shape)}")
        coarse_phys, X = hip.cascade_pack(coarse.contiguous(), self.gnn_mean, self.gnn_std, self.ds_mean, self.ds_std,
                                          self.static_fine, self.obs_window)
        rf = ((self.obs_window - 1) * self.C, self.obs_window * self.C) if self.residual else None
        return self.unet(X, residual_from=rf), coarse_phys

    def score(self, step: int, cascade_out, coarse_phys, t_fine, t_persist):
        """t_fine / t_persist: int64 [B] (device tensors or host ints); a frame outside the archive skips its sample."""
        dev = self.pairs.device
        as_dev = lambda t: (t if isinstance(t, torch.Tensor) else torch.tensor([int(v) for v in t], dtype=torch.int64)).to(dev)  # noqa: E731
        hip.cascade_scores(cascade_out, coarse_phys, self.pairs.fine, as_dev(t_fine), as_dev(t_persist), self.ds_mean,
                           self.ds_std, self.state, self.count, step)

    def results(self):
        """The dictionary `predict_cascade.py:481-494` writes: per horizon n_samples and, per dynamic channel,
        rmse_persist / rmse_gnn / rmse_cascade."""
        state, count = self.state.cpu().numpy(), self.count.cpu().numpy()
        static = set(self.pairs.info.get("static_channels", []))
        names = self.pairs.variables if self.pairs.variables else [f"ch{i}" for i in range(self.C)]
        out = {}
        for s in range(state.shape[0]):
            rmse = np.sqrt(state[s] / count[s]) if count[s] > 0 else np.zeros_like(state[s])
            out[f"+{(s + 1) * 6}h"] = {
                "n_samples": int(count[s]),
                "per_channel": {names[c]: {"rmse_persist": float(rmse[c, 2]), "rmse_gnn": float(rmse[c, 0]),
                                           "rmse_cascade": float(rmse[c, 1])}
                                for c in range(self.C) if c not in static}}
        return out


def predict_cascade(gnn_model, unet, test_dataset, pairs_or_dir, grid_lats, grid_lons, roi, gnn_mean, gnn_std,
                    ar_steps: int = 4, max_samples: int = 50, batch_size: int = 8, use_residual: bool = False,
                    unet_residual: bool = False, flat_grid: bool = True, obs_window: int = 2, refiner=None):
    """The loop of `predict_cascade.py:292-372` over a `batch(indices)`-style data set, `batch_size` samples at a time.

    Sample i sits at local_t = its `_sample_indices` entry's (else i); persistence is the fine frame t_persist =
    local_t + obs - 1 (a sample whose t_persist is outside the archive is left out altogether), the target of step s the
    frame t_fine = local_t + obs + s (a sample whose t_fine runs past the archive is skipped from that step on).  Each
    step runs the GNN, puts its ROI output on the fine grid through `prediction_tables` (all samples and channels in one
    launch), refines it (`CascadeRefiner.refine`) and scores it on the device; there is one host read, at the end.  The
    result does not depend on batch_size.  Returns the dictionary of `cascade_results.json`."""
    if refiner is None:
        refiner = CascadeRefiner(unet, pairs_or_dir, gnn_mean, gnn_std, obs_window, unet_residual, ar_steps)
    else:
        refiner.reset(ar_steps)
    pairs, C, T = refiner.pairs, refiner.C, refiner.T
    dev = pairs.device
    t_lats, t_lons = (np.asarray(a).astype(np.float32).astype(np.float64) for a in (pairs.lats, pairs.lons))
    pos, w = device_tables(*prediction_tables(grid_lats, grid_lons, roi, t_lats, t_lons, flat_grid), dev)
    n = min(int(max_samples), len(test_dataset))
    si = getattr(test_dataset, "_sample_indices", None)
    local_t = [int(si[i][1]) if si is not None and i < len(si) else i for i in range(n)]
    obs = None
    for a in range(0, n, max(1, int(batch_size))):
        idx = list(range(a, min(n, a + batch_size)))
        X, _ = test_dataset.batch(idx)
        B, G, F = X.shape
        obs = F // C
        keep = [k for k, i in enumerate(idx) if local_t[i] + obs - 1 < T]  # :308-310
        if not keep:
            continue
        if len(keep) < B:
            X = X[torch.tensor(keep, device=X.device)]
        lt = [local_t[idx[k]] for k in keep]
        B = len(keep)
        t_persist = torch.tensor([t + obs - 1 for t in lt], dtype=torch.int64).to(dev)
        curr = X.view(B, G, obs, C)
        offs = [b * G * C + c for b in range(B) for c in range(C)]
        offs_dev = torch.tensor(offs, dtype=torch.int64).to(dev)
        for step in range(int(ar_steps)):
            tf = [t + obs + step if t + obs + step < T else -1 for t in lt]  # :330-333: the sample ends here
            if all(t < 0 for t in tf):
                break
            with torch.no_grad():
                pred = gnn_model(X=curr.reshape(B, G, obs * C), attention_threshold=0.0)
            if pred.dim() == 2:
                pred = pred.unsqueeze(0)
            out = (curr[:, :, -1, :] + pred if use_residual else pred).detach().contiguous()
            curr = torch.cat([curr[:, :, 1:, :], out.unsqueeze(2)], dim=2)
            # the ROI nodes on the fine grid, float64 interpolation rounded once: [B * C, P], P latitude-major
            fine64 = hip.wrf_sample(hip.WrfSource(out, C, G, pos, w), offs, field_off_dev=offs_dev)
            coarse = fine64.to(torch.float32).view(B, C, refiner.H, refiner.W).permute(0, 2, 3, 1).contiguous()
            cascade_out, coarse_phys = refiner.refine(coarse)
            refiner.score(step, cascade_out, coarse_phys, torch.tensor(tf, dtype=torch.int64).to(dev), t_persist)
    return refiner.results()


def save_cascade_results(results, ds_dir: str) -> str:
    """`cascade_results.json` in the downscaler's experiment directory (predict_cascade.py:495-497)."""
    path = os.path.join(ds_dir, "cascade_results.json")
    with open(path, "w") as fh:
        json.dump(results, fh, indent=2)
    return path
