"""Multi-resolution input on the fly: the flat node set of the reference's `multires_*` / `region_*` experiments
(the global grid with the points inside a lat/lon box removed, a fine regional grid in their place) built per batch
from the series that are already in HBM.

The reference writes that node set to disk first (`scripts/build_multires_dataset.py`: per frame and channel a scipy
`RegularGridInterpolator` on the host, and a second full copy of the data) or builds frames per sample in numpy
(`scripts/evaluate_full_pipeline.py:113-144`).  Here `MultiresChunkDataset.batch` is one `gcl_multires_window_pack`
launch over the global (and, in merge mode, regional) fp16 series; `write_multires_dataset` produces the reference's
files from the same kernel for those who still want them.
"""
import json
import os
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip
from .data import _upload_fp16, sample_indices
from .verify import regrid_tables_latlon


# ======================================================================================================================
# Node mappings (host, once per geometry)
# ======================================================================================================================
def build_node_mapping(g_lats, g_lons, r_lats, r_lons, roi):
    """`scripts/build_multires_dataset.py:94-148`: (flat_lats f32, flat_lons f32, global_mask, region_mask,
    keep_global [n_lat, n_lon]).  The kept global points come first in (lat, lon)-major order, then every regional
    point in the same order; the coordinates are concatenated in their input dtype and rounded to float32 once."""
    lat_min, lat_max, lon_min, lon_max = roi
    g_lon_mesh, g_lat_mesh = np.meshgrid(g_lons, g_lats)
    keep_global = ~((g_lat_mesh >= lat_min) & (g_lat_mesh <= lat_max) & (g_lon_mesh >= lon_min) & (g_lon_mesh <= lon_max))
    g_flat_lats, g_flat_lons = g_lat_mesh[keep_global], g_lon_mesh[keep_global]
    n_kept = g_flat_lats.shape[0]
    r_lon_mesh, r_lat_mesh = np.meshgrid(r_lons, r_lats)
    flat_lats = np.concatenate([g_flat_lats, r_lat_mesh.reshape(-1)]).astype(np.float32)
    flat_lons = np.concatenate([g_flat_lons, r_lon_mesh.reshape(-1)]).astype(np.float32)
    global_mask = np.zeros(len(flat_lats), dtype=bool)
    global_mask[:n_kept] = True
    region_mask = np.zeros(len(flat_lats), dtype=bool)
    region_mask[n_kept:] = True
    return flat_lats, flat_lons, global_mask, region_mask, keep_global


def build_multires_coords(g_lats, g_lons, r_lats, r_lons, roi):
    """`scripts/evaluate_full_pipeline.py:87-110`: (flat_lats, flat_lons, region_mask, keep_global, n_global_kept).
    Same node order as `build_node_mapping`, but the meshgrid is built with indexing="ij" and every part is rounded to
    float32 before the concatenation."""
    lat_min, lat_max, lon_min, lon_max = roi
    g_lat_mesh, g_lon_mesh = np.meshgrid(g_lats, g_lons, indexing="ij")
    keep_global = ~((g_lat_mesh >= lat_min) & (g_lat_mesh <= lat_max) & (g_lon_mesh >= lon_min) & (g_lon_mesh <= lon_max))
    g_flat_lats = g_lat_mesh[keep_global].astype(np.float32)
    g_flat_lons = g_lon_mesh[keep_global].astype(np.float32)
    r_lon_mesh, r_lat_mesh = np.meshgrid(r_lons, r_lats)
    flat_lats = np.concatenate([g_flat_lats, r_lat_mesh.reshape(-1).astype(np.float32)])
    flat_lons = np.concatenate([g_flat_lons, r_lon_mesh.reshape(-1).astype(np.float32)])
    n_global_kept = len(g_flat_lats)
    region_mask = np.zeros(len(flat_lats), dtype=bool)
    region_mask[n_global_kept:] = True
    return flat_lats, flat_lons, region_mask, keep_global, n_global_kept


def rank_table(keep_global: np.ndarray) -> np.ndarray:
    """int32 [n_lat * n_lon], (lat, lon)-major: the output row of every global point, -1 for a removed one."""
    keep = np.asarray(keep_global, dtype=bool).reshape(-1)
    rank = np.full(keep.shape, -1, dtype=np.int32)
    rank[keep] = np.arange(int(keep.sum()), dtype=np.int32)
    return rank


def interpolation_tables(g_lats, g_lons, r_lats, r_lons) -> Tuple[np.ndarray, np.ndarray]:
    """Corner positions int32 [n_reg, 4] (lon * n_lat + lat, the layout of a (lon, lat, C) frame) and float64 weights
    [n_reg, 4] of the regional points, in the corner order of `verify.regrid_tables_latlon`."""
    cell, w = regrid_tables_latlon(g_lats, g_lons, r_lats, r_lons)
    n_lat = len(g_lats)
    la, lo = cell[:, 0].astype(np.int64), cell[:, 1].astype(np.int64)
    corner = np.stack([lo * n_lat + la, (lo + 1) * n_lat + la, lo * n_lat + la + 1, (lo + 1) * n_lat + la + 1], axis=1)
    assert corner.min() >= 0 and corner.max() < n_lat * len(g_lons)
    return np.ascontiguousarray(corner.astype(np.int32)), np.ascontiguousarray(w)


# ======================================================================================================================
# Datasets on disk (the reference's layout: raw fp16 data.npy + dataset_info.json + coords.npz + scalers.npz)
# ======================================================================================================================
def _load_info(data_dir: str) -> dict:
    with open(os.path.join(data_dir, "dataset_info.json")) as fh:
        return json.load(fh)


def _load_coords(path: str) -> Tuple[np.ndarray, np.ndarray]:
    c = np.load(path if path.endswith(".npz") else os.path.join(path, "coords.npz"))
    return c["latitude"].astype(np.float64), c["longitude"].astype(np.float64)


def _open_series(data_dir: str, info: dict) -> np.memmap:
    shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
    return np.memmap(os.path.join(data_dir, "data.npy"), dtype=np.float16, mode="r", shape=shape)


class MultiresChunkDataset:
    """`data.TimeseriesChunkDataset` over the multires node set, with nothing multires ever stored.

    global_dir: the global dataset (series (T, lon, lat, C) fp16).  region: in `mode="merge"` the regional dataset
    directory (its series fills the regional rows, `build_merge_mode` / `build_multires_frame(regional_data=...)`); in
    `mode="interpolate"` a directory or `coords.npz` that gives the regional axes (the rows are the bilinear
    interpolation of the global frame, `build_interpolate_mode`).  roi = (lat_min, lat_max, lon_min, lon_max).

    quantize=True gives what "build the dataset, then load it" gives: an interpolated value is rounded float64 ->
    float32 -> float16 -> float32 before the z-score.  quantize=False keeps the float32 value, as the on-the-fly frames
    of `scripts/evaluate_full_pipeline.py:452-468` do.  (Merge-mode rows are fp16 values either way.)

    `ds[i]`, `len(ds)`, `ds.batch(indices, out=None)`, `grid_nodes` and `flat_grid` are those of
    `TimeseriesChunkDataset`; `coordinates` = (flat_lats, flat_lons) and `is_regional` describe the node set."""

    flat_grid = True

    def __init__(self, global_dir: str, region: str, roi, mode: str = "interpolate", obs_window: int = 2,
                 pred_steps: int = 1, split: str = "train", n_features: Optional[int] = None,
                 test_fraction: float = 0.2, device="cuda:0", time_offset_global: int = 0, time_offset_region: int = 0,
                 quantize: bool = True):
        if mode not in ("merge", "interpolate"):
            raise ValueError(f"Unknown mode: {mode}")
        self.global_dir, self.region, self.roi, self.mode = str(global_dir), str(region), tuple(roi), mode
        self.obs_window, self.pred_steps, self.split = obs_window, pred_steps, split
        self.test_fraction, self.device, self.quantize = test_fraction, torch.device(device), bool(quantize)
        self.time_offset_global, self.time_offset_region = int(time_offset_global), int(time_offset_region)

        self.global_info = _load_info(self.global_dir)
        self.g_lats, self.g_lons = _load_coords(self.global_dir)
        g_host = _open_series(self.global_dir, self.global_info)
        Tg, n_lon, n_lat, Ct = g_host.shape
        if (n_lat, n_lon) != (len(self.g_lats), len(self.g_lons)):
            raise ValueError(f"global series is {n_lon} x {n_lat}, its coords.npz gives {len(self.g_lons)} x {len(self.g_lats)}")
        self.r_lats, self.r_lons = _load_coords(self.region)
        self.n_lon, self.n_lat, self.n_feat_total = n_lon, n_lat, Ct

        (self.flat_lats, self.flat_lons, self.global_mask, self.is_regional,
         self.keep_global) = build_node_mapping(self.g_lats, self.g_lons, self.r_lats, self.r_lons, self.roi)
        self.n_global_kept, self.n_regional = int(self.global_mask.sum()), int(self.is_regional.sum())
        self.n_nodes = self.n_global_kept + self.n_regional
        self.coordinates = (self.flat_lats, self.flat_lons)

        scalers = np.load(os.path.join(self.global_dir, "scalers.npz"))
        self.n_feat = n_features if n_features else Ct
        self.mean_np = scalers["mean"].astype(np.float32)[:self.n_feat]
        self.std_np = scalers["std"].astype(np.float32)[:self.n_feat]
        self.mean = torch.from_numpy(self.mean_np.copy()).to(self.device)
        self.std = torch.from_numpy(self.std_np.copy()).to(self.device)

        self.series = _upload_fp16(g_host, self.device)
        self.rank = torch.from_numpy(rank_table(self.keep_global)).to(self.device)
        self.region_series = self.corner = self.weights = None
        if mode == "merge":
            self.region_info = _load_info(self.region)
            r_host = _open_series(self.region, self.region_info)
            if r_host.shape[1:3] != (len(self.r_lons), len(self.r_lats)) or r_host.shape[3] != Ct:
                raise ValueError(f"regional series {r_host.shape[1:]} does not match its axes / the {Ct} global features")
            self.region_series = _upload_fp16(r_host, self.device)
            self.total_time = min(Tg - self.time_offset_global, r_host.shape[0] - self.time_offset_region)
        else:
            corner, w = interpolation_tables(self.g_lats, self.g_lons, self.r_lats, self.r_lons)
            self.corner, self.weights = torch.from_numpy(corner).to(self.device), torch.from_numpy(w).to(self.device)
            self.total_time = Tg - self.time_offset_global
        self.chunk_lengths = [self.total_time]
        self._sample_indices = sample_indices(self.chunk_lengths, obs_window, pred_steps, split, test_fraction)
        print(f"[MultiresDataset] {split}: {len(self._sample_indices)} samples, mode={mode}, flat_nodes={self.n_nodes} "
              f"({self.n_global_kept} global + {self.n_regional} regional), feat={self.n_feat}, obs={obs_window}, "
              f"pred={pred_steps}")

    def __len__(self):
        return len(self._sample_indices)

    @property
    def grid_nodes(self) -> int:
        return self.n_nodes

    def windows(self, t0: torch.Tensor, obs: int, pred: int, C: int, zscore: bool = True, out=None, out_f16=False):
        """The windows starting at the frames t0 (int64 [B], on the device): one launch."""
        return hip.multires_window_pack(
            self.series, self.region_series, self.rank, self.n_global_kept, self.n_regional, self.corner, self.weights,
            t0, self.time_offset_global, self.time_offset_region, self.mean if zscore else None,
            self.std if zscore else None, C, obs, pred, quantize=self.quantize, out=out, out_f16=out_f16)

    def batch(self, indices: Sequence[int], out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """`[B, N, obs*C]`, `[B, N, pred*C]` for the samples `indices`; out = (X, Y) fills those buffers in place
        (e.g. `TrainStep.input_buffers()`)."""
        t0 = torch.tensor([self._sample_indices[int(i)][1] for i in indices], dtype=torch.int64).to(self.device)
        return self.windows(t0, self.obs_window, self.pred_steps, self.n_feat, out=out)

    def __getitem__(self, idx):
        X, Y = self.batch([idx])
        return X[0], Y[0]


def write_multires_dataset(ds: MultiresChunkDataset, out_dir: str, frames_per_launch: int = 256) -> str:
    """Write `ds` in the on-disk format of `scripts/build_multires_dataset.py` (`data.npy` raw fp16 (T, N, C) with
    every stored feature, `coords.npz`, `dataset_info.json`, `scalers.npz`, `variables.json`).  The frames come from
    the kernel that serves `batch`, with the z-score off and fp16 output."""
    os.makedirs(out_dir, exist_ok=True)
    np.savez(os.path.join(out_dir, "coords.npz"), latitude=ds.flat_lats, longitude=ds.flat_lons, is_regional=ds.is_regional)
    T, N, C = ds.total_time, ds.n_nodes, ds.n_feat_total
    out = np.memmap(os.path.join(out_dir, "data.npy"), dtype=np.float16, mode="w+", shape=(T, N, C))
    for t in range(0, T, frames_per_launch):
        t0 = torch.arange(t, min(t + frames_per_launch, T), dtype=torch.int64, device=ds.device)
        X, _ = ds.windows(t0, 1, 0, C, zscore=False, out_f16=True)
        out[t:t + t0.numel()] = X.cpu().numpy()
    out.flush()
    del out

    with open(os.path.join(ds.global_dir, "variables.json")) as fh:
        variables = json.load(fh)
    g = ds.global_info
    merge = ds.mode == "merge"
    info = {
        "time_start": g.get("time_start", "") if merge else g["time_start"],
        "time_end": g.get("time_end", "") if merge else g["time_end"],
        "n_time": T, "n_nodes": N, "n_feat": C, "flat": True,
        "n_global_kept": ds.n_global_kept, "n_regional": ds.n_regional, "roi": list(ds.roi), "variables": variables,
        "dtype": "float16", "file": "data.npy", "source_global": ds.global_dir,
        ("source_region" if merge else "source_region_coords"): ds.region, "mode": ds.mode,
    }
    with open(os.path.join(out_dir, "dataset_info.json"), "w") as fh:
        json.dump(info, fh, indent=2, ensure_ascii=False)
    np.savez(os.path.join(out_dir, "scalers.npz"), **dict(np.load(os.path.join(ds.global_dir, "scalers.npz"))))
    with open(os.path.join(out_dir, "variables.json"), "w") as fh:
        json.dump(variables, fh)
    return out_dir
