"""Device-resident input pipeline: the reference's on-the-fly window loader, done on the GPU.

Mirrors `TimeseriesChunkDataset` of `src/data/dataloader_chunked.py:33-223`: the raw fp16 time series
(`data.npy` + `dataset_info.json`, or `chunk_*.npy`) is uploaded ONCE and stays in HBM as fp16 (the
81 GB of `wb2_512x256_19f_ar` fit beside the model in 288 GB); a batch of windows is then one
`gcl_window_pack` launch (dequantise, z-score, (lat, lon)-major transpose) instead of a host-side
numpy pass per sample plus an H2D copy of fp32 windows.  Sample indexing and the train / val / test
splits follow the reference (`:132-172`), windows never cross a chunk boundary.

Also here: the legacy tensor datasets of `src/data/dataloader.py` (`WeatherDataset`, `load_train_and_test_datasets`:
the stored tensors stay in HBM, a batch is one `gcl_tensor_batch_pack` launch), the dataset table of
`src/data/data_configs.py`, `load_chunked_datasets` (one upload shared by the three splits) and `DeviceLoader`, which
turns any of these datasets into the (X, y) batch iterable `train.train` takes.
"""
import glob
import json
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip


def _upload_fp16(mm: np.ndarray, device, slab_bytes: int = 1 << 30) -> torch.Tensor:
    """Stream a (memory-mapped) fp16 array to the GPU in slabs, so the host never holds it whole."""
    if mm.dtype != np.float16:
        raise TypeError(f"time series must be float16 on disk, got {mm.dtype}")
    out = torch.empty(mm.shape, dtype=torch.float16, device=device)
    per_t = max(1, int(np.prod(mm.shape[1:])) * 2)
    step = max(1, slab_bytes // per_t)
    for t in range(0, mm.shape[0], step):
        out[t:t + step].copy_(torch.from_numpy(np.array(mm[t:t + step])), non_blocking=False)
    return out


class TimeseriesChunkDataset:
    """`src/data/dataloader_chunked.py:33-223` with the series resident on `device`.

    `ds[i]` returns `(X [G, obs*C], Y [G, pred*C])` like the reference's `__getitem__` (on the GPU);
    `ds.batch(indices)` returns `[B, G, ...]` tensors from one kernel launch per chunk touched."""

    def __init__(self, data_dir: str, obs_window: int = 2, pred_steps: int = 1, split: str = "train",
                 n_features: Optional[int] = None, test_fraction: float = 0.2, device="cuda:0"):
        self.data_dir, self.obs_window, self.pred_steps = data_dir, obs_window, pred_steps
        self.split, self.test_fraction, self.device = split, test_fraction, torch.device(device)
        scalers = np.load(os.path.join(data_dir, "scalers.npz"))
        mean, std = scalers["mean"].astype(np.float32), scalers["std"].astype(np.float32)

        single, info_file = os.path.join(data_dir, "data.npy"), os.path.join(data_dir, "dataset_info.json")
        if os.path.exists(single) and os.path.exists(info_file):  # raw memmap without an .npy header (:79-96)
            with open(info_file) as fh:
                info = json.load(fh)
            self.flat_grid = bool(info.get("flat", False))
            shape = ((info["n_time"], info["n_nodes"], info["n_feat"]) if self.flat_grid
                     else (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"]))
            host_chunks = [np.memmap(single, dtype=np.float16, mode="r", shape=shape)]
        else:
            self.flat_grid = False
            files = sorted(glob.glob(os.path.join(data_dir, "chunk_*.npy")))
            if not files:
                raise FileNotFoundError(f"No data.npy or chunk_*.npy found in {data_dir}")
            host_chunks = [np.load(f, mmap_mode="r") for f in files]
        self.chunk_lengths = [int(c.shape[0]) for c in host_chunks]
        self.total_time = sum(self.chunk_lengths)
        c0 = host_chunks[0]
        if self.flat_grid:
            self.n_nodes, self.n_lon, self.n_lat, self.n_feat_total = int(c0.shape[1]), None, None, int(c0.shape[2])
        else:
            self.n_nodes, self.n_lon, self.n_lat, self.n_feat_total = None, int(c0.shape[1]), int(c0.shape[2]), int(c0.shape[3])
        self.n_feat = n_features if n_features else self.n_feat_total
        self.mean_np, self.std_np = mean[:self.n_feat], std[:self.n_feat]
        self.mean = torch.from_numpy(self.mean_np.copy()).to(self.device)
        self.std = torch.from_numpy(self.std_np.copy()).to(self.device)
        self.chunks = [_upload_fp16(c, self.device) for c in host_chunks]

        self._sample_indices = sample_indices(self.chunk_lengths, obs_window, pred_steps, split, test_fraction)
        where = f"flat_nodes={self.n_nodes}" if self.flat_grid else f"grid={self.n_lon}×{self.n_lat}"
        print(f"[ChunkDataset] {split}: {len(self._sample_indices)} samples, {where}, feat={self.n_feat}, "
              f"obs={obs_window}, pred={pred_steps}")

    @classmethod
    def from_series(cls, series: torch.Tensor, mean, std, obs_window: int = 2, pred_steps: int = 1, split: str = "train",
                    n_features: Optional[int] = None, test_fraction: float = 0.2) -> "TimeseriesChunkDataset":
        """The dataset over an fp16 series that is already on the GPU, (T, lon, lat, C) or flat (T, N, C), with its
        scalers (numpy or tensors): what `dataset.DatasetBuilder`, `repair_channels` or `add_time_features` leave in
        HBM trains without a disk round trip.  The series is used as it is, not copied."""
        if not (series.is_cuda and series.dtype == torch.float16 and series.is_contiguous() and series.dim() in (3, 4)):
            raise TypeError("from_series needs a contiguous float16 GPU series (T, lon, lat, C) or (T, N, C)")
        self = cls.__new__(cls)
        self.data_dir, self.obs_window, self.pred_steps = None, obs_window, pred_steps
        self.split, self.test_fraction, self.device = split, test_fraction, series.device
        self.flat_grid = series.dim() == 3
        self.chunk_lengths, self.total_time = [int(series.shape[0])], int(series.shape[0])
        if self.flat_grid:
            self.n_nodes, self.n_lon, self.n_lat, self.n_feat_total = int(series.shape[1]), None, None, int(series.shape[2])
        else:
            self.n_nodes, self.n_lon, self.n_lat = None, int(series.shape[1]), int(series.shape[2])
            self.n_feat_total = int(series.shape[3])
        self.n_feat = n_features if n_features else self.n_feat_total
        as_np = lambda a: (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(np.float32)  # noqa: E731
        self.mean_np, self.std_np = as_np(mean)[:self.n_feat], as_np(std)[:self.n_feat]
        self.mean = torch.from_numpy(self.mean_np.copy()).to(self.device)
        self.std = torch.from_numpy(self.std_np.copy()).to(self.device)
        self.chunks = [series]
        self._sample_indices = sample_indices(self.chunk_lengths, obs_window, pred_steps, split, test_fraction)
        return self

    def __len__(self):
        return len(self._sample_indices)

    @property
    def grid_nodes(self) -> int:
        return self.n_nodes if self.flat_grid else self.n_lon * self.n_lat

    def batch_shapes(self, B: int):
        """Shapes of the (X, Y) a batch of B samples fills."""
        G = self.grid_nodes
        return (B, G, self.obs_window * self.n_feat), (B, G, self.pred_steps * self.n_feat)

    def batch(self, indices: Sequence[int], out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """A whole batch of windows in one launch per chunk.  out = (X, Y): fill these buffers in place (e.g.
        `TrainStep.input_buffers()`, so that the captured step needs no copy of the batch)."""
        pairs = [self._sample_indices[int(i)] for i in indices]
        B, G = len(pairs), self.grid_nodes
        by_chunk = {}
        for pos, (ci, t) in enumerate(pairs):
            by_chunk.setdefault(ci, []).append((pos, t))
        X, Y = out if out is not None else (None, None)
        for ci, items in by_chunk.items():
            t0 = torch.tensor([t for _, t in items], dtype=torch.int64).to(self.device)
            if len(by_chunk) == 1:
                return hip.window_pack(self.chunks[ci], t0, self.mean, self.std, self.n_feat, self.obs_window,
                                       self.pred_steps, out=out)
            x, y = hip.window_pack(self.chunks[ci], t0, self.mean, self.std, self.n_feat, self.obs_window, self.pred_steps)
            if X is None:
                X = torch.empty(B, G, x.shape[-1], dtype=torch.float32, device=self.device)
                Y = torch.empty(B, G, y.shape[-1], dtype=torch.float32, device=self.device)
            pos = torch.tensor([p for p, _ in items], dtype=torch.int64, device=self.device)
            X.index_copy_(0, pos, x)
            Y.index_copy_(0, pos, y)
        return X, Y

    def __getitem__(self, idx):
        X, Y = self.batch([idx])
        return X[0], Y[0]


def sample_indices(chunk_lengths: Sequence[int], obs_window: int, pred_steps: int, split: str,
                   test_fraction: float) -> List[Tuple[int, int]]:
    """(chunk, local_t) of every window that fits inside one chunk, then the split by time
    (`src/data/dataloader_chunked.py:132-172`): train = first (1 - test_fraction), test = the rest,
    val / test_only = first / second half of the test part, all = everything."""
    window = obs_window + pred_steps
    idx = [(ci, t) for ci, T in enumerate(chunk_lengths) for t in range(max(0, T - window + 1))]
    cut = int(len(idx) * (1 - test_fraction))
    if split == "train":
        return idx[:cut]
    if split == "test":
        return idx[cut:]
    if split in ("val", "test_only"):
        test = idx[cut:]
        half = len(test) // 2
        return test[:half] if split == "val" else test[half:]
    if split == "all":
        return idx
    raise ValueError(f"Unknown split: {split}")


# ------------------------------------------------------------------------------------------------
# dataset metadata (src/data/data_configs.py)
# ------------------------------------------------------------------------------------------------
class DatasetMetadata:
    """src/data/data_configs.py:4-23 (`cordinates`, spelled as there, is attached by the loaders)."""

    def __init__(self, flattened: bool, num_latitudes: int, num_longitudes: int, num_features: int, obs_window: int,
                 pred_window):
        self.flattened = flattened
        self.num_latitudes = num_latitudes
        self.num_longitudes = num_longitudes
        self.num_features = num_features
        self.obs_window = obs_window
        self.pred_window = pred_window
        self.flat_grid = False
        self.num_grid_nodes = num_latitudes * num_longitudes
        self.is_regional = None  # bool array (N,) marking the regional nodes of a flat grid


# name: (flattened, num_latitudes, num_longitudes, num_features, obs_window, pred_window); src/data/data_configs.py:26-109
_DATASETS = {
    "64x32_10f_5y_3obs": (True, 32, 64, 10, 3, 1),
    "64x32_33f_5y_5obs_uns": (False, 32, 64, 33, 5, 1),
    "64x32_12f_2y_2obs_1pred_uns": (False, 32, 64, 12, 2, 1),
    "demo_era5_small": (True, 32, 64, 3, 2, 1),
    "wb2_64x32_11f_2obs_1pred": (True, 32, 64, 11, 2, 1),
    "wb2_64x32_zq_15f_4obs_1pred": (True, 32, 64, 15, 4, 1),
    "wb2_64x32_zq_15f_4obs_4pred": (True, 32, 64, 15, 4, 4),
    "wb2_64x32_ar_15f_4obs_4pred": (True, 32, 64, 15, 4, 4),
    "wb2_512x256_19f_ar": (True, 256, 512, 19, 2, 1),
}
# the datasets the reference reads through the chunked loader (src/main.py:81-87)
CHUNKED_DATASET_NAMES = ("wb2_512x256_19f_ar", "wb2_512x256_19f_ar_v2", "multires", "region_krsk_cds_19f",
                         "region_krsk_cds_23f")


def get_dataset_metadata(dataset_name) -> DatasetMetadata:
    """The reference's table of its legacy datasets; any other name raises NotImplementedError, as there."""
    name = str(getattr(dataset_name, "value", dataset_name))
    if name not in _DATASETS:
        raise NotImplementedError(f"Dataset {dataset_name} is not supported.")
    return DatasetMetadata(*_DATASETS[name])


# ------------------------------------------------------------------------------------------------
# legacy tensor datasets (src/data/dataloader.py)
# ------------------------------------------------------------------------------------------------
class WeatherDataset:
    """`WeatherDataset` of src/data/dataloader.py:12-23 over tensors that stay in HBM as the files store them
    ([N, G, W, F]): `batch` selects the samples, the last steps and the first features in one
    `gcl_tensor_batch_pack` launch, `X` / `y` / `ds[i]` give the reference's tensors (on the device).

    store_X / store_y: float32 [N, G, W, F] on the device, shared between the splits of one file; the split holds
    samples [first, first + count)."""

    def __init__(self, store_X, store_y, first: int, count: int, obs_used: int, pred_used: int, feats_used: int,
                 flattened: bool = True):
        if store_X.dim() != 4 or store_y.dim() != 4 or store_X.shape[:2] != store_y.shape[:2] or store_X.shape[3] != store_y.shape[3]:
            raise ValueError(f"WeatherDataset: stores are [N, G, W, F] over the same samples, nodes and features, got "
                             f"{tuple(store_X.shape)} and {tuple(store_y.shape)}")
        if not (0 <= first and first + count <= store_X.shape[0] and count >= 0):
            raise ValueError(f"WeatherDataset: samples [{first}, {first + count}) of {store_X.shape[0]}")
        self.store_X, self.store_y = store_X, store_y
        self.first, self.count = int(first), int(count)
        self.obs_used, self.pred_used, self.feats_used = int(obs_used), int(pred_used), int(feats_used)
        self.flattened = bool(flattened)
        self._full = None

    def __len__(self):
        return self.count

    @property
    def grid_nodes(self) -> int:
        return int(self.store_X.shape[1])

    def batch_shapes(self, B: int):
        """Shapes of the (X, y) a batch of B samples fills."""
        G, F = self.grid_nodes, self.feats_used
        if self.flattened:
            return (B, G, self.obs_used * F), (B, G, self.pred_used * F)
        return (B, G, self.obs_used, F), (B, G, self.pred_used, F)

    def batch(self, indices: Sequence[int], out=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(X, y) of the samples `indices` (any order, repeats allowed) in one launch.  out = (X, y): buffers of
        `batch_shapes(len(indices))`, row- and batch-strided if need be, to fill in place."""
        idx = [int(i) for i in indices]
        for i in idx:
            if not 0 <= i < self.count:
                raise ValueError(f"sample index {i} outside [0, {self.count})")
        B, G = len(idx), self.grid_nodes
        sx, sy = self.batch_shapes(B)
        X, y = out if out is not None else (None, None)
        if B == 0:
            dev = self.store_X.device
            return (torch.empty(sx, device=dev), torch.empty(sy, device=dev)) if out is None else (X, y)
        if X is None:
            X = torch.empty(sx, dtype=torch.float32, device=self.store_X.device)
            y = torch.empty(sy, dtype=torch.float32, device=self.store_X.device)
        if tuple(X.shape) != sx or tuple(y.shape) != sy:
            raise ValueError(f"batch: out buffers {tuple(X.shape)} / {tuple(y.shape)}, expected {sx} / {sy}")
        flat = lambda t: t if t.dim() == 3 else _merge_last(t)  # noqa: E731
        t_idx = torch.tensor([self.first + i for i in idx], dtype=torch.int64)
        if self.store_X.is_cuda:  # stream-ordered upload: the host does not wait for the steps still in flight
            t_idx = t_idx.pin_memory().to(self.store_X.device, non_blocking=True)
        hip.tensor_batch_pack(self.store_X, self.store_y, t_idx, self.obs_used, self.pred_used, self.feats_used,
                              out=(flat(X), flat(y)))
        return X, y

    def _all(self):
        if self._full is None:
            self._full = self.batch(range(self.count))
        return self._full

    @property
    def X(self):
        return self._all()[0]

    @property
    def y(self):
        return self._all()[1]

    def __getitem__(self, idx):
        i = int(idx)
        if i < 0:
            i += self.count
        X, y = self.batch([i])
        return X[0], y[0]


def _merge_last(t):
    """[B, G, W, F] with a dense (W, F) tail as the [B, G, W * F] view over the same memory."""
    B, G, W, F = t.shape
    if t.stride(3) != 1 or (W > 1 and t.stride(2) != F):
        raise ValueError(f"batch: the (steps, features) tail of an out buffer must be dense, got strides {t.stride()}")
    return t.as_strided((B, G, W * F), (t.stride(0), t.stride(1), 1))


def read_legacy_tensors(data_path: str, data_config):
    """The host part of `load_train_and_test_datasets` (src/data/dataloader.py:25-109): the four tensors as stored,
    viewed [N, G, W, F], the shape checks, the grid shape taken from the file and the axes put in
    `metadata.cordinates`.  Returns (X_train, y_train, X_test, y_test, metadata); launches nothing."""
    from .train import FileNames

    md = get_dataset_metadata(data_config.dataset_name)
    F, obs, pred = md.num_features, md.obs_window, md.pred_window
    assert data_config.num_features_used <= F
    assert data_config.obs_window_used <= obs
    assert data_config.pred_window_used <= pred
    load = lambda name: torch.load(os.path.join(data_path, name), map_location="cpu", weights_only=True)  # noqa: E731
    X_train, y_train = load(FileNames.TRAIN_X), load(FileNames.TRAIN_Y)
    X_test, y_test = load(FileNames.TEST_X), load(FileNames.TEST_Y)
    if X_train.ndim == 4:  # [N, LONG, LAT, obs*F]
        _, LONG, LAT, X_F = X_train.shape
        assert X_F == F * obs
        _, _, _, Y_F = y_train.shape
        assert Y_F == F * pred
    elif X_train.ndim == 5:  # [N, LONG, LAT, OBS, F]
        _, LONG, LAT, OBS, X_F = X_train.shape
        _, _, _, PRED, Y_F = y_train.shape
        assert X_F == F
        assert Y_F == X_F
        assert OBS == obs
        assert PRED == pred
    else:
        raise RuntimeError(f"Unexpected X_train.ndim={X_train.ndim}")
    if LONG != md.num_longitudes or LAT != md.num_latitudes:
        md.num_longitudes, md.num_latitudes = int(LONG), int(LAT)
    coords_npz = os.path.join(data_path, "coords.npz")
    if os.path.exists(coords_npz):
        cz = np.load(coords_npz)
        lons, lats = cz["longitude"].astype(np.float32), cz["latitude"].astype(np.float32)
    else:
        lats = np.linspace(-90, 90, LAT, endpoint=True).astype(np.float32)
        lons = np.linspace(0, 360, LONG, endpoint=False).astype(np.float32)
    md.cordinates = (lats, lons)
    G = LONG * LAT
    as4 = lambda t, W: t.to(torch.float32).contiguous().view(-1, G, W, F)  # noqa: E731
    return as4(X_train, obs), as4(y_train, pred), as4(X_test, obs), as4(y_test, pred), md


def legacy_split_sizes(n_test: int):
    """(val, test) sample counts: validation is the first half of the test file (src/data/dataloader.py:142-147)."""
    val = n_test // 2
    return val, n_test - val


def load_train_and_test_datasets(data_path: str, data_config, device="cuda:0"):
    """src/data/dataloader.py:25-153 with the tensors resident on `device`: each file is uploaded once, as stored; the
    validation and test sets are two ranges of the one test store.  Returns (train, val, test, metadata)."""
    X_train, y_train, X_test, y_test, md = read_legacy_tensors(data_path, data_config)
    dev = torch.device(device)
    X_train, y_train, X_test, y_test = (t.to(dev) for t in (X_train, y_train, X_test, y_test))
    used = (data_config.obs_window_used, data_config.pred_window_used, data_config.num_features_used,
            data_config.want_feats_flattened)
    n_val, n_test = legacy_split_sizes(int(X_test.shape[0]))
    return (WeatherDataset(X_train, y_train, 0, int(X_train.shape[0]), *used),
            WeatherDataset(X_test, y_test, 0, n_val, *used),
            WeatherDataset(X_test, y_test, n_val, n_test, *used), md)


# ------------------------------------------------------------------------------------------------
# chunked datasets (src/data/dataloader_chunked.py:226-303)
# ------------------------------------------------------------------------------------------------
def chunked_metadata(data_path: str, obs_window: int = 2, pred_steps: int = 1, n_features: Optional[int] = None):
    """(metadata, n_feat) of a chunked dataset directory, from coords.npz, dataset_info.json and variables.json
    alone (src/data/dataloader_chunked.py:242-259,274-301)."""
    coords = np.load(os.path.join(data_path, "coords.npz"))
    lons, lats = coords["longitude"], coords["latitude"]
    info_file, is_flat = os.path.join(data_path, "dataset_info.json"), False
    if os.path.exists(info_file):
        with open(info_file) as fh:
            is_flat = json.load(fh).get("flat", False)
    with open(os.path.join(data_path, "variables.json")) as fh:
        var_names = json.load(fh)
    n_feat = n_features if n_features else len(var_names)
    if is_flat:  # lats and lons are paired (N,) arrays
        md = DatasetMetadata(flattened=True, num_latitudes=0, num_longitudes=0, num_features=n_feat,
                             obs_window=obs_window, pred_window=pred_steps)
        md.flat_grid = True
        md.num_grid_nodes = len(lats)
        md.is_regional = coords["is_regional"] if "is_regional" in coords else None
    else:
        md = DatasetMetadata(flattened=True, num_latitudes=len(lats), num_longitudes=len(lons), num_features=n_feat,
                             obs_window=obs_window, pred_window=pred_steps)
        md.flat_grid = False
    md.cordinates = (lats.astype(np.float32), lons.astype(np.float32))
    return md, n_feat


def _resplit(ds: TimeseriesChunkDataset, split: str) -> TimeseriesChunkDataset:
    """Another split over the SAME device tensors (series chunks and scalers are shared, not copied): what
    `from_series` on the same tensor gives, for directories of several chunks as well."""
    import copy

    other = copy.copy(ds)
    other.split = split
    other._sample_indices = sample_indices(ds.chunk_lengths, ds.obs_window, ds.pred_steps, split, ds.test_fraction)
    return other


def load_chunked_datasets(data_path: str, obs_window: int = 2, pred_steps: int = 1, n_features: Optional[int] = None,
                          test_fraction: float = 0.2, test_split: str = "test_only", device="cuda:0"):
    """src/data/dataloader_chunked.py:226-303: (train, val, test, metadata).  The series is uploaded once and the
    three splits index the same tensor."""
    md, n_feat = chunked_metadata(data_path, obs_window, pred_steps, n_features)
    train = TimeseriesChunkDataset(data_path, obs_window=obs_window, pred_steps=pred_steps, split="train",
                                   n_features=n_feat, test_fraction=test_fraction, device=device)
    return train, _resplit(train, "val"), _resplit(train, test_split), md


# ------------------------------------------------------------------------------------------------
# batches from a device-resident dataset
# ------------------------------------------------------------------------------------------------
class DeviceLoader:
    """A re-iterable of (X, y) device batches from `dataset.batch(indices, out=...)`.

    The index stream is torch's own `DataLoader` over `range(len(dataset))` with the same `batch_size`, `shuffle`,
    `drop_last` and `generator` (and no workers): only integers pass through it, so the sample order and every draw
    from the global RNG are those of the reference's `DataLoader` over the dataset itself.

    buffers: a callable returning (X, y) buffers or None, e.g. `TrainStep.input_buffers`: a batch those buffers fit is
    written into them in place, so a captured step needs no second copy of it."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator=None, buffers=None):
        from torch.utils.data import DataLoader

        self.dataset, self.buffers = dataset, buffers
        self.batch_size = batch_size
        self._indices = DataLoader(range(len(dataset)), batch_size=batch_size, shuffle=shuffle, drop_last=drop_last,
                                   generator=generator, num_workers=0)

    def __len__(self):
        return len(self._indices)

    def _out(self, B: int):
        bufs = self.buffers() if self.buffers is not None else None
        if bufs is None:
            return None
        shapes = self.dataset.batch_shapes(B) if hasattr(self.dataset, "batch_shapes") else None
        if shapes is None or any(b is None or tuple(b.shape) != s for b, s in zip(bufs, shapes)):
            return None
        return tuple(bufs)

    def __iter__(self):
        for idx in self._indices:
            idx = idx.tolist()
            yield self.dataset.batch(idx, out=self._out(len(idx)))
