"""Build, repair and extend the fp16 dataset directory every loader of this tree starts from, on the GPU.

The five files (`data.npy`, a raw fp16 memmap of shape (T, lon, lat, C); `scalers.npz`; `coords.npz`; `variables.json`;
`dataset_info.json`) are what the reference makes and mends with a family of numpy scripts that share one arithmetic
core - a strided 2-byte pass per channel over a memmap plus two passes for the sums:

  scripts/build_dataset_512x256.py:195-353   DatasetBuilder            pack a time block, its sums, Welford
  scripts/recompute_wb2_scalers.py:145-206   ScalerStats / recompute_scalers
  scripts/repair_dataset.py:121-204          repair_channels           overwrite overflowed channels, stats of the rest
  scripts/add_time_features.py:51-150        add_time_features         four time channels, new scalers
  scripts/check_23f_data.py                  check_dataset
  scripts/compare_scalers.py                 compare_scalers

Here the series lives in HBM (as it does for training, see data.py) and every pass is one launch of csrc/dataset.hip.
Nothing synchronises until a result is asked for: a whole build enqueues its packs and Welford updates, and the state
crosses to the host once.  Where a source is already on the device (a decoder, a regridder, another series) nothing
else moves; a build from host arrays is bound by their upload, not by the pack.
"""
import json
import os
import shutil
from datetime import datetime, timedelta
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import hip
from .data import _upload_fp16

VAR_ORDER = [
    "t2m", "10u", "10v", "msl", "tp",
    "sp", "tcwv",
    "z_surf", "lsm",
    "t@850", "u@850", "v@850", "z@850", "q@850",
    "t@500", "u@500", "v@500", "z@500", "q@500",
]
# fp16 ends at 65504: pressures (Pa) and geopotentials (m^2/s^2) are scaled BEFORE the cast (:77-83)
SCALE_FACTORS = {"msl": 0.01, "sp": 0.01, "z_surf": 1 / 9.80665, "z@850": 1 / 9.80665, "z@500": 1 / 9.80665}
TIME_FEATURES = ["sin_hour", "cos_hour", "sin_doy", "cos_doy"]
STD_FLOOR = 1e-6  # :350-351


def welford_update(running_mean, running_m2, total_n, block_sum, block_sumsq, block_n):
    """Host form of `welford_update` (scripts/build_dataset_512x256.py:126-136), the reference's signature: merge a
    block given by its sum and sum of squares into running (mean, M2, n).  The device form is gcl_dataset_welford."""
    block_mean = block_sum / block_n
    block_var = np.maximum(block_sumsq / block_n - block_mean ** 2, 0.0)
    delta = block_mean - running_mean
    new_n = total_n + block_n
    running_mean += delta * (block_n / new_n)
    running_m2 += block_var * block_n + (delta ** 2) * total_n * block_n / new_n
    return running_mean, running_m2, new_n


def time_features(time_start: str, n_time: int) -> np.ndarray:
    """(T, 4) float32: sin / cos of the hour of day and of the day of year of 6-hourly steps from `time_start`
    ("YYYY-MM-DD"), exactly as scripts/add_time_features.py:51-65 forms them (float32 arithmetic throughout)."""
    t0 = datetime.strptime(time_start, "%Y-%m-%d")
    times = [t0 + timedelta(hours=6 * i) for i in range(n_time)]
    hours = np.array([t.hour + t.minute / 60 for t in times], dtype=np.float32)
    doys = np.array([t.timetuple().tm_yday for t in times], dtype=np.float32)
    return np.stack([np.sin(2 * np.pi * hours / 24.0), np.cos(2 * np.pi * hours / 24.0),
                     np.sin(2 * np.pi * doys / 365.25), np.cos(2 * np.pi * doys / 365.25)], axis=-1)


def _flags(nonfinite: str) -> int:
    try:
        return {"keep": 0, "nan": hip.DATASET_NAN_TO_ZERO,
                "zero": hip.DATASET_NAN_TO_ZERO | hip.DATASET_INF_TO_ZERO}[nonfinite]
    except KeyError:
        raise ValueError(f"nonfinite must be 'keep', 'nan' or 'zero', got {nonfinite!r}") from None


def _planes(arrays, device):
    """float32 contiguous device tensors of numpy arrays or tensors (a host array is uploaded, nothing else is copied)."""
    out = []
    for a in arrays:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) if isinstance(a, np.ndarray) else a
        out.append(t.to(device=device, dtype=torch.float32).contiguous())
    return out


class ScalerStats:
    """Running per-channel (mean, M2, n) on the device, merged block by block as the reference does on the host.

    `add_fields` takes raw float32 fields (statistics only, scripts/recompute_wb2_scalers.py:161-199), `add_series`
    rows of an fp16 series in `time_chunk` blocks (so block boundaries, and with them the rounding, match the
    reference's passes over a memmap), `result()` the final mean / std / n - the only call that synchronises."""

    def __init__(self, C: int, device, time_chunk: int = 500):
        self.C, self.device, self.time_chunk = int(C), torch.device(device), int(time_chunk)
        z = lambda dt, n=self.C: torch.zeros(n, dtype=dt, device=self.device)  # noqa: E731
        self.mean, self.m2, self.n = z(torch.float64), z(torch.float64), z(torch.int64, 1)
        self.block_sum, self.block_sumsq = z(torch.float64), z(torch.float64)
        self._rest = (z(torch.float32), z(torch.float32), z(torch.int64), z(torch.int64))

    def pack(self, series, t0: int, nt: int, sources, chans, scales, grid=None):
        """Pack `sources` into `series` (None: sums only) and leave their block sums in block_sum / block_sumsq."""
        m = hip.dataset_max_sources()
        for i in range(0, len(sources), m):
            hip.dataset_pack(sources[i:i + m], chans[i:i + m], scales[i:i + m], nt, series, t0, self.block_sum,
                             self.block_sumsq, grid=grid)

    def series_sums(self, series, t_s: int, t_e: int, nonfinite: str = "zero"):
        """Block sums of all channels of rows [t_s, t_e) of `series` into block_sum / block_sumsq."""
        hip.dataset_stats(series, t_s, t_e, _flags(nonfinite), out=(self.block_sum, self.block_sumsq) + self._rest)

    def merge(self, block_n: int):
        hip.dataset_welford(self.mean, self.m2, self.n, self.block_sum, self.block_sumsq, block_n)

    def add_fields(self, fields: Sequence, n_lon: int, n_lat: int, scales: Optional[Sequence[float]] = None):
        """One block of raw fields, one per channel in channel order: [nt, lon, lat] float32 (numpy or device), or
        [lon, lat] for a time-invariant one."""
        if len(fields) != self.C:
            raise ValueError(f"add_fields: {len(fields)} fields for {self.C} channels")
        planes = _planes(fields, self.device)
        P = n_lon * n_lat
        nt = max(int(p.numel() // P) for p in planes)
        self.pack(None, 0, nt, planes, list(range(self.C)), list(scales) if scales is not None else [1.0] * self.C,
                  grid=(n_lon, n_lat, self.C))
        self.merge(nt * P)

    def add_series(self, series: torch.Tensor, t_s: int = 0, t_e: Optional[int] = None, nonfinite: str = "zero"):
        """Rows [t_s, t_e) of an fp16 series, one Welford block per `time_chunk` rows counted from t_s."""
        t_e = series.shape[0] if t_e is None else int(t_e)
        P = int(np.prod(series.shape[1:-1]))
        for a in range(int(t_s), t_e, self.time_chunk):
            b = min(a + self.time_chunk, t_e)
            self.series_sums(series, a, b, nonfinite)
            self.merge((b - a) * P)

    def result(self) -> Tuple[np.ndarray, np.ndarray, int]:
        """(mean float32, std float32, n): std = max(sqrt(M2 / max(n, 1)), 1e-6) in float64, then the casts (:350-353)."""
        n = int(self.n.item())
        mean, m2 = self.mean.cpu().numpy(), self.m2.cpu().numpy()
        std = np.maximum(np.sqrt(m2 / max(n, 1)), STD_FLOOR)
        return mean.astype(np.float32), std.astype(np.float32), n


def _write_scalers(folder, mean, std, n):
    np.savez(os.path.join(folder, "scalers.npz"), mean=mean, std=std, n=n)


def _read_info(data_dir):
    with open(os.path.join(data_dir, "dataset_info.json")) as fh:
        info = json.load(fh)
    if info.get("flat", False):
        shape = (info["n_time"], info["n_nodes"], info["n_feat"])
    else:
        shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
    return info, shape


def load_series(data_dir: str, device) -> Tuple[torch.Tensor, dict]:
    """(`data.npy` of a dataset directory as an fp16 tensor on `device`, its dataset_info)."""
    info, shape = _read_info(data_dir)
    mm = np.memmap(os.path.join(data_dir, "data.npy"), dtype=np.float16, mode="r", shape=shape)
    return _upload_fp16(mm, device), info


def save_series(series: torch.Tensor, path: str, t_s: int = 0, t_e: Optional[int] = None, create: bool = False,
                slab_rows: Optional[int] = None):
    """Rows [t_s, t_e) of the device series into the raw memmap `path` (created with the series' shape if asked)."""
    t_e = series.shape[0] if t_e is None else t_e
    mm = np.memmap(path, dtype=np.float16, mode="w+" if create else "r+", shape=tuple(series.shape))
    per_t = max(1, int(np.prod(series.shape[1:])) * 2)
    step = slab_rows or max(1, (1 << 30) // per_t)
    for t in range(t_s, t_e, step):
        mm[t:min(t + step, t_e)] = series[t:min(t + step, t_e)].cpu().numpy()
    mm.flush()
    del mm


class DatasetBuilder:
    """`download_compute_save` + the metadata of `main` (scripts/build_dataset_512x256.py:195-353, :416-437) with the
    series on the device.  Feed it time blocks with `add_block`; `series` is the fp16 tensor (T, lon, lat, C) a
    `TimeseriesChunkDataset.from_series` trains on directly; with `out_dir` every block is also written to `data.npy`
    followed by `progress.json`, and `finish` writes the other four files."""

    def __init__(self, var_names: Sequence[str], n_time: int, n_lon: int, n_lat: int, time_start: str, time_end: str,
                 device, out_dir: Optional[str] = None, time_chunk: int = 500,
                 scale_factors: Dict[str, float] = SCALE_FACTORS):
        self.var_names = list(var_names)
        self.n_time, self.n_lon, self.n_lat = int(n_time), int(n_lon), int(n_lat)
        self.time_start, self.time_end, self.device = time_start, time_end, torch.device(device)
        self.out_dir, self.time_chunk, self.scale_factors = out_dir, int(time_chunk), dict(scale_factors)
        C = len(self.var_names)
        self.series = torch.empty(self.n_time, self.n_lon, self.n_lat, C, dtype=torch.float16, device=self.device)
        self.stats = ScalerStats(C, self.device, self.time_chunk)
        self.t_done = 0
        self._fresh = True  # data.npy has still to be created
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)

    def _scale(self, name: str) -> float:
        return float(np.float32(self.scale_factors.get(name, 1.0)))

    def add_block(self, t_start: int, fields: Dict[str, Union[np.ndarray, torch.Tensor]]):
        """Rows [t_start, t_start + nt) from {name: [nt, lon, lat] or, time-invariant, [lon, lat]} (numpy or device)."""
        missing = [n for n in self.var_names if n not in fields]
        if missing:
            raise KeyError(f"add_block: no field for {missing}")
        shapes = {tuple(fields[n].shape) for n in self.var_names}
        nts = {s[0] for s in shapes if len(s) == 3}
        if len(nts) != 1 or any(s[-2:] != (self.n_lon, self.n_lat) for s in shapes):
            raise ValueError(f"add_block: fields of shapes {sorted(shapes)} on a {self.n_lon} x {self.n_lat} grid")
        nt = nts.pop()
        if t_start < 0 or t_start + nt > self.n_time:
            raise ValueError(f"add_block: rows [{t_start}, {t_start + nt}) leave the {self.n_time} time steps")
        planes = _planes([fields[n] for n in self.var_names], self.device)
        self.stats.pack(self.series, t_start, nt, planes, list(range(len(planes))),
                        [self._scale(n) for n in self.var_names])
        self.stats.merge(nt * self.n_lon * self.n_lat)
        self.t_done = t_start + nt
        if self.out_dir:
            save_series(self.series, os.path.join(self.out_dir, "data.npy"), t_start, self.t_done, create=self._fresh)
            self._fresh = False
            with open(os.path.join(self.out_dir, "progress.json"), "w") as fh:
                fh.write(json.dumps({"last_completed_timestep": self.t_done, "chunk_size": self.time_chunk}))

    @classmethod
    def resume(cls, out_dir: str, var_names, n_time, n_lon, n_lat, time_start, time_end, device, time_chunk: int = 500,
               scale_factors: Dict[str, float] = SCALE_FACTORS) -> "DatasetBuilder":
        """Pick an interrupted build up from `progress.json`, one chunk back (:393-402: the last one may be incomplete);
        the rows before that are uploaded from `data.npy` and their statistics rebuilt by gcl_dataset_stats in
        `time_chunk` blocks (:238-253).  Continue with add_block(b.t_done, ...)."""
        b = cls(var_names, n_time, n_lon, n_lat, time_start, time_end, device, out_dir, time_chunk, scale_factors)
        prog, path = os.path.join(out_dir, "progress.json"), os.path.join(out_dir, "data.npy")
        start = 0
        if os.path.exists(prog) and os.path.exists(path):
            with open(prog) as fh:
                saved = json.load(fh).get("last_completed_timestep")
            if saved:
                start = max(0, int(saved) - b.time_chunk)
        if start > 0:
            mm = np.memmap(path, dtype=np.float16, mode="r", shape=tuple(b.series.shape))
            b.series[:start].copy_(_upload_fp16(mm[:start], b.device))
            b.stats.add_series(b.series, 0, start, nonfinite="zero")
            b._fresh = False
        b.t_done = start
        return b

    def dataset_info(self) -> dict:
        C = len(self.var_names)
        gb = self.n_time * self.n_lon * self.n_lat * C * 2 / (1024 ** 3)
        return {"time_start": self.time_start, "time_end": self.time_end, "n_time": self.n_time, "n_lon": self.n_lon,
                "n_lat": self.n_lat, "n_feat": C, "variables": self.var_names, "dtype": "float16", "file": "data.npy",
                "size_gb": round(gb, 1)}

    def finish(self, longitude, latitude) -> Tuple[np.ndarray, np.ndarray, int]:
        """(mean, std, n); with `out_dir` also scalers.npz, coords.npz, variables.json and dataset_info.json with the
        reference's keys and JSON text (:416-437), and progress.json goes."""
        mean, std, n = self.stats.result()
        if self.out_dir:
            _write_scalers(self.out_dir, mean, std, n)
            np.savez(os.path.join(self.out_dir, "coords.npz"), longitude=np.asarray(longitude).astype(np.float32),
                     latitude=np.asarray(latitude).astype(np.float32))
            with open(os.path.join(self.out_dir, "variables.json"), "w") as fh:
                fh.write(json.dumps(self.var_names, indent=2, ensure_ascii=False))
            with open(os.path.join(self.out_dir, "dataset_info.json"), "w") as fh:
                fh.write(json.dumps(self.dataset_info(), indent=2))
            prog = os.path.join(self.out_dir, "progress.json")
            if os.path.exists(prog):
                os.unlink(prog)
        return mean, std, n


def _series_of(src, device):
    """(series, data_dir or None) of a dataset directory or a device series."""
    if isinstance(src, (str, os.PathLike)):
        return load_series(os.fspath(src), device)[0], os.fspath(src)
    return src, None


def recompute_scalers(src, time_chunk: int = 500, nonfinite: str = "zero", device="cuda:0"):
    """(mean, std, n) of a dataset directory (its scalers.npz is rewritten) or of a device series, by the block scheme
    of the reference's builders (Welford over `time_chunk` rows, floor 1e-6)."""
    series, folder = _series_of(src, device)
    st = ScalerStats(series.shape[-1], series.device, time_chunk)
    st.add_series(series, 0, None, nonfinite)
    mean, std, n = st.result()
    if folder:
        _write_scalers(folder, mean, std, n)
    return mean, std, n


def repair_channels(src, blocks, channels: Dict[int, float], time_chunk: int = 500, device="cuda:0"):
    """scripts/repair_dataset.py:121-204: overwrite the channels that overflowed fp16 and recompute every scaler.

    channels: {channel index: scale factor}.  blocks: an iterable of (t_start, {channel index: raw float32 field
    [nt, lon, lat] or [lon, lat]}) covering the series in order.  Per block the other channels' sums come from the
    fp16 already there (NaN and +-inf as 0, :144), the listed ones from the new values; their columns are rewritten by
    a partial pack that leaves every other byte alone.  A directory gets its data.npy and scalers.npz rewritten.
    Returns (series, mean, std, n)."""
    series, folder = _series_of(src, device)
    chans = sorted(int(c) for c in channels)
    scales = [float(np.float32(channels[c])) for c in chans]
    P = int(np.prod(series.shape[1:-1]))
    st = ScalerStats(series.shape[-1], series.device, time_chunk)
    for t_start, fields in blocks:
        planes = _planes([fields[c] for c in chans], series.device)
        nt = max(int(p.numel() // P) for p in planes)
        st.series_sums(series, t_start, t_start + nt, "zero")  # all channels, then the listed ones are replaced
        st.pack(series, t_start, nt, planes, chans, scales)
        st.merge(nt * P)
    mean, std, n = st.result()
    if folder:
        save_series(series, os.path.join(folder, "data.npy"))
        _write_scalers(folder, mean, std, n)
    return series, mean, std, n


def add_time_features(src_dir: str, dst_dir: str, device="cuda:0"):
    """scripts/add_time_features.py: a copy of the dataset with the four time channels appended (one launch), its
    scalers recomputed over the new series and the metadata updated.  The scalers are mean and population std from
    float64 sums (std < 1e-8 -> 1.0); the reference forms them in float32 over the flattened array.  Returns the new
    device series."""
    src, info = load_series(src_dir, device)
    n_time, n_old = info["n_time"], info["n_feat"]
    extra = torch.from_numpy(time_features(info["time_start"], n_time).astype(np.float16)).to(src.device)
    dst = hip.dataset_widen(src, extra)
    del src
    s, q = hip.dataset_stats(dst, 0, n_time, 0)[:2]
    n = n_time * int(np.prod(dst.shape[1:-1]))
    s, q = s.cpu().numpy(), q.cpu().numpy()
    mean = s / n
    std = np.sqrt(np.maximum(q / n - mean * mean, 0.0))
    mean, std = mean.astype(np.float32), std.astype(np.float32)
    std[std < 1e-8] = 1.0
    os.makedirs(dst_dir, exist_ok=True)
    save_series(dst, os.path.join(dst_dir, "data.npy"), create=True)
    _write_scalers(dst_dir, mean, std, np.array(n))
    shutil.copy2(os.path.join(src_dir, "coords.npz"), os.path.join(dst_dir, "coords.npz"))
    new_vars = info["variables"] + TIME_FEATURES
    with open(os.path.join(dst_dir, "variables.json"), "w") as fh:
        json.dump(new_vars, fh, indent=2)
    new_info = dict(info)
    new_info["n_feat"] = n_old + 4
    new_info["variables"] = new_vars
    new_info["size_gb"] = round(int(np.prod(dst.shape)) * 2 / 1e9, 3)
    new_info["source"] = info.get("source", "") + " + time features (sin/cos hour, doy)"
    with open(os.path.join(dst_dir, "dataset_info.json"), "w") as fh:
        json.dump(new_info, fh, indent=2, ensure_ascii=False)
    return dst


def check_dataset(src, device="cuda:0", names: Optional[Sequence[str]] = None, verbose: bool = True) -> dict:
    """The per-channel table of scripts/check_23f_data.py: min / max over the finite values, mean / std (NaN and inf
    left out of the sums), the counts of NaN and of +-inf and, for a directory, the stored scalers next to them.  A
    channel that overflowed fp16 - the bug repair_channels exists for - shows as a non-zero `inf` count."""
    series, folder = _series_of(src, device)
    s, q, mn, mx, nn, ni = (t.cpu().numpy() for t in hip.dataset_stats(series, 0, series.shape[0], _flags("zero")))
    n = int(np.prod(series.shape[:-1]))
    mean = s / n
    std = np.sqrt(np.maximum(q / n - mean * mean, 0.0))
    out = {"min": mn, "max": mx, "mean": mean, "std": std, "nan": nn, "inf": ni, "n": n}
    if folder:
        sc = np.load(os.path.join(folder, "scalers.npz"))
        out["stored_mean"], out["stored_std"] = sc["mean"], sc["std"]
        if names is None and os.path.exists(os.path.join(folder, "variables.json")):
            with open(os.path.join(folder, "variables.json")) as fh:
                names = json.load(fh)
    out["names"] = list(names) if names is not None else [str(c) for c in range(series.shape[-1])]
    if verbose:
        print(f"{'#':>3s} {'name':>8s} {'min':>12s} {'max':>12s} {'mean':>12s} {'std':>12s} {'NaN':>10s} {'inf':>10s}")
        for c, name in enumerate(out["names"]):
            line = (f"{c:3d} {name:>8s} {mn[c]:12.4f} {mx[c]:12.4f} {mean[c]:12.4f} {std[c]:12.4f} {int(nn[c]):10d} "
                    f"{int(ni[c]):10d}")
            if folder:
                line += f"   stored mean={out['stored_mean'][c]:12.4f} std={out['stored_std'][c]:12.4f}"
            print(line)
    return out


def compare_scalers(dirs: Dict[str, str], verbose: bool = True) -> dict:
    """scripts/compare_scalers.py: {label: {variable: (mean, std)}} of several dataset directories, printed side by side
    in the reference's format."""
    out = {}
    for label, path in dirs.items():
        sc = np.load(os.path.join(path, "scalers.npz"))
        with open(os.path.join(path, "variables.json")) as fh:
            names = json.load(fh)
        out[label] = {v: (float(sc["mean"][i]), float(sc["std"][i])) for i, v in enumerate(names)}
        if verbose:
            print(f"\n=== {label} ===\nPath: {path}")
            for i, v in enumerate(names):
                print(f"  {i:2d} {v:>8s}  mean={sc['mean'][i]:12.4f}  std={sc['std'][i]:12.4f}")
    return out
