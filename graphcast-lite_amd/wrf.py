"""The WRF benchmark on the HIP path: drop-in for `scripts/compare_wrf_era5.py` (WRF against ERA5 on the curvilinear WRF
grid) and `scripts/compare_wrf.py` (forecast against WRF against ERA5 over the WRF box).

* Host helpers with the reference's names and results (numpy and json only): `load_wrf_json`, `load_wrf`, `load_era5`,
  `wrf_region_indices`, `match_steps`, `find_wrf_matching_sample`, and `wrf_point_tables` - what scipy's
  `RegularGridInterpolator(bounds_error=False, fill_value=nan)` does with the WRF points, as four node numbers and
  four float64 weights per point, negative numbers marking the points outside the source axes.
* Device functions: `interpolate_era5_to_wrf` (`gcl_wrf_sample`), `compute_metrics` (`gcl_wrf_scores`).
* `compare_wrf_era5`: every variable x step of WRF against the fp16 series in HBM, one launch, the script's table.
* `WrfBenchmark` / `CapturedWrfBenchmark`: box means of normalised forecast and truth batches (`gcl_wrf_box_means`),
  optionally field-level scores on the WRF grid, and the tables of `compare_wrf.py`.

Reading netCDF WRF output (xarray, netCDF4) and plotting are not provided: WRF comes from the JSON export.

Kernels: csrc/wrf.hip.
"""
import json
from datetime import datetime, timedelta
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured
from .interp_tables import CORNERS, TableCache, bilinear_corners, device_tables

# WRF d03 (Krasnoyarsk), compare_wrf.py:36-37
WRF_LAT_MIN, WRF_LAT_MAX = 55.5, 56.5
WRF_LON_MIN, WRF_LON_MAX = 92.0, 94.0

# compare_wrf.py:41-47
VAR_MAPPING = {
    "t2m": {"wrf_name": "T2", "unit": "K", "wrf_scale": 1.0, "our_scale": 1.0},
    "10u": {"wrf_name": "U10", "unit": "m/s", "wrf_scale": 1.0, "our_scale": 1.0},
    "10v": {"wrf_name": "V10", "unit": "m/s", "wrf_scale": 1.0, "our_scale": 1.0},
    "sp": {"wrf_name": "PSFC", "unit": "Pa", "wrf_scale": 1.0, "our_scale": 100.0},
}
# compare_wrf_era5.py:34-40
VAR_MAP = {
    "t2_K": {"era5": "t2m", "unit": "K", "era5_to_wrf": 1.0},
    "u10_ms": {"era5": "10u", "unit": "m/s", "era5_to_wrf": 1.0},
    "v10_ms": {"era5": "10v", "unit": "m/s", "era5_to_wrf": 1.0},
    "psfc_Pa": {"era5": "sp", "unit": "hPa", "era5_to_wrf": 0.01},
}
# compare_wrf_era5.py:45-51
DATASET_SCALE = {"msl": 0.01, "sp": 0.01, "z_surf": 1 / 9.80665, "z@850": 1 / 9.80665, "z@500": 1 / 9.80665}
JSON_KEY_MAP = {"t2_K": "t2m", "u10_ms": "10u", "v10_ms": "10v", "psfc_Pa": "sp"}  # compare_wrf.py:219-224
MATCH_DELTAS = (0, -1, 1, -2, 2)  # the order find_wrf_matching_sample tries the offsets in (:670-681)


# ======================================================================================================================
# Host helpers
# ======================================================================================================================
def load_wrf_json(path):
    """(fields, lat, lon, times, domain) of a WRF JSON export (compare_wrf_era5.py:54-73): fields[key] float32
    [n_time, ny, nx] for t2_K, u10_ms, v10_ms, psfc_Pa; lat / lon float32 [ny, nx]."""
    with open(path) as f:
        d = json.load(f)
    lat = np.array(d["lat"], dtype=np.float32)
    lon = np.array(d["lon"], dtype=np.float32)
    fields = {key: np.array(d["domain_fields"][key], dtype=np.float32) for key in VAR_MAP}
    return fields, lat, lon, d["times"], d["domain"]


def _six_hourly(hourly: np.ndarray) -> np.ndarray:
    """compare_wrf.py:235-243: 25 or more hourly values -> 0, 6, 12, 18, 24; 5 or more -> the first five (already 6 h
    apart); fewer -> all of them."""
    n = len(hourly)
    idx = [0, 6, 12, 18, 24] if n >= 25 else list(range(min(5, n))) if n >= 5 else list(range(n))
    return hourly[idx]


def load_wrf(wrf_path, n_horizons=None) -> Dict[str, np.ndarray]:
    """{our name: float32 domain means at the 6 h steps (init, +6 h, ..)} of a WRF JSON export (compare_wrf.py:208-249).
    netCDF files (the reference reads them through xarray or netCDF4) are not provided."""
    if not str(wrf_path).endswith(".json"):
        raise NotImplementedError(f"load_wrf: {wrf_path} is not a JSON export; reading netCDF WRF output (xarray / "
                                  "netCDF4) is not provided - export the domain means to JSON first")
    with open(wrf_path) as f:
        domain_mean = json.load(f).get("domain_mean", {})
    return {ours: _six_hourly(np.array(domain_mean[key], dtype=np.float32))
            for key, ours in JSON_KEY_MAP.items() if key in domain_mean}


def load_era5(era5_dir):
    """(data fp16 memmap [n_time, n_lon, n_lat, n_feat], lons float64, lats float64, var_names, info) of a dataset
    directory whose series is in physical units (compare_wrf_era5.py:76-124)."""
    era5_dir = Path(era5_dir)
    info = json.loads((era5_dir / "dataset_info.json").read_text())
    var_names = json.loads((era5_dir / "variables.json").read_text())
    coords = np.load(era5_dir / "coords.npz")
    lons, lats = coords["longitude"].astype(np.float64), coords["latitude"].astype(np.float64)
    shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
    data = np.memmap(str(era5_dir / "data.npy"), dtype=np.float16, mode="r", shape=shape)
    return data, lons, lats, var_names, info


def wrf_region_indices(lats, lons, flat_grid: bool = False) -> np.ndarray:
    """The nodes inside the WRF box (compare_wrf.py:93-132).  A flat grid (per-node coordinates; also auto-detected
    when both have the same length above 512) is filtered directly; a regular one gives `j * n_lat + i` over the
    longitudes j and latitudes i inside, longitude-major."""
    lats, lons = np.asarray(lats, dtype=np.float32), np.asarray(lons, dtype=np.float32)
    if not flat_grid and len(lats) == len(lons) and len(lats) > max(512, 256):
        flat_grid = True
    if flat_grid:
        mask = (lats >= WRF_LAT_MIN) & (lats <= WRF_LAT_MAX) & (lons >= WRF_LON_MIN) & (lons <= WRF_LON_MAX)
        return np.where(mask)[0]
    n_lat = len(lats)
    lat_idx = np.where((lats >= WRF_LAT_MIN) & (lats <= WRF_LAT_MAX))[0]
    lon_idx = np.where((lons >= WRF_LON_MIN) & (lons <= WRF_LON_MAX))[0]
    return np.array([j * n_lat + i for j in lon_idx for i in lat_idx], dtype=np.int64)


def match_steps(time_start: str, wrf_times: Sequence[str], n_era5: int):
    """[(era5 index, WRF hourly index, label)] of the five 6 h steps both hold (compare_wrf_era5.py:192-206)."""
    era5_t0 = datetime.strptime(time_start, "%Y-%m-%d")
    wrf_t0 = datetime.strptime(wrf_times[0][:10], "%Y-%m-%d")
    base = (wrf_t0 - era5_t0).days * 4
    return [(base + h, h * 6, f"+{h * 6:02d}h") for h in range(5) if base + h < n_era5 and h * 6 < len(wrf_times)]


def wrf_target_offset(time_start: str, wrf_times: Sequence[str], obs_window: int):
    """(target offset or None, log lines): the sample offset whose first prediction is WRF's +06h
    (compare_wrf.py:610-667)."""
    if not time_start:
        return None, ["  WARNING: time_start not found in dataset_info.json"]
    ds_start = None
    for fmt in ("%Y-%m-%dT%H:%M:%S", "%Y-%m-%dT%H:%M", "%Y-%m-%d", "%Y-%m-%d %H:%M:%S"):
        try:
            ds_start = datetime.strptime(time_start, fmt)
            break
        except ValueError:
            continue
    if ds_start is None:
        return None, ["  WARNING: cannot parse time_start='%s'" % time_start]
    wrf_init = None
    if wrf_times:
        t_str = wrf_times[0].replace("_", "T")[:19]
        for fmt in ("%Y-%m-%dT%H:%M:%S", "%Y-%m-%dT%H:%M", "%Y-%m-%d"):
            try:
                wrf_init = datetime.strptime(t_str, fmt)
                break
            except ValueError:
                continue
    if wrf_init is None:
        return None, ["  WARNING: cannot determine WRF init time, cannot auto-detect sample"]
    first = wrf_init + timedelta(hours=6)
    target = int(round((first - ds_start).total_seconds() / (6 * 3600))) - obs_window
    return target, ["", "  [WRF date matching]",
                    "    Dataset start: %s" % ds_start.isoformat(),
                    "    WRF init:      %s" % wrf_init.isoformat(),
                    "    WRF +06h:      %s" % first.isoformat(),
                    "    Target offset: %d (need pred[0] at global time %d)" % (target, target + obs_window)]


def match_offset(sample_offsets, target: int):
    """(sample index or None, delta, log lines): the exact offset first, then -1, +1, -2, +2 (compare_wrf.py:670-685)."""
    offs = list(sample_offsets)
    for delta in MATCH_DELTAS:
        for i, off in enumerate(offs):
            if off == target + delta:
                line = ("    ✓ Found: sample #%d (offset=%d)" % (i, off) if delta == 0 else
                        "    ~ Approximate match: sample #%d (offset=%d, wanted %d)" % (i, off, target))
                return i, delta, [line]
    return None, None, ["    ✗ No matching sample found! Offsets in predictions: %s" % offs[:10],
                        "      Need offset=%d. Try: predict.py --split all" % target]


def _match_sample(time_start, wrf_times, sample_offsets, obs_window):
    target, lines = wrf_target_offset(time_start, wrf_times, obs_window)
    if target is None:
        return None, lines
    i, _, more = match_offset(sample_offsets, target)
    return i, lines + more


def find_wrf_matching_sample(data_dir, wrf_path, sample_offsets, obs_window, P=None, verbose: bool = False):
    """The index of the sample whose forecast covers the WRF run, or None (compare_wrf.py:585-685): `time_start` of the
    dataset in any of its formats, the first WRF time with `_` for `T`, target = round(steps to WRF +06h) - obs_window;
    the exact offset first, then -1, +1, -2, +2."""
    info_path = Path(data_dir) / "dataset_info.json"
    if not info_path.exists():
        lines, idx = ["  WARNING: dataset_info.json not found, cannot auto-detect WRF sample"], None
    else:
        time_start = json.loads(info_path.read_text()).get("time_start", "")
        times = []
        if Path(wrf_path).suffix == ".json":
            with open(wrf_path) as f:
                times = json.load(f).get("times", [])
        idx, lines = _match_sample(time_start, times, sample_offsets, obs_window)
    if verbose:
        print("\n".join(lines))
    return idx


_TABLES = TableCache()


def wrf_point_tables(src_lons, src_lats, wrf_lon, wrf_lat, node_of=None):
    """(pos int32 [P, 4], w float64 [P, 4]) of the WRF points on a regular source grid stored longitude-major
    (node `j * n_lat + i`): what scipy's RegularGridInterpolator((lons, lats), field, bounds_error=False,
    fill_value=nan) does with the points (lon, lat).  The axes are float64 as given (strictly ascending), the query
    points the WRF float32 coordinates widened, cells as `verify.find_cells` finds them, corners (lon, lat),
    (lon, lat+1), (lon+1, lat), (lon+1, lat+1) with weights `(1 * w_lon) * w_lat`.  A point strictly below the first or
    strictly above the last node of either axis is outside: its positions are -1 and its weights 0 (the kernels give
    NaN); a point exactly on the last node is inside, cell n-2 with weight 1.  node_of (int [n_lon * n_lat]): the
    storage row of every regular node, for a flat grid that holds the same nodes in another order.  Cached per distinct
    arguments (the 16 most recently used); the arrays are shared and read-only."""
    src_lons, src_lats = np.asarray(src_lons, dtype=np.float64), np.asarray(src_lats, dtype=np.float64)
    q_lon = np.asarray(wrf_lon).reshape(-1).astype(np.float64)
    q_lat = np.asarray(wrf_lat).reshape(-1).astype(np.float64)
    if src_lons.ndim != 1 or src_lats.ndim != 1 or q_lon.shape != q_lat.shape or q_lon.size == 0:
        raise ValueError("wrf_point_tables: the source axes must be 1-d and the WRF coordinates of one shape")
    if not (np.all(np.isfinite(q_lon)) and np.all(np.isfinite(q_lat))):
        raise ValueError("wrf_point_tables: WRF coordinates must be finite")
    n_lon, n_lat = src_lons.size, src_lats.size
    if n_lon * n_lat >= 2 ** 31:
        raise ValueError("wrf_point_tables: the source grid has too many nodes for int32 positions")
    if node_of is not None:
        node_of = np.asarray(node_of, dtype=np.int64)
        if node_of.shape != (n_lon * n_lat,) or node_of.min() < 0 or node_of.max() >= 2 ** 31:
            raise ValueError("wrf_point_tables: node_of must hold one row per regular node")
    key = tuple(None if a is None else TableCache.array_key(a) for a in (src_lons, src_lats, q_lon, q_lat, node_of))

    def make():
        ilon, ilat, w = bilinear_corners(src_lons, src_lats, q_lon, q_lat)
        outside = (q_lon < src_lons[0]) | (q_lon > src_lons[-1]) | (q_lat < src_lats[0]) | (q_lat > src_lats[-1])
        pos = np.stack([(ilon + da) * n_lat + (ilat + do) for da, do in CORNERS], axis=1)
        if node_of is not None:
            pos = node_of[pos]
        pos[outside] = -1
        w[outside] = 0.0
        return pos.astype(np.int32), w

    return _TABLES.get(key, make)


# ======================================================================================================================
# Device functions
# ======================================================================================================================
def _field_source(field, era5_lons, era5_lats, wrf_lat, wrf_lon):
    """(WrfSource, element offset) of one [n_lon, n_lat] field tensor read in place."""
    n_lon, n_lat = len(era5_lons), len(era5_lats)
    if tuple(field.shape) != (n_lon, n_lat):
        raise ValueError(f"the field is {tuple(field.shape)}, the axes say ({n_lon}, {n_lat})")
    if field.stride(1) < 1 or field.stride(0) != n_lat * field.stride(1):
        field = field.contiguous()
    pos, w = wrf_point_tables(era5_lons, era5_lats, wrf_lon, wrf_lat)
    pos_d, w_d = device_tables(pos, w, field.device)
    return hip.WrfSource(field, field.stride(1), n_lon * n_lat, pos_d, w_d), 0


def interpolate_era5_to_wrf(field_2d, era5_lons, era5_lats, wrf_lat, wrf_lon):
    """A regular-grid field [n_lon, n_lat] (float32 or fp16) on the WRF points, float64 [ny, nx], NaN outside the
    source axes (compare_wrf_era5.py:127-152).  A GPU tensor (any view with a single node stride, such as one channel
    of one time of the series) is read in place and answered with a GPU tensor; a numpy array is uploaded and answered
    with a numpy array."""
    as_numpy = not isinstance(field_2d, torch.Tensor)
    if as_numpy:
        a = np.asarray(field_2d)
        if a.dtype not in (np.float32, np.float16):
            raise TypeError(f"interpolate_era5_to_wrf takes float32 or fp16 fields, got {a.dtype}")
        if not torch.cuda.is_available():
            raise RuntimeError("interpolate_era5_to_wrf needs a GPU (there is no CPU fallback)")
        field_2d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not field_2d.is_cuda:
        raise RuntimeError("interpolate_era5_to_wrf needs a GPU tensor (there is no CPU fallback)")
    src, off = _field_source(field_2d, era5_lons, era5_lats, wrf_lat, wrf_lon)
    out = hip.wrf_sample(src, [off]).view(np.asarray(wrf_lat).shape)
    return out.cpu().numpy() if as_numpy else out


def metrics_from_stats(stats):
    """(rmse, mae, bias) of one {n, sum d, sum d^2, sum |d|, ..} record (host floats): NaN when n == 0."""
    n = float(stats[0])
    if n == 0:
        return np.nan, np.nan, np.nan
    return np.sqrt(np.float64(stats[2]) / n), np.float64(stats[3]) / n, np.float64(stats[1]) / n


def _point_arena(x, device):
    """(float32 arena or None, float64 arena or None, side kind) of one array of point values."""
    if isinstance(x, torch.Tensor):
        t = x.to(device)
    else:
        a = np.asarray(x)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if t.dtype == torch.float64:
        return None, t.contiguous().view(-1), hip.WRF_POINT64
    if t.dtype != torch.float32:
        raise TypeError(f"compute_metrics takes float32 or float64 values, got {t.dtype}")
    return t.contiguous().view(-1), None, hip.WRF_POINT


def compute_metrics(pred, truth):
    """(rmse, mae, bias) over the points where neither array is NaN; all three NaN when there is none
    (compare_wrf_era5.py:155-164).  pred / truth: float32 or float64 arrays or GPU tensors of one shape."""
    if not torch.cuda.is_available():
        raise RuntimeError("compute_metrics needs a GPU (there is no CPU fallback)")
    dev = next((x.device for x in (pred, truth) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device("cuda:0"))
    if tuple(np.shape(pred)) != tuple(np.shape(truth)) or int(np.prod(np.shape(pred))) == 0:
        raise ValueError(f"compute_metrics: pred {tuple(np.shape(pred))} and truth {tuple(np.shape(truth))}")
    a32, a64, ka = _point_arena(pred, dev)
    b32, b64, kb = _point_arena(truth, dev)
    P = int(np.prod(np.shape(pred)))
    off_b = 0
    if ka == kb:  # both in one arena
        if ka == hip.WRF_POINT:
            a32, off_b = torch.cat([a32, b32]), P
        else:
            a64, off_b = torch.cat([a64, b64]), P
    pts, pts64 = (a32 if a32 is not None else b32), (a64 if a64 is not None else b64)
    stats = hip.wrf_scores(P, [(ka, 0, kb, off_b, 0, 0)], [(1.0, 0.0, 1.0, 0.0)], pts=pts, pts64=pts64)
    return metrics_from_stats(stats[0].cpu().numpy())


# ======================================================================================================================
# WRF against ERA5 on the WRF grid (compare_wrf_era5.py:212-298)
# ======================================================================================================================
def compare_wrf_era5(wrf, era5_series, era5_lons, era5_lats, var_names, time_start: str = "2023-01-18"):
    """WRF against the ERA5 series on the WRF grid.  wrf: what `load_wrf_json` returns; era5_series: the fp16 (or
    float32) series [n_time, n_lon, n_lat, n_feat] in physical units on the GPU, read in place.  Returns (results,
    means, text): results[var][label] = (rmse, mae, bias) as the script has them, means[var][label] = (WRF mean, ERA5
    mean) over each side's own non-NaN points, text the script's output from the per-variable block on.  One
    `gcl_wrf_scores` launch scores every variable x step."""
    fields, wrf_lat, wrf_lon, times, _ = wrf
    if not era5_series.is_cuda or era5_series.dim() != 4 or not era5_series.is_contiguous():
        raise RuntimeError("compare_wrf_era5 needs the contiguous series [T, n_lon, n_lat, C] on the GPU (there is no "
                           "CPU fallback)")
    T, n_lon, n_lat, C = era5_series.shape
    if (n_lon, n_lat) != (len(era5_lons), len(era5_lats)) or C != len(var_names):
        raise ValueError(f"the series is {tuple(era5_series.shape)}; the axes say ({len(era5_lons)}, {len(era5_lats)}) "
                         f"and the variables {len(var_names)}")
    steps = match_steps(time_start, times, T)
    dev = era5_series.device
    P = int(np.asarray(wrf_lat).size)
    present = [(k, v) for k, v in VAR_MAP.items() if v["era5"] in var_names]
    lines = ["", "=" * 75, "WRF vs ERA5  —  per-variable, per-horizon RMSE on d03 domain", "=" * 75]
    results, means = {}, {}
    stats = None
    if present and steps:
        pos, w = wrf_point_tables(era5_lons, era5_lats, wrf_lon, wrf_lat)
        src = hip.WrfSource(era5_series, C, n_lon * n_lat, *device_tables(pos, w, dev))
        arena = np.stack([fields[k][wi].reshape(-1) for k, _ in present for _, wi, _ in steps]).astype(np.float32)
        jobs, conv = [], []
        for a, (k, v) in enumerate(present):
            vi = var_names.index(v["era5"])
            scale = float(v["era5_to_wrf"])
            kw = hip.WRF_POINT | (hip.WRF_CONVERT if scale != 1.0 else 0)
            for b, (ei, _, _) in enumerate(steps):
                po, fo = (a * len(steps) + b) * P, ei * n_lon * n_lat * C + vi
                jobs += [(kw, po, hip.WRF_SRC0, fo, 0, 0), (kw, po, kw, po, 0, 0),
                         (hip.WRF_SRC0, fo, hip.WRF_SRC0, fo, 0, 0)]
                conv += [(scale, 0.0, 1.0, 0.0), (scale, 0.0, scale, 0.0), (1.0, 0.0, 1.0, 0.0)]
        stats = hip.wrf_scores(P, jobs, conv, src0=src, pts=torch.from_numpy(arena).to(dev).view(-1)).cpu().numpy()
        stats = stats.reshape(len(present), len(steps), 3, 6)
    for key, v in VAR_MAP.items():
        if v["era5"] not in var_names:
            lines.append(f"  SKIP {v['era5']}: not in ERA5 dataset")
            continue
        name, unit = v["era5"], v["unit"]
        a = [k for k, _ in present].index(key)
        results[name], means[name] = {}, {}
        lines += ["", f"  {name} ({unit}):"]
        all_rmse = []
        for b, (_, _, label) in enumerate(steps):
            rmse, mae, bias = metrics_from_stats(stats[a, b, 0])
            with np.errstate(invalid="ignore", divide="ignore"):
                wrf_mean = np.float64(stats[a, b, 1, 4]) / stats[a, b, 1, 0]
                era5_mean = np.float64(stats[a, b, 2, 4]) / stats[a, b, 2, 0]
            results[name][label] = (rmse, mae, bias)
            means[name][label] = (wrf_mean, era5_mean)
            all_rmse.append(rmse)
            lines.append(f"    {label}: RMSE={rmse:.3f} {unit} | MAE={mae:.3f} | "
                         f"bias={bias:+.3f} | WRF_mean={wrf_mean:.1f} ERA5_mean={era5_mean:.1f}")
        lines.append(f"    AVG (без 0h): RMSE={_nanmean(all_rmse[1:]):.3f} {unit}")
    lines += ["", "=" * 75, "ИТОГОВАЯ ТАБЛИЦА  —  WRF RMSE vs ERA5 на домене Красноярска",
              "(для сравнения с GraphCast-lite)", "=" * 75]
    header = f"{'Переменная':<12} | {'Единица':<8}"
    for _, _, label in steps:
        header += f" | {label:>8}"
    header += f" | {'AVG':>8}"
    lines += [header, "-" * len(header)]
    for key, v in VAR_MAP.items():
        name = v["era5"]
        if name not in results:
            continue
        row = f"{name:<12} | {v['unit']:<8}"
        vals = []
        for _, _, label in steps:
            r = results[name].get(label, (np.nan, 0, 0))[0]
            row += f" | {r:>8.3f}"
            vals.append(r)
        avg = _nanmean(vals[1:]) if len(vals) > 1 else np.nan
        lines.append(row + f" | {avg:>8.3f}")
    lines += ["=" * 75, "", "Примечания:",
              "  - +00h = инициализация WRF (ожидается малая ошибка vs ERA5)",
              "  - +06h..+24h = прогноз WRF",
              "  - AVG = среднее RMSE по горизонтам +06h..+24h (без инициализации)",
              "  - PSFC сравнивается в hPa (WRF PSFC ÷ 100)",
              "  - ERA5 интерполирована билинейно на WRF-сетку d03 (96×84)"]
    return results, means, "\n".join(lines) + "\n"


def _nanmean(vals):
    vals = np.asarray(vals, dtype=np.float64)
    keep = ~np.isnan(vals)
    return np.float64(vals[keep].mean()) if keep.any() else np.float64(np.nan)


# ======================================================================================================================
# Forecast against WRF against ERA5 (compare_wrf.py:357-582)
# ======================================================================================================================
def _metrics_f32(pred, truth):
    """compare_wrf.py:348-354 on float32 vectors."""
    diff = pred - truth
    return np.sqrt(np.mean(diff ** 2)), np.mean(np.abs(diff)), np.mean(diff)


def benchmark_tables(pred_mean, truth_mean, var_names, wrf_data, wrf_si, sample_offsets, match_lines=()):
    """The text of compare_wrf.py:388-582 from the domain means [n, P, C] (float32, the reference's own numpy
    arithmetic on them): {"metrics": the all-sample block, "wrf": the three-way table of sample wrf_si or the warning,
    "summary": the summary table and the all-sample lines}.  wrf_data: what `load_wrf` returns or None; match_lines:
    what the date matching printed (it prints again inside the summary table)."""
    n_samples, P, _ = pred_mean.shape
    compare_vars = [v for v in VAR_MAPPING if v in var_names]
    unit_of = lambda var: "hPa" if var == "sp" else VAR_MAPPING[var]["unit"]  # noqa: E731
    out = ["", "=" * 70, "OUR MODEL metrics (domain-averaged, physical units)", "=" * 70]
    for var in compare_vars:
        vi = var_names.index(var)
        p_vals, t_vals = pred_mean[:, :, vi].flatten(), truth_mean[:, :, vi].flatten()
        rmse, mae, bias = _metrics_f32(p_vals, t_vals)
        out.append("  %-5s: RMSE=%.3f %s | MAE=%.3f | bias=%+.3f | mean_truth=%.1f" % (
            var, rmse, unit_of(var), mae, bias, t_vals.mean()))
        for h in range(min(P, 4)):
            r, m, b = _metrics_f32(pred_mean[:, h, vi], truth_mean[:, h, vi])
            out.append("    +%02dh: RMSE=%.3f | MAE=%.3f | bias=%+.3f" % ((h + 1) * 6, r, m, b))
    text = {"metrics": "\n".join(out) + "\n"}

    out = []
    if wrf_data:
        if wrf_si is not None and wrf_si < n_samples:
            out += ["", "=" * 70, "WRF vs ERA5 vs Ours — per-horizon (sample #%d, offset=%s)" % (
                wrf_si, sample_offsets[wrf_si] if wrf_si < len(sample_offsets) else "?"), "=" * 70]
            our_pred_h, our_truth_h = pred_mean[wrf_si], truth_mean[wrf_si]
            for var in compare_vars:
                if var not in wrf_data:
                    continue
                vi = var_names.index(var)
                wrf_vals = wrf_data[var] / 100.0 if var == "sp" else wrf_data[var]
                out += ["", "  %s (%s):" % (var, unit_of(var)),
                        "    Horizon | ERA5 truth | Our pred | WRF pred | Our err | WRF err", "    " + "-" * 65]
                our_errs, wrf_errs = [], []
                for h in range(min(P, len(wrf_vals) - 1)):
                    era5_val, our_val, wrf_val = our_truth_h[h, vi], our_pred_h[h, vi], wrf_vals[h + 1]
                    our_err, wrf_err = abs(our_val - era5_val), abs(wrf_val - era5_val)
                    our_errs.append(our_err)
                    wrf_errs.append(wrf_err)
                    winner = "<- us" if our_err < wrf_err else "<- WRF" if wrf_err < our_err else "   tie"
                    out.append("    +%02dh    | %8.2f   | %8.2f | %8.2f  | %6.2f  | %6.2f  %s" % (
                        (h + 1) * 6, era5_val, our_val, wrf_val, our_err, wrf_err, winner))
                if our_errs:
                    our_rmse = np.sqrt(np.mean(np.array(our_errs) ** 2))
                    wrf_rmse = np.sqrt(np.mean(np.array(wrf_errs) ** 2))
                    out.append("    AVG     |            |          |          | %6.2f  | %6.2f  %s" % (
                        our_rmse, wrf_rmse, "<- us" if our_rmse < wrf_rmse else "<- WRF"))
        else:
            out += ["", "WARNING: Could not find WRF-matching sample in predictions.",
                    "  Available sample offsets: %s" % list(sample_offsets),
                    "  Use --split all when running predict.py, or --wrf-sample N"]
    text["wrf"] = "\n".join(out) + "\n" if out else ""

    out = ["", "=" * 70, "SUMMARY TABLE (for thesis)", "=" * 70]
    header, sep = "%-8s | %-6s" % ("Var", "Unit"), "-" * 10
    for h in range(min(P, 4)):
        header += " | Our +%02dh | WRF +%02dh" % ((h + 1) * 6, (h + 1) * 6)
        sep += "-" * 22
    out += [header + " | Our AVG | WRF AVG", sep + "-" * 20]
    if wrf_data:
        out += list(match_lines)
    for var in compare_vars:
        vi = var_names.index(var)
        row = "%-8s | %-6s" % (var, unit_of(var))
        our_errs, wrf_errs = [], []
        for h in range(min(P, 4)):
            if wrf_data and var in wrf_data and wrf_si is not None and wrf_si < n_samples:
                era5_val, our_val = truth_mean[wrf_si, h, vi], pred_mean[wrf_si, h, vi]
                our_err = abs(our_val - era5_val)
                our_errs.append(our_err)
                wrf_vals = wrf_data[var] / 100.0 if var == "sp" else wrf_data[var]
                if h + 1 < len(wrf_vals):
                    wrf_err = abs(wrf_vals[h + 1] - era5_val)
                    wrf_errs.append(wrf_err)
                    row += " | %7.3f  | %7.3f " % (our_err, wrf_err)
                else:
                    row += " | %7.3f  |    N/A " % our_err
            else:
                our_r = _metrics_f32(pred_mean[:, h, vi], truth_mean[:, h, vi])[0]
                our_errs.append(our_r)
                row += " | %7.3f  |    N/A " % our_r
        our_avg = np.mean(our_errs) if our_errs else 0
        wrf_avg = np.mean(wrf_errs) if wrf_errs else 0
        if wrf_errs:
            row += " | %7.3f | %7.3f%s" % (our_avg, wrf_avg, " <- us" if our_avg < wrf_avg else " <- WRF")
        else:
            row += " | %7.3f |    N/A" % our_avg
        out.append(row)
    out.append("=" * 70)
    if wrf_si is not None:
        out += ["NOTE: Both Our and WRF values are for sample #%d (same WRF period)." % wrf_si,
                "      Fair comparison: same init time, same verification period."]
    out += ["", "  Our model — all %d samples (region-averaged), per-horizon:" % n_samples]
    for var in compare_vars:
        vi = var_names.index(var)
        vals = [_metrics_f32(pred_mean[:, h, vi], truth_mean[:, h, vi])[0] for h in range(min(P, 4))]
        line = "    %-5s (%s): " % (var, unit_of(var))
        line += " | ".join("+%02dh=%.3f" % ((h + 1) * 6, vals[h]) for h in range(len(vals)))
        out.append(line + " | AVG=%.3f" % np.mean(vals))
    text["summary"] = "\n".join(out) + "\n\n"
    return text


GRID_KINDS = ("ours_vs_era5", "ours_vs_wrf", "wrf_vs_era5")


def _regular_axes(lats, lons, flat_grid: bool):
    """(lon axis, lat axis, node_of or None) of the model grid: the given axes of a regular grid (float64 of the
    float32 coordinates), or the distinct coordinates of a flat grid that holds every (lon, lat) pair exactly once."""
    lats, lons = np.asarray(lats, dtype=np.float32), np.asarray(lons, dtype=np.float32)
    if not flat_grid:
        return lons.astype(np.float64), lats.astype(np.float64), None
    ulon, jl = np.unique(lons, return_inverse=True)
    ulat, il = np.unique(lats, return_inverse=True)
    reg = jl.astype(np.int64) * ulat.size + il
    if ulon.size * ulat.size != lats.size or np.unique(reg).size != lats.size:
        raise ValueError("on_wrf_grid: the flat grid's nodes do not form a complete regular lon x lat grid")
    node_of = np.empty(lats.size, dtype=np.int64)
    node_of[reg] = np.arange(lats.size)
    return ulon.astype(np.float64), ulat.astype(np.float64), node_of


class WrfBenchmark:
    """compare_wrf.py on device batches.

    mean / std: the output scalers (their first C entries are used, C = len(var_names)); lats / lons: the dataset's
    coordinates (axes of a regular grid, per-node values of a flat one); ar_steps: P.  wrf_means: what `load_wrf`
    returns (None: no WRF comparison); wrf_times and time_start (the dataset's `time_start`) locate the sample that
    matches the WRF run; wrf_fields: what `load_wrf_json` returns, needed for `on_wrf_grid`.

    `update(pred, truth, sample_offsets)` takes normalised [B, G, P * C] GPU batches and appends the WRF-box means of
    both to a device state of `capacity` samples.  With `on_wrf_grid` it also scores, per horizon and mapped variable,
    the forecast against the truth on the WRF grid for every sample and, for the sample that matches the WRF run, the
    forecast against WRF and WRF against the truth: forecast and truth are sampled from their normalised rows with the
    denormalisation as the kernel's conversion, WRF is brought to the dataset's units (psfc_Pa * 0.01); one
    `gcl_wrf_scores` launch per update, the sums in a float64 device state.  `results()` brings back the means and the
    sums and builds the reference's tables."""

    def __init__(self, mean, std, var_names: Sequence[str], lats, lons, ar_steps: int, device, flat_grid: bool = False,
                 wrf_means: Optional[dict] = None, wrf_times: Sequence[str] = (), time_start: str = "",
                 obs_window: int = 2, wrf_fields=None, on_wrf_grid: bool = False, capacity: int = 1024):
        self.var_names, self.C, self.P = list(var_names), len(var_names), int(ar_steps)
        self.K = self.P * self.C
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("WrfBenchmark needs a GPU device (there is no CPU fallback)")
        mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
        if mean.size < self.C or std.size < self.C:
            raise ValueError(f"the scalers hold {mean.size} channels, var_names {self.C}")
        if self.P < 1 or capacity < 1:
            raise ValueError(f"ar_steps={ar_steps}, capacity={capacity}")
        self.mean, self.std = mean[:self.C].copy(), std[:self.C].copy()
        lats32, lons32 = np.asarray(lats, dtype=np.float32), np.asarray(lons, dtype=np.float32)
        self.flat_grid = bool(flat_grid) or (len(lats32) == len(lons32) and len(lats32) > 512)
        self.G = len(lats32) if self.flat_grid else len(lats32) * len(lons32)
        rows = wrf_region_indices(lats32, lons32, self.flat_grid)
        if rows.size == 0:
            raise ValueError("no grid node lies inside the WRF box")
        self.region_indices = rows
        self._rows = torch.from_numpy(rows.astype(np.int32)).to(self.device)
        self._mean, self._std = torch.from_numpy(self.mean).to(self.device), torch.from_numpy(self.std).to(self.device)
        self.capacity = int(capacity)
        self._means = torch.zeros(2, self.capacity, self.K, dtype=torch.float32, device=self.device)
        self._offs = torch.zeros(self.capacity, dtype=torch.int64, device=self.device)
        self._count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._ar = torch.arange(self.capacity, dtype=torch.int64, device=self.device)
        self.n = 0  # samples taken so far (the host's copy of the device count: every update adds its batch)
        self.wrf_means, self.wrf_times = wrf_means, list(wrf_times)
        self.time_start, self.obs_window = time_start, int(obs_window)
        self.target, self._target_lines = (wrf_target_offset(time_start, self.wrf_times, self.obs_window)
                                           if wrf_means or self.wrf_times else (None, []))
        self.launches = 0
        self.on_wrf_grid = bool(on_wrf_grid)
        if self.on_wrf_grid:
            self._init_grid(lats32, lons32, wrf_fields)

    # ---- the WRF-grid scores ------------------------------------------------------------------------------------
    def _init_grid(self, lats32, lons32, wrf_fields):
        if wrf_fields is None:
            raise ValueError("on_wrf_grid needs the WRF fields (load_wrf_json)")
        fields, wrf_lat, wrf_lon = wrf_fields[0], wrf_fields[1], wrf_fields[2]
        ax_lon, ax_lat, node_of = _regular_axes(lats32, lons32, self.flat_grid)
        pos, w = wrf_point_tables(ax_lon, ax_lat, wrf_lon, wrf_lat, node_of=node_of)
        self._pos, self._w = device_tables(pos, w, self.device)
        self.Pw = int(pos.shape[0])
        self.grid_vars = [(key, v["era5"], float(v["era5_to_wrf"])) for key, v in VAR_MAP.items()
                          if v["era5"] in self.var_names]
        if not self.grid_vars:
            raise ValueError("on_wrf_grid: none of t2m, 10u, 10v, sp is among the variables")
        nt = min(len(fields[k]) for k, _, _ in self.grid_vars)
        self.grid_horizons = min(self.P, (nt - 1) // 6) if self.target is not None else 0
        arena = [fields[k][(h + 1) * 6].reshape(-1) for k, _, _ in self.grid_vars for h in range(self.grid_horizons)]
        self._pts = (torch.from_numpy(np.stack(arena).astype(np.float32)).to(self.device).view(-1) if arena else None)
        # slots: (kind, delta, horizon, variable); the WRF kinds once per offset the matching may settle on
        self.slots = [(0, 0, h, v) for h in range(self.P) for v in range(len(self.grid_vars))]
        for kind in (1, 2):
            self.slots += [(kind, d, h, v) for d in MATCH_DELTAS for h in range(self.grid_horizons)
                           for v in range(len(self.grid_vars))]
        S = len(self.slots)
        self._stats = torch.zeros(S, 6, dtype=torch.float64, device=self.device)
        self._filled = torch.zeros(S, dtype=torch.int32, device=self.device)
        self._job_cache = {}

    def _jobs(self, B: int, bs_pred: int, bs_truth: int):
        key = (B, bs_pred, bs_truth)
        hit = self._job_cache.get(key)
        if hit is None:
            jobs, conv = [], []
            grid = hip.WRF_CONVERT
            for b in range(B):
                for kind, delta, h, v in self.slots:
                    _, name, scale = self.grid_vars[v]
                    vi = self.var_names.index(name)
                    col = h * self.C + vi
                    fc = (hip.WRF_SRC0 | grid, b * bs_pred + col, float(self.std[vi]), float(self.mean[vi]))
                    tr = (hip.WRF_SRC1 | grid, b * bs_truth + col, float(self.std[vi]), float(self.mean[vi]))
                    wf = (hip.WRF_POINT | (hip.WRF_CONVERT if scale != 1.0 else 0),
                          (v * self.grid_horizons + h) * self.Pw, scale, 0.0)
                    a, c = ((fc, tr), (fc, wf), (wf, tr))[kind]
                    jobs.append((a[0], a[1], c[0], c[1], int(kind != 0), delta))
                    conv.append((a[2], a[3], c[2], c[3]))
            span = [[o for j in jobs for k, o in ((j[0], j[1]), (j[2], j[3])) if k & 3 == side] for side in (1, 2)]
            hit = self._job_cache[key] = (jobs, conv, torch.tensor(jobs, dtype=torch.int64, device=self.device),
                                          torch.tensor(conv, dtype=torch.float32, device=self.device),
                                          [(min(o), max(o)) if o else () for o in span])
        return hit

    def _score(self, pred, truth, offs):
        B = pred.shape[0]
        jobs, conv, jobs_d, conv_d, span = self._jobs(B, pred.stride(0), truth.stride(0))
        src = [hip.WrfSource(x, x.stride(1), self.G, self._pos, self._w) for x in (pred, truth)]
        for k in (0, 1):  # the job table was checked when it was built; what changes is the buffer behind it
            src[k].check_offsets(span[k], "WrfBenchmark.update")
        hip.wrf_scores(self.Pw, jobs, conv, jobs_d, conv_d, src0=src[0], src1=src[1], pts=self._pts,
                       slots=len(self.slots), offsets=offs, target=self.target if self.target is not None else 0,
                       filled=self._filled, accumulate=True, out=self._stats, validated=True)
        self.launches += 1

    # ---- updates --------------------------------------------------------------------------------------------------
    def _check_batch(self, pred, truth):
        for name, x in (("pred", pred), ("truth", truth)):
            if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32:
                raise RuntimeError(f"WrfBenchmark.update needs float32 GPU batches (there is no CPU fallback): {name}")
            if x.dim() != 3 or x.shape[1] != self.G or x.shape[2] != self.K or x.stride(2) != 1:
                raise ValueError(f"{name} must be [B, {self.G}, {self.K}] with unit column stride, got {tuple(x.shape)}")
        if pred.shape[0] != truth.shape[0] or pred.shape[0] == 0:
            raise ValueError(f"pred holds {pred.shape[0]} samples, truth {truth.shape[0]}")

    def _offsets_tensor(self, sample_offsets, B: int):
        if isinstance(sample_offsets, torch.Tensor):
            offs = sample_offsets.to(self.device, torch.int64).contiguous()
        else:
            offs = torch.tensor([int(o) for o in sample_offsets], dtype=torch.int64).to(self.device)
        if offs.shape != (B,):
            raise ValueError(f"{B} samples with {tuple(offs.shape)} offsets")
        return offs

    def _device_update(self, pred, truth, offs, truth_scalers=None):
        """Everything an update launches: two box means at the device count, the scores, the count.  truth_scalers:
        (std, mean) of the truth side when they are not the forecast's."""
        B = pred.shape[0]
        t_std, t_mean = truth_scalers if truth_scalers is not None else (self._std, self._mean)
        for k, (x, sd, mu) in enumerate(((pred, self._std, self._mean), (truth, t_std, t_mean))):
            # (rows come from the mask over this grid's coordinates: in range by construction)
            hip.wrf_box_means(x, self._rows, self.G, sd, mu, out=self._means[k], count=self._count, validated=True)
        self.launches += 2
        idx = (self._count + self._ar[:B]).clamp_(max=self.capacity - 1)
        self._offs.scatter_(0, idx, offs)
        if self.on_wrf_grid:
            self._score(pred, truth, offs)
        self._count.add_(B)

    def _update(self, pred, truth, offs):
        self._device_update(pred, truth, offs)

    def update(self, pred, truth, sample_offsets, truth_is_physical: bool = False):
        """Take one batch: pred / truth normalised float32 [B, G, P * C] on the GPU, sample_offsets B ints (or an
        int64 tensor).  truth_is_physical: the truth is in physical units already (a legacy bundle's, rebuilt from the
        series): its box mean is taken with the scalers (1, 0) - x * 1 + 0 leaves the float32 bits - in eager launches,
        and the WRF-grid scores are not available."""
        self._check_batch(pred, truth)
        B = pred.shape[0]
        if self.n + B > self.capacity:
            raise ValueError(f"the state holds {self.capacity} samples; {self.n} are taken and {B} more arrive")
        offs = self._offsets_tensor(sample_offsets, B)
        if truth_is_physical:
            if self.on_wrf_grid:
                raise NotImplementedError("on_wrf_grid with a legacy bundle (truth from data.npy) is not provided")
            self._device_update(pred, truth, offs, (torch.ones_like(self._std), torch.zeros_like(self._mean)))
        else:
            self._update(pred, truth, offs)
        self.n += B

    # ---- results --------------------------------------------------------------------------------------------------
    def results(self, wrf_sample: Optional[int] = None) -> dict:
        """Bring back the [n, P, C] means and the sums and build the tables.  wrf_sample forces the sample compared
        with WRF (the script's --wrf-sample); by default it is found from the dates."""
        n = self.n
        means = self._means[:, :n].cpu().numpy().reshape(2, n, self.P, self.C)
        offsets = [int(o) for o in self._offs[:n].cpu().numpy()]
        pred_mean, truth_mean = means[0], means[1]
        wrf_si, delta, lines = wrf_sample, None, []
        if wrf_sample is None:
            lines = list(self._target_lines)
            if self.target is not None:
                wrf_si, delta, more = match_offset(offsets, self.target)
                lines += more
        elif self.target is not None and 0 <= wrf_sample < n:
            # the WRF-grid sums belong to the first sample at an offset; a forced sample has them only if it is that one
            d = offsets[wrf_sample] - self.target
            delta = d if d in MATCH_DELTAS and offsets.index(offsets[wrf_sample]) == wrf_sample else None
        if not self.wrf_means:
            lines = []
        text = benchmark_tables(pred_mean, truth_mean, self.var_names, self.wrf_means, wrf_si, offsets, lines)
        out = {"pred_mean": pred_mean, "truth_mean": truth_mean, "sample_offsets": offsets, "wrf_sample": wrf_si,
               "n_samples": n, "match_lines": lines, "text": text}
        if self.on_wrf_grid:
            out.update(self._grid_results(delta))
        return out

    def _grid_results(self, delta):
        """grid_stats[kind][(variable, horizon)] = the six sums; the WRF kinds are those of the matched offset."""
        stats = self._stats.cpu().numpy()
        grid = {k: {} for k in GRID_KINDS}
        for s, (kind, d, h, v) in enumerate(self.slots):
            if kind == 0 or (delta is not None and d == delta):
                grid[GRID_KINDS[kind]][(self.grid_vars[v][1], h)] = stats[s]
        lines = ["", "=" * 70, "FIELD-LEVEL scores on the WRF grid (RMSE | MAE | bias, dataset units)", "=" * 70]
        for _, name, _ in self.grid_vars:
            unit = "hPa" if name == "sp" else VAR_MAPPING[name]["unit"]
            lines += ["", "  %s (%s):" % (name, unit)]
            for h in range(self.P):
                row = "    +%02dh" % ((h + 1) * 6)
                for kind in GRID_KINDS:
                    st = grid[kind].get((name, h))
                    if st is None:
                        row += " | %-13s        N/A" % kind
                    else:
                        r, m, b = metrics_from_stats(st)
                        row += " | %s %.3f %.3f %+.3f (n=%d)" % (kind, r, m, b, int(st[0]))
                lines.append(row)
        return {"grid_stats": grid, "grid_text": "\n".join(lines) + "\n"}

    # ---- bundles --------------------------------------------------------------------------------------------------
    @classmethod
    def from_bundle(cls, data_dir, pred_path, ar_steps: int = 4, wrf_path=None, device="cuda:0", batch_size: int = 8,
                    on_wrf_grid: bool = False, captured: bool = False):
        """The benchmark of a dataset directory and a `predictions.pt` (compare_wrf.py:58-205, :373-386), already fed
        with every sample.  The bundle is the dictionary `predict.save_predictions` writes or the legacy bare tensor,
        whose truth is rebuilt from the regular-grid series `data.npy` (:171-196; the physical values are normalised
        again so that one path serves both)."""
        from . import predict

        data_dir = Path(data_dir)
        sc = np.load(data_dir / "scalers.npz")
        if "mean" in sc:
            mean, std = sc["mean"].astype(np.float32), sc["std"].astype(np.float32)
        elif "y_mean" in sc:
            mean, std = sc["y_mean"].astype(np.float32), sc["y_scale"].astype(np.float32)
        else:
            raise ValueError("Expected scalers with 'mean'/'std' or 'y_mean'/'y_scale'")
        var_names = json.loads((data_dir / "variables.json").read_text())
        coords = np.load(data_dir / "coords.npz")
        lons, lats = coords["longitude"].astype(np.float32), coords["latitude"].astype(np.float32)
        info_path = data_dir / "dataset_info.json"
        info = json.loads(info_path.read_text()) if info_path.exists() else {}
        flat_grid = bool(info.get("flat_grid", info.get("flat", False)))
        bundle = predict.load_predictions(pred_path)
        is_dict = isinstance(bundle, dict) and "predictions" in bundle
        preds = bundle["predictions"] if is_dict else bundle
        truth = bundle["ground_truth"] if is_dict else None
        C = bundle.get("n_features", len(var_names)) if is_dict else len(var_names)
        if preds.dim() == 2:
            preds = preds.unsqueeze(0)
        if truth is not None and truth.dim() == 2:
            truth = truth.unsqueeze(0)
        n, G = preds.shape[0], preds.shape[1]
        P = preds.shape[2] // C
        physical_truth = False
        if truth is None:
            if not info or flat_grid or (len(lats) == len(lons) and len(lats) > 512):
                raise RuntimeError("No ground truth available: predictions.pt has no 'ground_truth' key "
                                   "and dataset_info.json not found or flat_grid=True")
            shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
            data = np.memmap(str(data_dir / "data.npy"), dtype=np.float16, mode="r", shape=shape)
            flat = data.reshape(shape[0], shape[1] * shape[2], shape[3])
            obs_w = 2
            total = shape[0] - obs_w - ar_steps + 1
            split = int(total * 0.8)
            test_all = total - split
            val = test_all // 2
            start = split + val
            n = min(n, test_all - val)
            truth4 = np.zeros((n, G, P, C), dtype=np.float32)
            for i in range(n):
                for p in range(P):
                    t = start + i + obs_w + p
                    if t < shape[0]:
                        truth4[i, :, p, :] = flat[t].astype(np.float32)
            truth, preds, physical_truth = torch.from_numpy(truth4.reshape(n, G, P * C)), preds[:n], True
        offsets = bundle.get("sample_offsets", list(range(n))) if is_dict else list(range(n))
        obs_window = bundle.get("obs_window", 2) if is_dict else 2
        wrf_means = wrf_fields = None
        times = []
        if wrf_path is not None:
            wrf_means = load_wrf(wrf_path, P)
            with open(wrf_path) as f:
                times = json.load(f).get("times", [])
            if on_wrf_grid:
                wrf_fields = load_wrf_json(wrf_path)
        klass = CapturedWrfBenchmark if captured else cls
        bench = klass(mean, std, var_names[:C] if C < len(var_names) else var_names, lats, lons, P, device,
                      flat_grid=flat_grid, wrf_means=wrf_means, wrf_times=times, time_start=info.get("time_start", ""),
                      obs_window=obs_window, wrf_fields=wrf_fields, on_wrf_grid=on_wrf_grid, capacity=max(n, 1))
        if not info_path.exists() and wrf_means:
            bench.target, bench._target_lines = None, ["  WARNING: dataset_info.json not found, cannot auto-detect "
                                                      "WRF sample"]
        for s in range(0, n, batch_size):
            p = preds[s:s + batch_size].to(device, torch.float32).contiguous()
            t = truth[s:s + batch_size].to(device, torch.float32).contiguous()
            bench.update(p, t, list(offsets[s:s + batch_size]), truth_is_physical=physical_truth)
        return bench


class CapturedWrfBenchmark(WrfBenchmark, Captured):
    """`WrfBenchmark` whose update (two box means, the scores, the count) is replayed from a hipGraph
    (capture.Captured): the first two updates of a shape run eagerly, the third captures, later ones copy their inputs
    into the captured buffers and replay.  The means, the sums and the sample count are device state, so a replay
    counts like an eager update and gives the same bits.  Falls back to eager launches if capture is not possible (see
    `.launch_mode`)."""

    def __init__(self, *args, use_graph: bool = True, **kw):
        WrfBenchmark.__init__(self, *args, **kw)
        Captured.__init__(self, use_graph=use_graph, recapture=True)

    def _work(self, pred, truth, offs):
        self._device_update(pred, truth, offs)

    def _update(self, pred, truth, offs):
        self._run(pred, truth, offs)
