"""The live forecast on the HIP path: drop-in for `scripts/live_gdas_forecast.py` and
`scripts/export_live_runtime_bundle.py` from the decoded analysis fields on.

* Host helpers with the reference's names and results: `cycle_floor_6h`, `cycle_label`, `load_scalers`,
  `get_var_order`, `load_coords`, `load_template_static` (and their `*_from_bundle` variants), `load_runtime_assets`,
  `export_bundle`, `normalize_frame`, `denormalize_prediction`, `build_city_mask`, `summarize_city`,
  `forecast_valid_times`.
* `point_tables`: what `build_interpolator` + `interp_to_nodes` (`:378-407`) make scipy do, as four positions and four
  float64 weights per node (host, cached per distinct axes and node list).
* `LiveFramePacker`: one cycle's fields -> one or more normalised window slots, one launch (`gcl_live_frame_pack`).
* `LiveForecaster`: `forecast` (pack, `predict.CapturedRollout`, `pipeline.denormalize`, MOS, city box) and `hindcast`
  (an archive of past cycles in one batched rollout, every cycle interpolated once).

Finding, downloading and decoding GRIB and the t2m plot are not provided: the input is plain arrays keyed by the
model's variable names.  `AnalysisFields` is a mapping `name -> (values[nlat, nlon], lats, lons)`; values are float32
numpy arrays or device tensors in the source's own orientation, and different variables may sit on different axes.

Kernels: csrc/live.hip.
"""
import json
from datetime import datetime, timedelta
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import hip, mos, pipeline, predict
from .interp_tables import CORNERS, TableCache, bilinear_corners

CITY_BBOX = (55.5, 56.5, 92.0, 94.0)

DEFAULT_VAR_ORDER = [
    "t2m", "10u", "10v", "msl", "tp",
    "sp", "tcwv",
    "z_surf", "lsm",
    "t@850", "u@850", "v@850", "z@850", "q@850",
    "t@500", "u@500", "v@500", "z@500", "q@500",
]

# the names extract_live_channels (:440-458) knows how to find in an analysis
SUPPORTED_VARS = frozenset(
    ["t2m", "10u", "10v", "msl", "sp", "tcwv", "tp"] + [f"{v}@{p}" for p in (850, 500) for v in "tuvzq"])
PRESSURE_IN_PA = frozenset(["msl", "sp"])  # scaled to hPa (:480-481)
STATIC_NAMES = ("z_surf", "lsm")
SUMMARY_VARS = (("t2m", "C"), ("10u", "m/s"), ("10v", "m/s"), ("msl", "hPa"))  # :547-558
_BUNDLE_FILES = ("coords.npz", "scalers.npz", "variables.json")

AnalysisFields = Dict[str, Tuple[object, object, object]]


# ======================================================================================================================
# Cycles and valid times (:108-121, :661-664)
# ======================================================================================================================
def cycle_floor_6h(dt_utc: datetime) -> datetime:
    """The 00 / 06 / 12 / 18 UTC cycle at or before dt_utc."""
    return dt_utc.replace(hour=6 * (dt_utc.hour // 6), minute=0, second=0, microsecond=0)


def cycle_label(cycle_dt: datetime) -> str:
    return cycle_dt.strftime("%Y%m%d_%H")


def forecast_valid_times(last_cycle: datetime, ar_steps: int) -> List[datetime]:
    """Valid time of every forecast step: 6 h apart, the first 6 h after the last input cycle."""
    return [last_cycle + timedelta(hours=6 * (s + 1)) for s in range(ar_steps)]


# ======================================================================================================================
# Dataset directory / runtime bundle (:212-375, export_live_runtime_bundle.py:31-97)
# ======================================================================================================================
def _variables_json(folder: Path) -> List[str]:
    p = Path(folder) / "variables.json"
    if not p.exists():
        return list(DEFAULT_VAR_ORDER)
    with p.open("r", encoding="utf-8") as fh:
        return json.load(fh)


def get_var_order(data_dir) -> List[str]:
    return _variables_json(data_dir)


def get_var_order_from_bundle(bundle_dir) -> List[str]:
    return _variables_json(bundle_dir)


def load_scalers(data_dir):
    """(x_mean, x_std, y_mean, y_std), float32; a `mean` / `std` file serves both sides."""
    z = np.load(Path(data_dir) / "scalers.npz")
    if "mean" in z:
        m, s = z["mean"].astype(np.float32), z["std"].astype(np.float32)
        return m, s, m, s
    return tuple(z[k].astype(np.float32) for k in ("x_mean", "x_scale", "y_mean", "y_scale"))


def load_coords(data_dir):
    z = np.load(Path(data_dir) / "coords.npz")
    return z["latitude"].astype(np.float32), z["longitude"].astype(np.float32)


def load_coords_from_bundle(bundle_dir):
    """(latitude, longitude, is_regional or None)."""
    z = np.load(Path(bundle_dir) / "coords.npz")
    return (z["latitude"].astype(np.float32), z["longitude"].astype(np.float32),
            z["is_regional"] if "is_regional" in z else None)


def _first_frame_statics(data_dir: Path, info: dict, var_order) -> Dict[str, np.ndarray]:
    """z_surf / lsm of the first frame of the fp16 series `data.npy`, per node, float32."""
    flat = bool(info.get("flat", False))
    shape = ((info["n_time"], info["n_nodes"], info["n_feat"]) if flat
             else (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"]))
    series = np.memmap(str(Path(data_dir) / "data.npy"), dtype=np.float16, mode="r", shape=shape)
    names = info.get("variables", var_order)
    out = {}
    for name in STATIC_NAMES:
        if name in names:
            out[name] = series[0, ..., names.index(name)].astype(np.float32).reshape(-1)
    return out


def load_template_static(data_dir, var_order) -> Dict[str, np.ndarray]:
    data_dir = Path(data_dir)
    info_path = data_dir / "dataset_info.json"
    if not info_path.exists() or not (data_dir / "data.npy").exists():
        return {}
    return _first_frame_statics(data_dir, json.loads(info_path.read_text(encoding="utf-8")), var_order)


def load_template_static_from_bundle(bundle_dir) -> Dict[str, np.ndarray]:
    p = Path(bundle_dir) / "static_fields.npz"
    if not p.exists():
        return {}
    z = np.load(p)
    return {name: z[name].astype(np.float32) for name in z.files}


def _metadata(latitudes, longitudes, is_regional) -> dict:
    return {"flat_grid": True, "num_grid_nodes": len(latitudes),
            "cordinates": (latitudes.astype(np.float32), longitudes.astype(np.float32)), "is_regional": is_regional}


def load_runtime_assets(data_dir, runtime_bundle_dir, obs_window: int, pred_window: int):
    """(x_mean, x_std, y_mean, y_std, var_order, latitudes, longitudes, template_static, metadata) from a runtime bundle
    (which wins) or a dataset directory.  metadata is a dict with `flat_grid`, `num_grid_nodes`, `cordinates` and
    `is_regional` in place of the reference's DatasetMetadata."""
    if runtime_bundle_dir is not None:
        bundle = Path(runtime_bundle_dir)
        for name in _BUNDLE_FILES:
            if not (bundle / name).exists():
                raise FileNotFoundError(f"Missing runtime bundle file: {bundle / name}")
        scalers = load_scalers(bundle)
        var_order = get_var_order_from_bundle(bundle)
        lat, lon, is_regional = load_coords_from_bundle(bundle)
        statics = load_template_static_from_bundle(bundle)
        missing = [n for n in STATIC_NAMES if n in var_order and n not in statics]
        if missing:
            raise FileNotFoundError("Runtime bundle is incomplete: missing static fields "
                                    f"{missing} in {bundle / 'static_fields.npz'}")
        return (*scalers, var_order, lat, lon, statics, _metadata(lat, lon, is_regional))
    if data_dir is None:
        raise ValueError("data_dir must be provided when runtime_bundle_dir is not set")
    data_dir = Path(data_dir)
    for name in _BUNDLE_FILES:
        if not (data_dir / name).exists():
            raise FileNotFoundError(f"Missing dataset file: {data_dir / name}")
    scalers = load_scalers(data_dir)
    var_order = get_var_order(data_dir)
    lat, lon = load_coords(data_dir)
    statics = load_template_static(data_dir, var_order)
    z = np.load(data_dir / "coords.npz")
    is_regional = z["is_regional"] if "is_regional" in z else None
    return (*scalers, var_order, lat, lon, statics, _metadata(lat, lon, is_regional))


def export_bundle(data_dir, out_dir) -> None:
    """The lightweight runtime bundle of a dataset directory: coords.npz, scalers.npz, variables.json,
    static_fields.npz and bundle_meta.json."""
    data_dir, out_dir = Path(data_dir), Path(out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    for name in _BUNDLE_FILES + ("dataset_info.json", "data.npy"):
        if not (data_dir / name).exists():
            raise FileNotFoundError(f"Missing required dataset file: {data_dir / name}")
    info = json.loads((data_dir / "dataset_info.json").read_text(encoding="utf-8"))
    coords = np.load(data_dir / "coords.npz")
    scalers = np.load(data_dir / "scalers.npz")
    var_order = _variables_json(data_dir)

    cz = {"latitude": coords["latitude"].astype(np.float32), "longitude": coords["longitude"].astype(np.float32)}
    if "is_regional" in coords:
        cz["is_regional"] = coords["is_regional"]
    np.savez_compressed(out_dir / "coords.npz", **cz)
    keys = ("mean", "std") if "mean" in scalers else ("x_mean", "x_scale", "y_mean", "y_scale")
    np.savez_compressed(out_dir / "scalers.npz", **{k: scalers[k].astype(np.float32) for k in keys})
    (out_dir / "variables.json").write_text(json.dumps(var_order, ensure_ascii=False, indent=2), encoding="utf-8")
    statics = _first_frame_statics(data_dir, info, var_order)
    np.savez_compressed(out_dir / "static_fields.npz", **statics)
    meta = {"flat_grid": bool(info.get("flat", False)),
            "n_nodes": int(info.get("n_nodes", len(coords["latitude"]))),
            "n_feat": int(info["n_feat"]),
            "variables": var_order,
            "static_fields": sorted(statics)}
    (out_dir / "bundle_meta.json").write_text(json.dumps(meta, ensure_ascii=False, indent=2), encoding="utf-8")


# ======================================================================================================================
# Host arithmetic and the summary (:486-501, :530-560)
# ======================================================================================================================
def normalize_frame(frame: np.ndarray, x_mean: np.ndarray, x_std: np.ndarray) -> np.ndarray:
    return (frame - x_mean[None, :]) / x_std[None, :]


def denormalize_prediction(prediction: np.ndarray, y_mean: np.ndarray, y_std: np.ndarray) -> np.ndarray:
    return prediction * y_std[None, None, :] + y_mean[None, None, :]


def build_city_mask(latitudes: np.ndarray, longitudes: np.ndarray, city_bbox=CITY_BBOX) -> np.ndarray:
    lat0, lat1, lon0, lon1 = city_bbox
    return (latitudes >= lat0) & (latitudes <= lat1) & (longitudes >= lon0) & (longitudes <= lon1)


def summarize_city(out_path, prediction_phys: np.ndarray, latitudes: np.ndarray, longitudes: np.ndarray,
                   var_order: Sequence[str], cycles: Sequence[datetime], warnings: Sequence[str],
                   city_bbox=CITY_BBOX) -> None:
    """summary.txt: input cycles, warnings and, when the city box holds a node, mean / min / max of t2m (deg C), 10u,
    10v and msl per horizon."""
    mask = build_city_mask(latitudes, longitudes, city_bbox)
    lines = ["# GDAS Live Forecast", "", "Input cycles:"]
    lines += [f"- {c.isoformat()}" for c in cycles]
    lines += ["", "Warnings:"]
    lines += [f"- {w}" for w in warnings] if warnings else ["- none"]
    lines.append("")
    if mask.sum() > 0:
        lines.append("City-area means:")
        for s in range(prediction_phys.shape[1]):
            lines.append(f"- Horizon +{(s + 1) * 6}h")
            for name, unit in SUMMARY_VARS:
                if name not in var_order:
                    continue
                v = prediction_phys[:, s, list(var_order).index(name)][mask]
                if name == "t2m":
                    v = v - 273.15
                lines.append(f"  {name}: mean={v.mean():.2f} {unit} min={v.min():.2f} max={v.max():.2f}")
    Path(out_path).write_text("\n".join(lines) + "\n", encoding="utf-8")


# ======================================================================================================================
# Point tables (:378-407)
# ======================================================================================================================
MAX_CACHED_TABLES = 16  # a key holds copies of its axes and node lists, a value 48 bytes per node
_TABLES = TableCache(MAX_CACHED_TABLES)


def point_tables(src_lats, src_lons, node_lats, node_lons):
    """(pos int32 [G, 4], w float64 [G, 4]): for every node the positions `row * nlon + col` of its four corners in a
    source field [nlat, nlon] stored as the source stores it, and their bilinear weights - what scipy's
    RegularGridInterpolator does with the reference's interpolator: the source axes as float32, longitudes % 360, both
    axes sorted, the wrap column `lons_sorted[0] + 360` appended (it maps back to the first sorted column), query
    points (float32 lat, float32(mod(lon, 360))), cells found as `verify.find_cells` finds them (points past the last
    latitude extrapolate), corners (lat, lon), (lat, lon+1), (lat+1, lon), (lat+1, lon+1) with weights
    `(1 * w_lat) * w_lon`.  Cached per distinct axes and node list (the MAX_CACHED_TABLES most recently used); the arrays
    are shared and read-only."""
    src_lats, src_lons = np.asarray(src_lats), np.asarray(src_lons)
    node_lats, node_lons = np.asarray(node_lats), np.asarray(node_lons)
    if src_lats.ndim != 1 or src_lons.ndim != 1 or node_lats.ndim != 1 or node_lats.shape != node_lons.shape:
        raise ValueError("point_tables: the source axes and the node coordinates must be 1-d (nodes of equal length)")
    key = tuple(TableCache.array_key(a) for a in (src_lats, src_lons, node_lats, node_lons))

    def make():
        lats = np.asarray(src_lats, dtype=np.float32)
        lons = np.asarray(src_lons, dtype=np.float32) % 360.0
        lat_order, lon_order = np.argsort(lats), np.argsort(lons)
        lats_sorted, lons_sorted = lats[lat_order], lons[lon_order]
        ext_lons = np.concatenate([lons_sorted, [lons_sorted[0] + 360.0]])
        col_of = np.concatenate([lon_order, lon_order[:1]])  # the wrap column is the first sorted column again
        q_lat = node_lats.astype(np.float32)
        q_lon = np.mod(node_lons, 360.0).astype(np.float32)
        if not (np.all(np.isfinite(q_lat)) and np.all(np.isfinite(q_lon))):
            raise ValueError("point_tables: node coordinates must be finite")
        ilat, ilon, w = bilinear_corners(lats_sorted, ext_lons, q_lat, q_lon)
        nlon = lons.size
        pos = np.stack([lat_order[ilat + da].astype(np.int64) * nlon + col_of[ilon + do] for da, do in CORNERS], axis=1)
        if pos.size and (pos.min() < 0 or pos.max() >= lats.size * nlon or lats.size * nlon >= 2 ** 31):
            raise ValueError("point_tables: a corner position lies outside the source field")
        return pos.astype(np.int32), w

    return _TABLES.get(key, make)


# ======================================================================================================================
# One cycle -> window slots
# ======================================================================================================================
def cycle_warnings(var_order: Sequence[str], static_names: Sequence[str], fields) -> List[str]:
    """The warning strings of `extract_live_channels` (:460-483) for one cycle, in its order: a name that the template
    statics supply never warns, a name outside `var_specs` is unsupported, an absent one is missing (tp with its own
    message)."""
    out = []
    for name in var_order:
        if name in static_names:
            continue
        if name not in SUPPORTED_VARS:
            out.append(f"Unsupported variable {name}; filling zeros")
        elif name not in fields:
            out.append("GDAS analysis does not expose tp in this path; filling zeros" if name == "tp"
                       else f"Missing {name} in GDAS payload; filling zeros")
    return out


class LiveFramePacker:
    """Writes one analysis cycle into normalised window slots with one launch.

    var_order: the model's channel names; node_lats / node_lons: per node (G,); x_mean / x_std: the input scalers
    (their first len(var_order) entries are used); template_static: name -> per-node values that replace the analysis
    (z_surf, lsm).  Everything that does not change between cycles (scalers, statics, point tables, the channel table
    of a payload layout) is uploaded once; a cycle's fields go to the device once, in one arena."""

    def __init__(self, var_order: Sequence[str], node_lats, node_lons, x_mean, x_std, template_static, device):
        self.var_order = list(var_order)
        self.node_lats, self.node_lons = np.asarray(node_lats), np.asarray(node_lons)
        if self.node_lats.ndim != 1 or self.node_lats.shape != self.node_lons.shape or self.node_lats.size == 0:
            raise ValueError("node_lats and node_lons must be 1-d arrays of the same, non-zero length")
        self.G, self.C = int(self.node_lats.size), len(self.var_order)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LiveFramePacker needs a GPU device (there is no CPU fallback)")
        x_mean, x_std = np.asarray(x_mean, dtype=np.float32), np.asarray(x_std, dtype=np.float32)
        if x_mean.size < self.C or x_std.size < self.C:
            raise ValueError(f"the scalers hold {x_mean.size} channels, var_order {self.C}")
        self._mean = torch.from_numpy(x_mean[:self.C].copy()).to(self.device)
        self._std = torch.from_numpy(x_std[:self.C].copy()).to(self.device)
        self.static_names = [n for n in self.var_order if n in template_static]
        rows = []
        for n in self.static_names:
            v = np.asarray(template_static[n]).astype(np.float32).reshape(-1)
            if v.size != self.G:
                raise ValueError(f"template static {n} has {v.size} values for {self.G} nodes")
            rows.append(v)
        self._statics = torch.from_numpy(np.stack(rows)).to(self.device) if rows else None
        self._div = torch.tensor([100.0 if n in PRESSURE_IN_PA and n not in self.static_names else 1.0
                                  for n in self.var_order], dtype=torch.float32).to(self.device)
        self._plans = {}  # payload layout -> (chan table, pos, w) on the device
        self.launches = 0

    def _plan(self, present, fields):
        """The device tables of a payload layout: which names are present, on which axes."""
        axes, layout = [], []
        for name in present:
            values, lats, lons = fields[name]
            lats, lons = np.asarray(lats), np.asarray(lons)
            if tuple(values.shape) != (lats.size, lons.size):
                raise ValueError(f"{name}: values {tuple(values.shape)} do not match the axes ({lats.size}, {lons.size})")
            layout.append((name, TableCache.array_key(lats), TableCache.array_key(lons)))
            axes.append((lats, lons))
        key = tuple(layout)
        hit = self._plans.get(key)
        if hit is not None:
            return hit
        offs, off = {}, 0  # arena offsets, in the order the fields are laid down
        for name, (lats, lons) in zip(present, axes):
            offs[name] = off
            off += lats.size * lons.size
        slot = {name: i for i, name in enumerate(present)}
        tab_of, tabs = {}, []
        chan = np.zeros((self.C, 3), dtype=np.int64)  # (absent and unsupported names stay zero fill)
        for c, name in enumerate(self.var_order):
            if name in self.static_names:
                chan[c] = (2, self.static_names.index(name), 0)
            elif name in slot:
                lk = layout[slot[name]][1:]
                if lk not in tab_of:
                    tab_of[lk] = len(tabs)
                    tabs.append(point_tables(*axes[slot[name]], self.node_lats, self.node_lons))
                chan[c] = (1, offs[name], tab_of[lk])
        pos = w = None
        if tabs:
            # every position of a table was validated against its field's size by point_tables
            pos = torch.from_numpy(np.stack([t[0] for t in tabs])).to(self.device)
            w = torch.from_numpy(np.stack([t[1] for t in tabs])).to(self.device)
        hit = self._plans[key] = (torch.from_numpy(chan).to(self.device), pos, w, off)
        return hit

    def _arena(self, present, fields, total: int):
        vals = [fields[n][0] for n in present]
        if not vals:
            return None
        if all(isinstance(v, np.ndarray) for v in vals):
            host = np.empty(total, dtype=np.float32)
            o = 0
            for v in vals:
                host[o:o + v.size] = np.asarray(v, dtype=np.float32).reshape(-1)
                o += v.size
            return torch.from_numpy(host).to(self.device)
        return torch.cat([(v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float32)))
                          .to(self.device, torch.float32).reshape(-1) for v in vals])

    def _offsets(self, out, dests):
        obs_c = out.shape[-1]
        if out.dim() not in (2, 3) or out.shape[-2] != self.G or obs_c % self.C or out.stride(-1) != 1:
            raise ValueError(f"out must be [G, obs * C] or [B, G, obs * C] with unit column stride, got {tuple(out.shape)}")
        obs = obs_c // self.C
        offs = []
        for d in dests:
            b, slot = d if isinstance(d, (tuple, list)) else (None, d)
            if (b is None) != (out.dim() == 2) or not 0 <= slot < obs or (b is not None and not 0 <= b < out.shape[0]):
                raise ValueError(f"destination {d!r} does not name a slot of a window {tuple(out.shape)}")
            offs.append((0 if b is None else b * out.stride(0)) + slot * self.C)
        return offs

    def pack(self, fields: AnalysisFields, out: torch.Tensor, dests) -> List[str]:
        """Interpolate, convert, normalise and store one cycle into every slot of `dests`: slot numbers for a window
        out [G, obs * C], (sample, slot) pairs for a batch [B, G, obs * C] (row stride out.stride(-2), so padded and
        offset windows work).  Returns the reference's warning strings in its order."""
        if not out.is_cuda or out.dtype != torch.float32:
            raise RuntimeError("LiveFramePacker.pack needs a float32 GPU window (there is no CPU fallback)")
        warnings = cycle_warnings(self.var_order, self.static_names, fields)
        present = [n for n in self.var_order if n in fields and n in SUPPORTED_VARS and n not in self.static_names]
        present = list(dict.fromkeys(present))
        chan, pos, w, total = self._plan(present, fields)
        arena = self._arena(present, fields, total)
        hip.live_frame_pack(arena, self._statics, chan, self._div, pos, w, self._mean, self._std, out,
                            self._offsets(out, dests), out.stride(-2), self.G, self.C)
        self.launches += 1
        return warnings


# ======================================================================================================================
# The forecast
# ======================================================================================================================
def hindcast_windows(frames, anchors, obs_window: int) -> List[List[int]]:
    """The frame indices of every anchor's window (the anchor is its last cycle).  ValueError for no anchors, a repeated
    anchor, an anchor whose window reaches before frames[0] or past the end, and window frames that are not 6 h
    apart."""
    six = timedelta(hours=6)
    anchors = [int(a) for a in anchors]
    if not anchors:
        raise ValueError("hindcast: no anchors")
    if len(set(anchors)) != len(anchors):
        raise ValueError("hindcast: an anchor is listed more than once")
    wins = []
    for a in anchors:
        if not 0 <= a < len(frames) or a - obs_window + 1 < 0:
            raise ValueError(f"anchor {a}: its window of {obs_window} cycles does not lie inside the {len(frames)} frames")
        idx = list(range(a - obs_window + 1, a + 1))
        for i, k in zip(idx, idx[1:]):
            if frames[k][0] - frames[i][0] != six:
                raise ValueError(f"anchor {a}: frames {i} and {k} are not 6 h apart")
        wins.append(idx)
    return wins


class LiveForecaster:
    """Analysis fields -> corrected forecast, everything after the host tables on the device.

    model: a one-step model of this package (`obs_window`, called as `model(X=..., attention_threshold=...)`); scalers:
    (x_mean, x_std, y_mean, y_std); mos_table: the dict of `mos.load_mos_table`; learned_mos: a `mos.LearnedMOS`, a
    `mos.MOSForest`, the bundle dict of `mos.load_learned_mos` or the fitted model (it wins over the table, :666-692).
    With `use_graph` the rollout is a `predict.CapturedRollout` (one per batch size), else `predict.rollout`."""

    def __init__(self, model, var_order: Sequence[str], node_lats, node_lons, scalers, template_static, ar_steps: int,
                 use_residual: bool, mos_table: Optional[dict] = None, learned_mos=None, city_bbox=CITY_BBOX,
                 use_graph: bool = True):
        self.model, self.var_order = model, list(var_order)
        self.latitudes, self.longitudes = np.asarray(node_lats), np.asarray(node_lons)
        self.ar_steps, self.use_residual, self.use_graph = int(ar_steps), bool(use_residual), bool(use_graph)
        self.obs_window = int(model.obs_window)
        self.device = next(model.parameters()).device
        x_mean, x_std, y_mean, y_std = scalers
        self.G, self.C = int(self.latitudes.size), len(self.var_order)
        model_nodes = getattr(model, "_num_grid_nodes", None)
        if model_nodes is not None and int(model_nodes) != self.G:
            raise ValueError(f"{self.G} node coordinates for a model of {int(model_nodes)} grid nodes")
        if self.obs_window > hip.live_max_dest():
            raise ValueError(f"obs_window {self.obs_window}: one pack launch fills at most {hip.live_max_dest()} slots")
        self.packer = LiveFramePacker(self.var_order, self.latitudes, self.longitudes, x_mean, x_std, template_static,
                                      self.device)
        self._y_mean = torch.from_numpy(np.asarray(y_mean, dtype=np.float32)[:self.C].copy()).to(self.device)
        self._y_std = torch.from_numpy(np.asarray(y_std, dtype=np.float32)[:self.C].copy()).to(self.device)
        self.mos_table = mos_table
        if learned_mos is not None and not isinstance(learned_mos, mos.LearnedMOS):
            learned_mos = mos.LearnedMOS(learned_mos, self.var_order, self.latitudes, self.longitudes,
                                         device=self.device)
        self.learned_mos = learned_mos
        self.city_bbox = tuple(city_bbox)
        rows = np.nonzero(build_city_mask(self.latitudes, self.longitudes, self.city_bbox))[0]
        self.city_names = [n for n, _ in SUMMARY_VARS if n in self.var_order]
        self._city_rows = self._city_chans = self._city_offs = None
        if rows.size and self.city_names:
            self._city_rows = torch.from_numpy(rows.astype(np.int32)).to(self.device)
            self._city_chans = torch.tensor([self.var_order.index(n) for n in self.city_names],
                                            dtype=torch.int32).to(self.device)
            self._city_offs = torch.tensor([-273.15 if n == "t2m" else 0.0 for n in self.city_names],
                                           dtype=torch.float32).to(self.device)
        self._rollouts = {}

    @property
    def graph_active(self) -> bool:
        """True while some batch size's rollout is replayed from a captured hipGraph."""
        return any(r.graph_active for r in self._rollouts.values())

    def _rollout(self, X3: torch.Tensor) -> torch.Tensor:
        if not self.use_graph:
            return predict.rollout(self.model, X3, self.ar_steps, use_residual=self.use_residual)
        r = self._rollouts.get(X3.shape[0])
        if r is None:
            r = self._rollouts[X3.shape[0]] = predict.CapturedRollout(self.model, self.ar_steps,
                                                                      use_residual=self.use_residual)
        return r(X3)

    def _post(self, X3: torch.Tensor, valid_times):
        """Rollout, denormalise, MOS and the city box of a packed batch X3 [B, G, obs * C]; valid_times: one list per
        sample."""
        B = X3.shape[0]
        norm = self._rollout(X3).view(B, self.G, self.ar_steps, self.C)
        phys = pipeline.denormalize(norm, self._y_mean, self._y_std)
        mos_applied = learned_applied = False
        if self.learned_mos is not None:
            if self.learned_mos.has_t2m:
                tfeat = self.learned_mos.time_features(valid_times)
                phys, _ = self.learned_mos.apply(phys, tfeat, out=torch.empty_like(phys))
            learned_applied = True
        elif self.mos_table is not None:
            phys = mos.apply_mos_t2m(phys, self.var_order, self.mos_table, valid_times)
            mos_applied = True
        stats = None
        if self._city_rows is not None:
            # (rows come from the mask over this G's coordinates, channels from var_order: in range by construction)
            stats = hip.live_region_stats(phys, self._city_rows, self._city_chans, self._city_offs, validated=True)
        return norm, phys, stats, mos_applied, learned_applied

    def _city(self, stats):
        return None if stats is None else {"names": list(self.city_names), "rows": int(self._city_rows.numel()),
                                           "stats": stats}

    def forecast(self, cycles) -> dict:
        """cycles: obs_window pairs (datetime, AnalysisFields), oldest first.  Returns the reference's payload (:694-709)
        with device tensors - `input_normalized` [G, obs * C], `prediction_normalized` / `prediction_physical`
        [G, steps, C] - plus `city_stats`: None when the city box holds no node, else {"names", "rows", "stats"
        float64 [steps, len(names), 3] = mean, min, max (t2m in deg C)}."""
        cycles = list(cycles)
        if len(cycles) != self.obs_window:
            raise ValueError(f"forecast needs {self.obs_window} cycles, got {len(cycles)}")
        X = torch.empty(1, self.G, self.obs_window * self.C, dtype=torch.float32, device=self.device)
        warnings = []
        for j, (dt, fields) in enumerate(cycles):
            warnings += [f"{dt.isoformat()}: {line}" for line in self.packer.pack(fields, X[0], [j])]
        times = [forecast_valid_times(cycles[-1][0], self.ar_steps)]
        norm, phys, stats, mos_applied, learned_applied = self._post(X, times)
        return {"cycles": [dt.isoformat() for dt, _ in cycles], "var_names": self.var_order,
                "latitudes": self.latitudes, "longitudes": self.longitudes, "input_normalized": X[0],
                "prediction_normalized": norm[0], "prediction_physical": phys[0], "warnings": warnings,
                "mos_applied": mos_applied, "learned_mos_applied": learned_applied,
                "city_stats": self._city(stats[0] if stats is not None else None)}

    def hindcast(self, frames, anchors) -> dict:
        """Re-forecast past cycles in one batched rollout.  frames: time-ordered (datetime, AnalysisFields) at 6 h
        spacing; anchors: indices into it, each the LAST input cycle of one forecast.  Every distinct cycle is
        interpolated once and written into every window slot that needs it; an anchor may be listed once.  Returns `forecast`'s payload with a
        leading batch axis: tensors [B, G, ..], `cycles` / `warnings` one list per anchor, `city_stats["stats"]`
        [B, steps, names, 3]."""
        frames = list(frames)
        wins = hindcast_windows(frames, anchors, self.obs_window)
        B = len(wins)
        X = torch.empty(B, self.G, self.obs_window * self.C, dtype=torch.float32, device=self.device)
        dests = {}
        for b, idx in enumerate(wins):
            for slot, f in enumerate(idx):
                dests.setdefault(f, []).append((b, slot))
        # distinct anchors: a cycle fills at most obs_window slots, which one launch takes (checked in __init__)
        lines = {f: self.packer.pack(frames[f][1], X, dests[f]) for f in sorted(dests)}
        warnings = [[f"{frames[f][0].isoformat()}: {line}" for f in idx for line in lines[f]] for idx in wins]
        times = [forecast_valid_times(frames[idx[-1]][0], self.ar_steps) for idx in wins]
        norm, phys, stats, mos_applied, learned_applied = self._post(X, times)
        return {"anchors": [idx[-1] for idx in wins],
                "cycles": [[frames[f][0].isoformat() for f in idx] for idx in wins], "var_names": self.var_order,
                "latitudes": self.latitudes, "longitudes": self.longitudes, "input_normalized": X,
                "prediction_normalized": norm, "prediction_physical": phys, "warnings": warnings,
                "mos_applied": mos_applied, "learned_mos_applied": learned_applied, "city_stats": self._city(stats)}


# ======================================================================================================================
# Output files (:694-713)
# ======================================================================================================================
def _host(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x


def save_forecast(payload: dict, path, experiment_dir=None, checkpoint=None, data_dir=None, runtime_bundle=None) -> None:
    """forecast.pt with the reference's keys: lists, flags and host numpy arrays (`torch.save`).  The four provenance
    strings of the reference's command line are the keyword arguments (None when not given)."""
    out = {"cycles": list(payload["cycles"]), "var_names": list(payload["var_names"]),
           "latitudes": np.asarray(payload["latitudes"]), "longitudes": np.asarray(payload["longitudes"]),
           "input_normalized": _host(payload["input_normalized"]),
           "prediction_normalized": _host(payload["prediction_normalized"]),
           "prediction_physical": _host(payload["prediction_physical"]), "warnings": list(payload["warnings"]),
           "experiment_dir": None if experiment_dir is None else str(experiment_dir),
           "checkpoint": None if checkpoint is None else str(checkpoint),
           "data_dir": None if data_dir is None else str(data_dir),
           "runtime_bundle": None if runtime_bundle is None else str(runtime_bundle),
           "mos_applied": bool(payload["mos_applied"]), "learned_mos_applied": bool(payload["learned_mos_applied"])}
    torch.save(out, str(path))


def write_summary(payload: dict, path, city_bbox=CITY_BBOX) -> None:
    """summary.txt of a `forecast` payload through `summarize_city` on the host copy of the physical forecast."""
    phys = _host(payload["prediction_physical"])
    if phys.ndim != 3:
        raise ValueError("write_summary takes a forecast() payload ([G, steps, C]); index a hindcast by anchor first")
    summarize_city(path, phys, np.asarray(payload["latitudes"]), np.asarray(payload["longitudes"]),
                   payload["var_names"], [datetime.fromisoformat(c) for c in payload["cycles"]], payload["warnings"],
                   city_bbox)
