"""MOS (model output statistics) correction of 2 m temperature on the HIP path: drop-in for
`src/postprocessing/mos_correction.py`.

* `load_mos_table`, `get_t2m_bias`, `apply_mos_t2m` (`:18-69`): the per-(month, hour) bias table.  The lookup is on the
  host; the add runs on the device (`gcl_mos_table_apply`).
* `load_learned_mos` (`:93-95`): joblib, as in the reference (sklearn is needed only to unpickle the bundle); an
  `.npz` written by `save_learned_mos` loads without sklearn.
* `MOSForest`: the bundle's `HistGradientBoostingRegressor` flattened for the device; `save` / `load` keep it in an npz
  so a machine without sklearn can run it.
* `apply_learned_mos_t2m` (`:244-340`) with the reference's signature and return convention: `(corrected,
  n_corrected)` when `t2m` is present, the input itself otherwise.  `LearnedMOS` prepares the station groups, the
  forest and the IDW points once; its `apply` neither synchronises nor allocates after the first call, and
  `CapturedLearnedMOS` replays it from a hipGraph.

Predictions are device tensors `[G, steps, C]` or `[B, G, steps, C]`, float32 or float64, in physical units (t2m in
Kelvin).  Coordinates are host arrays.  The host-side features (valid time and station) are computed with Python's
`math` exactly as the reference computes them and uploaded as one small float64 tensor, so new valid times need no
re-capture.

Fitting (scripts/build_learned_mos.py:203-266, :313-315, :332, :340-467): `training_table`, `fit_mos_table`,
`MOSFitter` / `fit_learned_mos` (the histogram gradient boosting of `HistGradientBoostingRegressor.fit` on the device,
sklearn-free), `evaluate_learned_mos`, `save_learned_mos`.

Kernels: csrc/mos.hip, csrc/mos_fit.hip.
"""
import json
import math
from datetime import datetime
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured, graph_enabled

NUM_FEATURES = 20  # FEATURE_COLUMNS of the reference's build_learned_mos.py
NUM_TIME_FEATURES = 8  # hour sin/cos, doy sin/cos, solar elevation, station lat/lon/elev
MAX_POINTS = 128  # station groups and stations per group (csrc/mos.hip kMaxPoints)
_ALT_NAMES = {"u10": "10u", "10u": "u10", "v10": "10v", "10v": "v10"}
DEFAULT_STATION = {"lat": 56.173, "lon": 92.493, "elev": 287.0, "name": "default"}
# The (idw_power, idw_max_radius_km, label) grid of scripts/mos_idw_sweep_v2.py:192-203 (mos_idw_sweep.py:164-176 has the
# same ten in another order); the first is the reference's default.
IDW_SWEEP_CONFIGS = (
    (2.0, 300.0, "p2.0_r300"), (2.0, 200.0, "p2.0_r200"), (2.0, 150.0, "p2.0_r150"), (2.0, 100.0, "p2.0_r100"),
    (2.0, 50.0, "p2.0_r50"), (3.0, 300.0, "p3.0_r300"), (3.0, 150.0, "p3.0_r150"), (3.0, 100.0, "p3.0_r100"),
    (1.5, 300.0, "p1.5_r300"), (1.5, 150.0, "p1.5_r150"))


# ======================================================================================================================
# Table MOS (mos_correction.py:18-69)
# ======================================================================================================================
def load_mos_table(path) -> dict:
    """The bias table JSON as a dict."""
    with open(path, "r", encoding="utf-8") as f:
        return json.load(f)


def get_t2m_bias(mos_table: dict, valid_time: datetime) -> float:
    """The additive t2m correction (degC) for a UTC valid time: `bias_table[month][hour]`, 0.0 when either key is
    missing."""
    return mos_table["bias_table"].get(str(valid_time.month), {}).get(str(valid_time.hour), 0.0)


# ======================================================================================================================
# Learned MOS: the forest
# ======================================================================================================================
def load_learned_mos(path) -> dict:
    """The learned-MOS bundle (a dict with the fitted model under "model"): an `.npz` of `save_learned_mos` (the model
    is a `MOSForest`, no sklearn needed), anything else unpickled with joblib as in the reference."""
    if str(path).endswith(".npz"):
        z = np.load(path)
        bundle = json.loads(str(z["bundle_json"]))
        bundle["model"] = MOSForest(*(z[k] for k in MOSForest._FIELDS), float(z["baseline"]), int(z["n_features"]))
        return bundle
    import joblib

    return joblib.load(path)


class MOSForest:
    """A `HistGradientBoostingRegressor` as flat arrays: per node `feature`, `value` (threshold of a split, value of a
    leaf), `left`, `right` (indices into the whole forest), `missing_left`, `is_leaf`; `roots[t]` is tree t's first
    node; `baseline` the model's baseline prediction.  `to(device)` packs the nodes into the kernels' 16-byte layout."""

    _FIELDS = ("feature", "value", "left", "right", "missing_left", "is_leaf", "roots")

    def __init__(self, feature, value, left, right, missing_left, is_leaf, roots, baseline: float,
                 n_features: int = NUM_FEATURES):
        self.feature = np.ascontiguousarray(feature, dtype=np.int32)
        self.value = np.ascontiguousarray(value, dtype=np.float64)
        self.left = np.ascontiguousarray(left, dtype=np.int64)
        self.right = np.ascontiguousarray(right, dtype=np.int64)
        self.missing_left = np.ascontiguousarray(missing_left, dtype=np.uint8)
        self.is_leaf = np.ascontiguousarray(is_leaf, dtype=np.uint8)
        self.roots = np.ascontiguousarray(roots, dtype=np.int32)
        self.baseline = float(baseline)
        self.n_features = int(n_features)
        self._validate()
        self._dev = {}

    def _validate(self):
        n = self.value.shape[0]
        if n == 0 or n >= (1 << 24):
            raise ValueError(f"MOSForest: {n} nodes (1 .. 2^24 - 1 supported)")
        if self.n_features > 32:
            raise ValueError(f"MOSForest: {self.n_features} features (at most 32)")
        for a in (self.feature, self.left, self.right, self.missing_left, self.is_leaf):
            if a.shape != (n,):
                raise ValueError("MOSForest: node arrays of different lengths")
        split = self.is_leaf == 0
        idx = np.arange(n)
        # children come after their parent: every walk ends at a leaf
        if np.any((self.left[split] <= idx[split]) | (self.right[split] <= idx[split])
                  | (self.left[split] >= n) | (self.right[split] >= n)):
            raise ValueError("MOSForest: a split's children must follow it in the node array")
        if np.any((self.feature[split] < 0) | (self.feature[split] >= self.n_features)):
            raise ValueError("MOSForest: split feature outside the feature vector")
        if self.roots.size == 0 or np.any((self.roots < 0) | (self.roots >= n)):
            raise ValueError("MOSForest: bad tree roots")

    @property
    def num_trees(self) -> int:
        return int(self.roots.size)

    @property
    def num_nodes(self) -> int:
        return int(self.value.size)

    @classmethod
    def from_sklearn(cls, model) -> "MOSForest":
        """Flatten a fitted `HistGradientBoostingRegressor`.  Raises ValueError for categorical splits, more than one
        tree per iteration (classifiers with several classes) and a loss whose link is not the identity."""
        if getattr(model, "n_trees_per_iteration_", 1) != 1:
            raise ValueError(f"MOSForest: {model.n_trees_per_iteration_} trees per iteration (only 1 is supported)")
        link = getattr(getattr(model, "_loss", None), "link", None)
        if link is None or type(link).__name__ != "IdentityLink":
            raise ValueError(f"MOSForest: loss link {type(link).__name__} is not the identity")
        if getattr(model, "_preprocessor", None) is not None or (
                getattr(model, "is_categorical_", None) is not None and np.any(model.is_categorical_)):
            raise ValueError("MOSForest: categorical features are not supported")
        cols = {k: [] for k in ("feature", "value", "left", "right", "missing_left", "is_leaf")}
        roots, off = [], 0
        for it in model._predictors:
            nodes = it[0].nodes
            if np.any(nodes["is_categorical"]):
                raise ValueError("MOSForest: categorical splits are not supported")
            leaf = nodes["is_leaf"].astype(np.uint8)
            roots.append(off)
            cols["feature"].append(np.where(leaf, 0, nodes["feature_idx"]))
            cols["value"].append(np.where(leaf, nodes["value"], nodes["num_threshold"]))
            cols["left"].append(np.where(leaf, 0, nodes["left"].astype(np.int64) + off))
            cols["right"].append(np.where(leaf, 0, nodes["right"].astype(np.int64) + off))
            cols["missing_left"].append(nodes["missing_go_to_left"])
            cols["is_leaf"].append(leaf)
            off += len(nodes)
        base = np.asarray(model._baseline_prediction, dtype=np.float64).reshape(-1)
        return cls(*(np.concatenate(cols[k]) for k in cols), np.asarray(roots), float(base[0]),
                   n_features=int(model.n_features_in_))

    def save(self, path):
        np.savez_compressed(path, baseline=np.float64(self.baseline), n_features=np.int32(self.n_features),
                            **{k: getattr(self, k) for k in self._FIELDS})

    @classmethod
    def load(cls, path) -> "MOSForest":
        z = np.load(path)
        return cls(*(z[k] for k in cls._FIELDS), float(z["baseline"]), int(z["n_features"]))

    def predict_host(self, X: np.ndarray) -> np.ndarray:
        """The same forest walked with numpy on the host (a restatement for checks; the product path is
        `predict`)."""
        X = np.asarray(X, dtype=np.float64)
        out = np.full(X.shape[0], self.baseline)
        rows = np.arange(X.shape[0])
        for r in self.roots:
            node = np.full(X.shape[0], r, dtype=np.int64)
            active = self.is_leaf[node] == 0
            while active.any():
                a = node[active]
                x = X[rows[active], self.feature[a]]
                go_left = np.where(np.isnan(x), self.missing_left[a] != 0, x <= self.value[a])
                node[active] = np.where(go_left, self.left[a], self.right[a])
                active = self.is_leaf[node] == 0
            out = out + self.value[node]
        return out

    def to(self, device):
        """(packed nodes uint8 [N * 16], roots int32) on `device`, uploaded once per device."""
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            packed = np.zeros(self.num_nodes, dtype=[("v", "<f8"), ("a", "<u4"), ("b", "<u4")])
            packed["v"] = self.value
            packed["a"] = self.left.astype(np.uint32)
            packed["b"] = (self.right.astype(np.uint32) | (self.feature.astype(np.uint32) << 24)
                           | (self.missing_left.astype(np.uint32) << 29) | (self.is_leaf.astype(np.uint32) << 30))
            nodes = torch.from_numpy(packed.view(np.uint8).copy()).to(device)
            roots = torch.from_numpy(self.roots.copy()).to(device)
            t = self._dev[key] = (nodes, roots)
        return t

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """sklearn's `predict` on float64 device rows X [n, 20] (gcl_mos_forest_eval)."""
        if not X.is_cuda:
            raise RuntimeError("MOSForest.predict needs a GPU tensor (there is no CPU fallback)")
        if X.dim() != 2 or X.shape[1] != NUM_FEATURES:
            raise ValueError(f"MOSForest.predict: X must be [n, {NUM_FEATURES}], got {tuple(X.shape)}")
        X = X.to(torch.float64).contiguous()
        nodes, roots = self.to(X.device)
        y = torch.empty(X.shape[0], dtype=torch.float64, device=X.device)
        hip._check(hip.lib().gcl_mos_forest_eval(nodes.data_ptr(), roots.data_ptr(), self.num_trees, self.baseline,
                                                 X.data_ptr(), X.shape[0], y.data_ptr(), hip._stream()))
        return y


_FORESTS = {}


def _forest_of(forest_or_bundle) -> MOSForest:
    """A MOSForest from a MOSForest, a bundle dict or a fitted model; flattened once per model object."""
    if isinstance(forest_or_bundle, MOSForest):
        return forest_or_bundle
    model = forest_or_bundle["model"] if isinstance(forest_or_bundle, dict) else forest_or_bundle
    if isinstance(model, MOSForest):  # a device-fitted bundle (save_learned_mos / MOSFit.bundle)
        return model
    hit = _FORESTS.get(id(model))
    if hit is None or hit[0] is not model:
        hit = _FORESTS[id(model)] = (model, MOSForest.from_sklearn(model))
    return hit[1]


# ======================================================================================================================
# Host features (mos_correction.py:74-90, :152-160, :172)
# ======================================================================================================================
def solar_elevation(lat_deg: float, lon_deg: float, dt: datetime) -> float:
    """Solar elevation in degrees after Spencer (1971), in the reference's operation order."""
    doy = dt.timetuple().tm_yday
    hour = dt.hour + dt.minute / 60.0
    g = 2 * math.pi * (doy - 1) / 365.0
    decl = (0.006918 - 0.399912 * math.cos(g) + 0.070257 * math.sin(g)
            - 0.006758 * math.cos(2 * g) + 0.000907 * math.sin(2 * g))
    eqt = 229.18 * (0.000075 + 0.001868 * math.cos(g) - 0.032077 * math.sin(g)
                    - 0.014615 * math.cos(2 * g) - 0.04089 * math.sin(2 * g))
    ha = math.radians((hour * 60 + eqt + 4 * lon_deg) / 4.0 - 180.0)
    la = math.radians(lat_deg)
    s = math.sin(la) * math.sin(decl) + math.cos(la) * math.cos(decl) * math.cos(ha)
    return math.degrees(math.asin(max(-1.0, min(1.0, s))))


def time_station_features(valid_time: datetime, st: dict) -> list:
    """The 8 host features of one (station, valid time): hour sin/cos, day-of-year sin/cos, solar elevation, station
    lat / lon / elev (features 9-13 and 17-19 of the reference's vector)."""
    h = valid_time.hour
    doy = valid_time.timetuple().tm_yday
    return [math.sin(2 * math.pi * h / 24), math.cos(2 * math.pi * h / 24),
            math.sin(2 * math.pi * doy / 365.25), math.cos(2 * math.pi * doy / 365.25),
            solar_elevation(st["lat"], st["lon"], valid_time), float(st["lat"]), float(st["lon"]),
            float(st["elev"])]


def group_stations(stations: Sequence[dict], latitudes, longitudes):
    """Map each station to its nearest grid index (the reference's squared-degree argmin, in the coordinates' own
    dtype) and group the stations that share one.  Returns `[(grid_idx, [station, ...]), ...]` in first-seen order."""
    lat, lon = np.asarray(latitudes), np.asarray(longitudes)
    groups = {}
    for st in stations:
        gi = int(np.argmin((lat - st["lat"]) ** 2 + (lon - st["lon"]) ** 2))
        groups.setdefault(gi, []).append(st)
    return list(groups.items())


def _channel(var_order: Sequence[str], name: str) -> int:
    if name in var_order:
        return list(var_order).index(name)
    alt = _ALT_NAMES.get(name)
    if alt is not None and alt in var_order:
        return list(var_order).index(alt)
    return -1


def _as4(pred: torch.Tensor, who: str) -> torch.Tensor:
    if not isinstance(pred, torch.Tensor) or not pred.is_cuda:
        raise RuntimeError(f"{who} needs a GPU tensor (there is no CPU fallback)")
    if pred.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: prediction must be float32 or float64, got {pred.dtype}")
    if pred.dim() not in (3, 4):
        raise ValueError(f"{who}: prediction must be [G, steps, C] or [B, G, steps, C], got {tuple(pred.shape)}")
    p4 = pred if pred.dim() == 4 else pred.unsqueeze(0)
    if p4.stride(3) != 1:
        p4 = p4.contiguous()
    return p4


def _times_2d(valid_times, B: int):
    """valid_times as B lists (one list, or one per sample)."""
    vt = list(valid_times)
    if vt and isinstance(vt[0], (list, tuple)):
        if len(vt) != B:
            raise ValueError(f"{len(vt)} lists of valid times for a batch of {B}")
        return [list(v) for v in vt]
    return [vt] * B


# ======================================================================================================================
# Table MOS on the device
# ======================================================================================================================
def apply_mos_t2m(prediction_phys: torch.Tensor, var_order: list, mos_table: dict, forecast_valid_times):
    """`corrected[..., s, t2m] += get_t2m_bias(mos_table, valid_times[s])` for the first len(valid_times) steps, in the
    reference's arithmetic (float32 input: f32(x + f32(bias)); float64: exact adds).  Returns a new tensor, or the
    input itself when `t2m` is not in var_order.  `forecast_valid_times` may be one list per sample for a batch."""
    if "t2m" not in var_order:
        return prediction_phys
    p4 = _as4(prediction_phys, "apply_mos_t2m")
    B, G, S, C = p4.shape
    times = _times_2d(forecast_valid_times, B)
    n = len(times[0])
    if any(len(t) != n for t in times) or n > S:
        raise IndexError(f"{n} valid times for {S} forecast steps")
    out = torch.empty(p4.shape, dtype=p4.dtype, device=p4.device)
    if n == 0 or p4.numel() == 0:  # (an empty view has a null data_ptr(), which the C entry point refuses)
        out.copy_(p4)
        return out if prediction_phys.dim() == 4 else out[0]
    t2m = list(var_order).index("t2m")
    f64 = int(p4.dtype == torch.float64)
    shared = all(ts is times[0] for ts in times)
    parts = [(p4, out, times[0])] if shared else [(p4[b:b + 1], out[b:b + 1], times[b]) for b in range(B)]
    for src, dst, ts in parts:  # one launch per bias vector
        tb = torch.tensor([get_t2m_bias(mos_table, t) for t in ts], dtype=torch.float64).to(p4.device)
        hip._check(hip.lib().gcl_mos_table_apply(
            src.data_ptr(), f64, src.stride(0), src.stride(1), src.stride(2), dst.data_ptr(), dst.stride(0),
            dst.stride(1), dst.stride(2), G, S, C, t2m, tb.data_ptr(), n, src.shape[0], hip._stream()))
    return out if prediction_phys.dim() == 4 else out[0]


# ======================================================================================================================
# Learned MOS on the device
# ======================================================================================================================
class LearnedMOS:
    """The learned-MOS correction of one station set on one grid, prepared once.

    forest_or_bundle: a `MOSForest`, the bundle dict of `load_learned_mos` or the fitted model.  stations: list of
    {"lat", "lon", "elev"} dicts (None: the reference's single default station).  latitudes / longitudes: per grid node
    (G,).  With `spatial_idw` and at least two distinct station grid points the biases are spread to every node by
    inverse-distance weighting (`power`, `radius` km); otherwise only the station grid points change.

    `time_features(valid_times)` builds the float64 device tensor of the host features; `apply(pred, tfeat)` runs
    the two kernels.  After the first call per shape `apply` neither synchronises nor allocates: its bias, count and
    (when `out` is not given) output buffers are reused by the next call."""

    def __init__(self, forest_or_bundle, var_order: Sequence[str], latitudes, longitudes,
                 stations: Optional[Sequence[dict]] = None, spatial_idw: bool = False, power: float = 2.0,
                 radius: float = 300.0, device=None):
        self.var_order = list(var_order)
        self.has_t2m = "t2m" in self.var_order
        self.forest = _forest_of(forest_or_bundle)
        if self.forest.n_features != NUM_FEATURES:
            raise ValueError(f"the learned MOS model takes {self.forest.n_features} features, not {NUM_FEATURES}")
        self.latitudes, self.longitudes = np.asarray(latitudes), np.asarray(longitudes)
        if self.latitudes.shape != self.longitudes.shape or self.latitudes.ndim != 1:
            raise ValueError("latitudes and longitudes must be 1-d arrays of the same length (one entry per node)")
        self.stations = [dict(DEFAULT_STATION)] if stations is None else list(stations)
        if not self.stations:
            raise ValueError("LearnedMOS: no stations")
        self.groups = group_stations(self.stations, self.latitudes, self.longitudes)
        if len(self.groups) > MAX_POINTS or max(len(g[1]) for g in self.groups) > MAX_POINTS:
            raise ValueError(f"LearnedMOS: at most {MAX_POINTS} station grid points and {MAX_POINTS} stations each")
        self.grid_idx = [g for g, _ in self.groups]
        self.ordered_stations = [st for _, sts in self.groups for st in sts]
        self.idw = bool(spatial_idw) and len(self.groups) >= 2
        self.power, self.radius = float(power), float(radius)
        self.chans = tuple(_channel(self.var_order, n) for n in ("t2m", "u10", "v10", "sp", "tp"))
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        dev = self.device
        self._nodes, self._roots = self.forest.to(dev)
        self._gidx = torch.tensor(self.grid_idx, dtype=torch.int32, device=dev)
        starts = np.cumsum([0] + [len(s) for _, s in self.groups]).astype(np.int32)
        self._gstart = torch.from_numpy(starts).to(dev)
        self._lat = torch.from_numpy(self.latitudes.astype(np.float64)).to(dev)
        self._lon = torch.from_numpy(self.longitudes.astype(np.float64)).to(dev)
        self._bufs = {}
        self._sweep_cfg = {}  # config list -> [(power, radius) device tensors per launch]

    @property
    def num_points(self) -> int:
        return len(self.groups)

    def time_features(self, valid_times) -> torch.Tensor:
        """float64 device tensor [B, stations, steps, 8] of the host features; valid_times is [steps] (B = 1) or one
        list per sample."""
        vt = list(valid_times)
        per_sample = [list(v) for v in vt] if vt and isinstance(vt[0], (list, tuple)) else [vt]
        arr = np.array([[[time_station_features(t, st) for t in ts] for st in self.ordered_stations]
                        for ts in per_sample], dtype=np.float64)
        return torch.from_numpy(arr).to(self.device)

    def _buffers(self, B: int, S: int, dtype, shape, with_out: bool):
        key = (B, S)
        bufs = self._bufs.get(key)
        if bufs is None:
            bufs = self._bufs[key] = {
                "bias": torch.empty(B, self.num_points, S, dtype=torch.float64, device=self.device),
                "n": torch.zeros(B, dtype=torch.int32, device=self.device)}
        if with_out:
            o = bufs.get(("out", dtype, tuple(shape)))
            if o is None:
                o = bufs[("out", dtype, tuple(shape))] = torch.empty(shape, dtype=dtype, device=self.device)
            return bufs, o
        return bufs, None

    def apply(self, pred: torch.Tensor, tfeat: torch.Tensor, out: Optional[torch.Tensor] = None,
              inplace: bool = False, feat_out: Optional[torch.Tensor] = None):
        """(corrected, n_corrected int32 device tensor [B]) for pred [G, steps, C] / [B, G, steps, C]; pred itself
        and None when t2m is absent.  `out` receives the result (same shape and dtype); `inplace` corrects pred.
        `feat_out` (float64 [B, stations, steps, 20], optional) receives the station features (for checks)."""
        if not self.has_t2m:
            return pred, None
        p4 = _as4(pred, "LearnedMOS.apply")
        if inplace and p4.data_ptr() != pred.data_ptr():
            raise ValueError("LearnedMOS.apply(inplace=True) needs a prediction with unit channel stride")
        B, G, S, C = p4.shape
        if G != self.latitudes.shape[0]:
            raise ValueError(f"prediction has {G} grid rows, the coordinates {self.latitudes.shape[0]}")
        if C != len(self.var_order):
            raise ValueError(f"prediction has {C} channels, var_order {len(self.var_order)}")
        if tfeat.shape != (B, len(self.ordered_stations), S, NUM_TIME_FEATURES) or tfeat.dtype != torch.float64 \
                or not tfeat.is_cuda or not tfeat.is_contiguous():
            raise ValueError(f"tfeat must be contiguous float64 [{B}, {len(self.ordered_stations)}, {S}, "
                             f"{NUM_TIME_FEATURES}] on the device (time_features), got {tuple(tfeat.shape)}")
        if inplace:
            o4, bufs = p4, self._buffers(B, S, p4.dtype, p4.shape, False)[0]
        elif out is not None:
            if out.shape != pred.shape or out.dtype != pred.dtype or not out.is_cuda:
                raise ValueError("out must match the prediction's shape, dtype and device")
            o4 = out if out.dim() == 4 else out.unsqueeze(0)
            if o4.stride(3) != 1:
                raise ValueError("out needs unit channel stride")
            bufs = self._buffers(B, S, p4.dtype, p4.shape, False)[0]
        else:
            bufs, o4 = self._buffers(B, S, p4.dtype, p4.shape, True)
        if feat_out is not None:
            assert feat_out.shape == (B, len(self.ordered_stations), S, NUM_FEATURES) and feat_out.is_contiguous()
            assert feat_out.dtype == torch.float64 and feat_out.is_cuda
        f64 = int(p4.dtype == torch.float64)
        L, st = hip.lib(), hip._stream()
        bias, ncorr = bufs["bias"], bufs["n"]
        hip._check(L.gcl_mos_forest_predict(
            self._nodes.data_ptr(), self._roots.data_ptr(), self.forest.num_trees, self.forest.baseline,
            p4.data_ptr(), f64, p4.stride(0), p4.stride(1), p4.stride(2), S, *self.chans, self._gidx.data_ptr(),
            self._gstart.data_ptr(), self.num_points, len(self.ordered_stations), tfeat.data_ptr(), bias.data_ptr(),
            feat_out.data_ptr() if feat_out is not None else None, ncorr.data_ptr(), B, st))
        hip._check(L.gcl_mos_idw_apply(
            p4.data_ptr(), f64, p4.stride(0), p4.stride(1), p4.stride(2), o4.data_ptr(), o4.stride(0), o4.stride(1),
            o4.stride(2), G, S, C, self.chans[0], self._lat.data_ptr(), self._lon.data_ptr(), self._gidx.data_ptr(),
            self.num_points, bias.data_ptr(), int(self.idw), self.power, self.radius, ncorr.data_ptr(), B, st))
        res = pred if inplace else (out if out is not None else (o4 if pred.dim() == 4 else o4[0]))
        return res, ncorr

    def _sweep_configs(self, configs):
        """The (power, radius) device tensors of a config list, one pair per chunk of at most the kernel's cap,
        uploaded at first use."""
        key = tuple((float(c[0]), float(c[1])) for c in configs)
        if not key:
            raise ValueError("LearnedMOS.sweep: no settings")
        cache = self._sweep_cfg
        hit = cache.get(key)
        if hit is None:
            cap = hip.mos_idw_sweep_max_configs()
            hit = cache[key] = [
                (torch.tensor([c[0] for c in key[i:i + cap]], dtype=torch.float64).to(self.device),
                 torch.tensor([c[1] for c in key[i:i + cap]], dtype=torch.float64).to(self.device))
                for i in range(0, len(key), cap)]
        return hit

    def sweep(self, pred: torch.Tensor, tfeat: torch.Tensor, truth_t2m: torch.Tensor, configs, acc: torch.Tensor,
              h: int = 0, fields_out: Optional[torch.Tensor] = None, n_out: Optional[torch.Tensor] = None):
        """The squared t2m error of every IDW setting of `configs` ((power, radius_km[, label]) tuples, e.g.
        `IDW_SWEEP_CONFIGS`) in one pass (scripts/mos_idw_sweep.py:260-272): `acc[p, h + s] += sum over b, g of
        (y_p - truth_t2m)^2`, where y_p is the t2m `LearnedMOS(..., True, power_p, radius_p).apply(pred, tfeat)` would
        give, with the difference and the square in the forecast's dtype and the sums in float64.  The station forest
        runs once (the biases do not depend on the setting), then one kernel serves all settings; the instance's own
        `power` / `radius` are not used, its station set decides whether IDW applies at all (fewer than two distinct
        points: every setting is the station-only correction).

        pred [G, steps, C] / [B, G, steps, C]; truth_t2m [G, steps] / [B, G, steps] in pred's dtype (any strides); acc
        float64 [len(configs), H] on the device.  fields_out ([P, B, G, steps], pred's dtype) receives every y_p and
        n_out (int32 [P, B]) the n_corrected of every setting; both optional.  No host sync; nothing is allocated
        after the first call per shape and config list.  Returns acc."""
        if not self.has_t2m:
            raise ValueError("LearnedMOS.sweep: var_order has no t2m")
        p4 = _as4(pred, "LearnedMOS.sweep")
        B, G, S, C = p4.shape
        if G != self.latitudes.shape[0] or C != len(self.var_order):
            raise ValueError(f"prediction [{G} rows, {C} channels] does not match the coordinates "
                             f"({self.latitudes.shape[0]}) / var_order ({len(self.var_order)})")
        if tfeat.shape != (B, len(self.ordered_stations), S, NUM_TIME_FEATURES) or tfeat.dtype != torch.float64 \
                or not tfeat.is_cuda or not tfeat.is_contiguous():
            raise ValueError(f"tfeat must be contiguous float64 [{B}, {len(self.ordered_stations)}, {S}, "
                             f"{NUM_TIME_FEATURES}] on the device (time_features), got {tuple(tfeat.shape)}")
        if not isinstance(truth_t2m, torch.Tensor) or not truth_t2m.is_cuda:
            raise RuntimeError("LearnedMOS.sweep needs GPU tensors (there is no CPU fallback)")
        t3 = truth_t2m if truth_t2m.dim() == 3 else truth_t2m.unsqueeze(0)
        if t3.shape != (B, G, S) or t3.dtype != p4.dtype:
            raise ValueError(f"truth_t2m must be {p4.dtype} [{B}, {G}, {S}], got {truth_t2m.dtype} "
                             f"{tuple(truth_t2m.shape)}")
        chunks = self._sweep_configs(configs)
        P = sum(c[0].numel() for c in chunks)
        if not acc.is_cuda or acc.dtype != torch.float64 or acc.dim() != 2 or acc.shape[0] != P \
                or not acc.is_contiguous() or not 0 <= h <= acc.shape[1] - S:
            raise ValueError(f"acc must be contiguous float64 [{P}, H >= {h + S}] on the device, got "
                             f"{acc.dtype} {tuple(acc.shape)}")
        if fields_out is not None and (fields_out.shape != (P, B, G, S) or fields_out.dtype != p4.dtype
                                       or not fields_out.is_cuda or not fields_out.is_contiguous()):
            raise ValueError(f"fields_out must be contiguous {p4.dtype} [{P}, {B}, {G}, {S}] on the device")
        if n_out is not None and (n_out.shape != (P, B) or n_out.dtype != torch.int32 or not n_out.is_cuda
                                  or not n_out.is_contiguous()):
            raise ValueError(f"n_out must be contiguous int32 [{P}, {B}] on the device")
        bufs = self._buffers(B, S, p4.dtype, p4.shape, False)[0]
        cap = chunks[0][0].numel()
        ws = bufs.get(("sweep_ws", cap))
        if ws is None:
            need = int(hip.lib().gcl_mos_idw_sweep_ws_bytes(G, cap, S, B))
            ws = bufs[("sweep_ws", cap)] = torch.empty(need, dtype=torch.uint8, device=self.device)
        f64 = int(p4.dtype == torch.float64)
        bias = bufs["bias"]
        hip._check(hip.lib().gcl_mos_forest_predict(
            self._nodes.data_ptr(), self._roots.data_ptr(), self.forest.num_trees, self.forest.baseline,
            p4.data_ptr(), f64, p4.stride(0), p4.stride(1), p4.stride(2), S, *self.chans, self._gidx.data_ptr(),
            self._gstart.data_ptr(), self.num_points, len(self.ordered_stations), tfeat.data_ptr(), bias.data_ptr(),
            None, None, B, hip._stream()))
        if n_out is not None:
            hip.zero_(n_out)
        p0 = 0
        for power, radius in chunks:
            n = power.numel()
            hip.mos_idw_sweep(p4, t3, self.chans[0], self._lat, self._lon, self._gidx, bias, self.idw, power, radius,
                              acc[p0:p0 + n], h, fields_out[p0:p0 + n] if fields_out is not None else None,
                              n_out[p0:p0 + n] if n_out is not None else None, ws)
            p0 += n
        return acc

    @property
    def station_bias(self) -> torch.Tensor:
        """The last call's per-point biases, float64 [B, points, steps] (of the most recently used shape)."""
        return next(reversed(self._bufs.values()))["bias"]


class CapturedLearnedMOS(LearnedMOS, Captured):
    """`LearnedMOS.apply` replayed from a hipGraph (capture.Captured): the forecast and the time features are the
    graph's arguments, so a new forecast or new valid times replay the same graph.  Returns the graph's output buffers
    (overwritten by the next call)."""

    def __init__(self, *args, use_graph: bool = True, **kw):
        LearnedMOS.__init__(self, *args, **kw)
        Captured.__init__(self, use_graph=use_graph, recapture=True)

    def _work(self, pred, tfeat):
        return LearnedMOS.apply(self, pred, tfeat)

    def __call__(self, pred: torch.Tensor, tfeat: torch.Tensor):
        if not self.has_t2m:
            return pred, None
        return self._run(pred, tfeat)


def apply_learned_mos_t2m(prediction_phys: torch.Tensor, var_order: list, model_bundle, latitudes, longitudes,
                          forecast_valid_times, station_lat: float = 56.173, station_lon: float = 92.493,
                          station_elev: float = 287.0, stations: Optional[list] = None, spatial_idw: bool = False,
                          idw_power: float = 2.0, idw_max_radius_km: float = 300.0):
    """The reference's `apply_learned_mos_t2m` on the device: `(corrected, n_corrected)` when t2m is present (a list
    of ints for a batched prediction), the input itself otherwise.  Synchronises once, for the count."""
    if "t2m" not in var_order:
        return prediction_phys
    if stations is None:
        stations = [{"lat": station_lat, "lon": station_lon, "elev": station_elev, "name": "default"}]
    p = prediction_phys
    dev = p.device if isinstance(p, torch.Tensor) and p.is_cuda else None
    if dev is None:
        raise RuntimeError("apply_learned_mos_t2m needs a GPU tensor (there is no CPU fallback)")
    mos = LearnedMOS(model_bundle, var_order, latitudes, longitudes, stations, spatial_idw, idw_power,
                     idw_max_radius_km, device=dev)
    B = p.shape[0] if p.dim() == 4 else 1
    steps = p.shape[-2]
    times = _times_2d(forecast_valid_times, B)
    if any(len(t) != steps for t in times):
        raise ValueError(f"{len(times[0])} valid times for {steps} forecast steps")
    tfeat = mos.time_features(times if p.dim() == 4 else times[0])
    if tfeat.shape[0] != B:
        tfeat = tfeat.expand(B, -1, -1, -1).contiguous()
    out = torch.empty_like(p, memory_format=torch.contiguous_format)
    corrected, n = mos.apply(p, tfeat, out=out)
    counts = n.cpu().tolist()
    return corrected, (counts if p.dim() == 4 else counts[0])


# ======================================================================================================================
# Fitting the learned MOS (scripts/build_learned_mos.py)
# ======================================================================================================================
# The model's input columns in order (build_learned_mos.py:245-266); the "feature_columns" of a saved bundle.
FEATURE_COLUMNS = (
    "era5_temperature_2m", "era5_dewpoint_2m", "era5_windspeed_10m", "wind_dir_sin", "wind_dir_cos",
    "era5_surface_pressure", "era5_cloudcover", "era5_shortwave_radiation", "era5_precipitation", "hour_sin",
    "hour_cos", "doy_sin", "doy_cos", "solar_elevation", "dewpoint_depression", "era5_t2m_lag6h", "delta_t2m_6h",
    "station_lat", "station_lon", "station_elev")
_ERA5_COLUMNS = ("era5_temperature_2m", "era5_dewpoint_2m", "era5_windspeed_10m", "era5_winddirection_10m",
                 "era5_surface_pressure", "era5_cloudcover", "era5_shortwave_radiation", "era5_precipitation")
SEASONS = {"DJF": (12, 1, 2), "MAM": (3, 4, 5), "JJA": (6, 7, 8), "SON": (9, 10, 11)}
_BIN_SUBSAMPLE = 200000  # sklearn's _BinMapper(subsample=...)


def training_table(times, era5: dict, station_t2m_C, station: dict):
    """One station's fitting table (build_learned_mos.py:313-315, build_features :203-242, :332).

    times: n datetimes in time order; era5: {column: float array [n]} with the eight hourly columns
    era5_temperature_2m, era5_dewpoint_2m, era5_windspeed_10m, era5_winddirection_10m (degrees), era5_surface_pressure,
    era5_cloudcover, era5_shortwave_radiation, era5_precipitation; station_t2m_C [n] the observation (NaN where
    missing); station {"lat", "lon", "elev"}.  Rows without t2m or observation and rows with |bias| >= 20 go first, the
    6-hour lag is then the sixth row before (as the reference's `shift(6)`), and rows with a NaN feature or bias go last.
    Returns (X float64 [m, 20] in FEATURE_COLUMNS order, bias float64 [m], the m kept times).  Tables of several
    stations are concatenated and sorted by time by the caller (:330-331)."""
    times = list(times)
    cols = {k: np.asarray(era5[k], dtype=np.float64) for k in _ERA5_COLUMNS}
    obs = np.asarray(station_t2m_C, dtype=np.float64)
    n = len(times)
    if obs.shape != (n,) or any(v.shape != (n,) for v in cols.values()):
        raise ValueError(f"training_table: every column must have one entry per time ({n})")
    t2m = cols["era5_temperature_2m"]
    with np.errstate(invalid="ignore"):
        bias = obs - t2m
        keep = ~np.isnan(t2m) & ~np.isnan(obs) & (np.abs(bias) < 20.0)
    idx = np.nonzero(keep)[0]
    times = [times[i] for i in idx]
    cols = {k: v[idx] for k, v in cols.items()}
    bias, t2m = bias[idx], t2m[idx]
    hour = np.array([t.hour for t in times], dtype=np.int64)
    doy = np.array([t.timetuple().tm_yday for t in times], dtype=np.int64)
    lag = np.full(t2m.shape, np.nan)
    lag[6:] = t2m[:-6]
    wd = np.deg2rad(cols["era5_winddirection_10m"])
    lat, lon, elev = station["lat"], station["lon"], station["elev"]
    feats = {
        "wind_dir_sin": np.sin(wd), "wind_dir_cos": np.cos(wd),
        "hour_sin": np.sin(2 * np.pi * hour / 24), "hour_cos": np.cos(2 * np.pi * hour / 24),
        "doy_sin": np.sin(2 * np.pi * doy / 365.25), "doy_cos": np.cos(2 * np.pi * doy / 365.25),
        "solar_elevation": np.array([solar_elevation(lat, lon, t) for t in times], dtype=np.float64),
        "dewpoint_depression": t2m - cols["era5_dewpoint_2m"], "era5_t2m_lag6h": lag, "delta_t2m_6h": t2m - lag,
        "station_lat": np.full(t2m.shape, lat, dtype=np.float64),
        "station_lon": np.full(t2m.shape, lon, dtype=np.float64),
        "station_elev": np.full(t2m.shape, elev, dtype=np.float64)}
    X = np.column_stack([feats[c] if c in feats else cols[c] for c in FEATURE_COLUMNS]).reshape(len(times), 20)
    ok = ~(np.isnan(X).any(axis=1) | np.isnan(bias))
    return np.ascontiguousarray(X[ok]), bias[ok], [t for t, k in zip(times, ok) if k]


def fit_mos_table(times, bias) -> dict:
    """The static baseline of build_learned_mos.py:381-385: the mean bias per (month, hour), in the
    `{"bias_table": {str(month): {str(hour): float}}}` form of `load_mos_table` / `get_t2m_bias` / `apply_mos_t2m`."""
    bias = np.asarray(bias, dtype=np.float64)
    groups = {}
    for i, t in enumerate(times):
        groups.setdefault((t.month, t.hour), []).append(i)
    table = {}
    for (m, h) in sorted(groups):
        table.setdefault(str(m), {})[str(h)] = float(np.mean(bias[groups[(m, h)]]))
    return {"bias_table": table}


def bin_thresholds(X: np.ndarray, max_bins: int = 255, seed=None) -> list:
    """sklearn's `_BinMapper.fit` for rows without NaN: per feature the float64 thresholds between bins.  With at most
    `max_bins` distinct values they are the midpoints of consecutive distinct values ((a + b) * 0.5), else the
    `max_bins - 1` inner percentiles of the sorted column (method "midpoint"); a one-valued feature has none.  Above
    200 000 rows they come from the rows `RandomState(seed).choice(n, 200000, replace=False)`."""
    X = np.asarray(X, dtype=np.float64)
    if X.shape[0] > _BIN_SUBSAMPLE:
        X = X.take(np.random.RandomState(seed).choice(X.shape[0], _BIN_SUBSAMPLE, replace=False), axis=0)
    out = []
    for f in range(X.shape[1]):
        col = np.sort(X[:, f])
        distinct = np.unique(col)
        if len(distinct) <= max_bins:
            mid = distinct[:-1] + distinct[1:]
            mid *= 0.5
        else:
            mid = np.percentile(col, np.linspace(0, 100, num=max_bins + 1)[1:-1], method="midpoint").astype(np.float64)
        np.clip(mid, None, 1e300, out=mid)  # sklearn's ALMOST_INF
        out.append(mid)
    return out


def early_stopping_split(n: int, validation_fraction: float = 0.1, random_state=42):
    """(seed, train_rows, val_rows) as sklearn's fit draws them: seed = RandomState(random_state).randint(2^32 - 1),
    perm = RandomState(seed).permutation(n), validation = the first ceil(fraction n) of perm, training = the next
    floor((1 - fraction) n)."""
    seed = int(np.random.RandomState(random_state).randint(np.iinfo(np.uint32).max, dtype="u8"))
    perm = np.random.RandomState(seed).permutation(n)
    n_val = int(math.ceil(validation_fraction * n))
    n_train = int(math.floor((1.0 - validation_fraction) * n))
    return seed, perm[n_val:n_val + n_train], perm[:n_val]


def should_stop(scores, n_iter_no_change: int = 15, tol: float = 1e-7) -> bool:
    """sklearn's `_should_stop`: with p = n_iter_no_change + 1, True once there are p scores and none of the last p - 1
    exceeds scores[-p] + tol."""
    p = n_iter_no_change + 1
    if len(scores) < p:
        return False
    ref = scores[-p] + (0.0 if tol is None else tol)
    return not any(s > ref for s in scores[-p + 1:])


class MOSFit(NamedTuple):
    """What `MOSFitter.fit` returns: the forest, sklearn's `n_iter_` and `validation_score_` (index 0: the baseline;
    empty without early stopping), the bin thresholds per feature and the rows of X used for training / validation."""
    forest: MOSForest
    n_iter_: int
    validation_score_: np.ndarray
    bin_thresholds: list
    train_rows: np.ndarray
    val_rows: np.ndarray

    def bundle(self, **metadata) -> dict:
        """The reference's bundle dict (build_learned_mos.py:453-464) with the forest as "model"."""
        return {"model": self.forest, "feature_columns": list(FEATURE_COLUMNS), **metadata}


class _TreeStep(Captured):
    """One boosting iteration (gcl_mos_fit_tree): the same launch sequence every time, replayed from a hipGraph."""

    def __init__(self, call, use_graph):
        super().__init__(graph_enabled(use_graph), required=use_graph is True)
        self._call = call

    def _work(self):
        hip._check(self._call(hip._stream()))

    def __call__(self):
        return self._run()


class MOSFitter:
    """`HistGradientBoostingRegressor(loss="squared_error").fit` on the device (build_learned_mos.py:357-369), for rows
    without missing values.  Hyper-parameters carry sklearn's names; the defaults are the reference's.  The fit
    reproduces sklearn's trees (features, thresholds, structure) wherever float64 sums decide a split unambiguously,
    and repeats its own bytes from run to run."""

    def __init__(self, max_iter: int = 500, max_depth: int = 8, learning_rate: float = 0.05, min_samples_leaf: int = 20,
                 l2_regularization: float = 0.1, max_leaf_nodes: int = 31, max_bins: int = 255,
                 early_stopping: bool = True, validation_fraction: float = 0.1, n_iter_no_change: int = 15,
                 tol: float = 1e-7, random_state=42):
        if not 2 <= max_bins <= 255:
            raise ValueError(f"max_bins={max_bins} (2 .. 255)")
        if not 2 <= max_leaf_nodes <= 256:
            raise ValueError(f"max_leaf_nodes={max_leaf_nodes} (2 .. 256)")
        if max_iter < 1 or max_depth is None or max_depth < 1 or min_samples_leaf < 1:
            raise ValueError("max_iter, max_depth and min_samples_leaf must be at least 1")
        self.max_iter, self.max_depth, self.learning_rate = int(max_iter), int(max_depth), float(learning_rate)
        self.min_samples_leaf, self.l2_regularization = int(min_samples_leaf), float(l2_regularization)
        self.max_leaf_nodes, self.max_bins, self.early_stopping = int(max_leaf_nodes), int(max_bins), bool(early_stopping)
        self.validation_fraction, self.n_iter_no_change, self.tol = validation_fraction, int(n_iter_no_change), tol
        self.random_state = random_state

    @staticmethod
    def _host(a, what, ndim):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != ndim:
            raise ValueError(f"MOSFitter.fit: {what} must have {ndim} dimension(s), got shape {a.shape}")
        if not np.isfinite(a).all():
            raise ValueError(f"MOSFitter.fit: NaN or inf in {what} (the reference drops such rows before fitting)")
        return a

    def fit(self, X, y, validation=None, check_every: int = 16, use_graph=None, device=None) -> MOSFit:
        """Fit on X float64 [n, F <= 32] (host array or device tensor) and y [n].  `validation=(X_val, y_val)` replaces
        the random split of early stopping.  The device runs whole iterations without the host; every `check_every`
        iterations the host reads the scores, applies sklearn's stopping rule to each prefix and, when it fires, drops
        the trees grown past that iteration.  `use_graph`: replay an iteration from a hipGraph (None: unless
        GCL_NO_GRAPH is set)."""
        X, y = self._host(X, "X", 2), self._host(y, "y", 1)
        n_all, F = X.shape
        if F < 1 or F > 32:
            raise ValueError(f"MOSFitter.fit: {F} features (1 .. 32, MOSForest's limit)")
        if y.shape[0] != n_all:
            raise ValueError(f"MOSFitter.fit: {n_all} rows of X, {y.shape[0]} of y")
        if check_every < 1:
            raise ValueError("MOSFitter.fit: check_every must be at least 1")
        seed = int(np.random.RandomState(self.random_state).randint(np.iinfo(np.uint32).max, dtype="u8"))
        train_rows, val_rows = np.arange(n_all), np.arange(0)
        Xv = yv = None
        if validation is not None:
            Xv, yv = self._host(validation[0], "X_val", 2), self._host(validation[1], "y_val", 1)
            if Xv.shape[1] != F or Xv.shape[0] != yv.shape[0]:
                raise ValueError("MOSFitter.fit: validation rows do not match X / y_val")
        elif self.early_stopping:
            _, train_rows, val_rows = early_stopping_split(n_all, self.validation_fraction, self.random_state)
            Xv, yv = X[val_rows], y[val_rows]
        if not self.early_stopping:
            Xv = yv = None
        n_val = 0 if Xv is None else Xv.shape[0]
        if self.early_stopping and n_val == 0:
            raise ValueError("MOSFitter.fit: early stopping needs at least one validation row")
        Xt, yt = (X, y) if train_rows.size == n_all else (X[train_rows], y[train_rows])
        n = Xt.shape[0]
        if n < 1:
            raise ValueError("MOSFitter.fit: no training rows")
        if not torch.cuda.is_available():
            raise RuntimeError("MOSFitter.fit needs a GPU (there is no CPU fallback)")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = hip.lib()
        thresholds = bin_thresholds(Xt, self.max_bins, seed)
        baseline = float(np.mean(yt))
        with torch.cuda.device(dev):
            thr = np.zeros((F, 256), dtype=np.float64)
            for f, t in enumerate(thresholds):
                thr[f, :len(t)] = t
            d_thr = torch.from_numpy(thr).to(dev)
            d_nthr = torch.tensor([len(t) for t in thresholds], dtype=torch.int32).to(dev)

            def binned(A):
                ld = (A.shape[0] + 255) // 256 * 256
                b = torch.zeros(F, ld, dtype=torch.uint8, device=dev)
                dA = torch.from_numpy(A).to(dev)
                hip._check(L.gcl_mos_fit_bin(dA.data_ptr(), A.shape[0], F, d_thr.data_ptr(), d_nthr.data_ptr(),
                                             b.data_ptr(), ld, hip._stream()))
                return b, ld

            bins, ld = binned(np.ascontiguousarray(Xt))
            d_y = torch.from_numpy(np.ascontiguousarray(yt)).to(dev)
            raw = torch.full((n,), baseline, dtype=torch.float64, device=dev)
            need = int(L.gcl_mos_fit_ws_bytes(n, n_val, F, self.max_leaf_nodes, self.max_iter))
            if need == 0:
                raise ValueError("MOSFitter.fit: the table is outside what gcl_mos_fit_tree takes")
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            nodes = torch.zeros(self.max_iter * (2 * self.max_leaf_nodes - 1) * 16, dtype=torch.uint8, device=dev)
            roots = torch.zeros(self.max_iter + 1, dtype=torch.int32, device=dev)
            scores = torch.zeros(self.max_iter + 1, dtype=torch.float64, device=dev)
            state = torch.zeros(2, dtype=torch.int32, device=dev)
            if n_val:
                bins_v, ld_v = binned(np.ascontiguousarray(Xv))
                d_yv = torch.from_numpy(np.ascontiguousarray(yv)).to(dev)
                raw_v = torch.full((n_val,), baseline, dtype=torch.float64, device=dev)
                hip._check(L.gcl_mos_fit_score(raw_v.data_ptr(), d_yv.data_ptr(), n_val, scores.data_ptr(),
                                               ws.data_ptr(), need, hip._stream()))
                val_args = (bins_v.data_ptr(), ld_v, n_val, d_yv.data_ptr(), raw_v.data_ptr())
            else:
                val_args = (None, 0, 0, None, None)

            def call(stream):
                return L.gcl_mos_fit_tree(
                    bins.data_ptr(), ld, n, F, d_nthr.data_ptr(), d_thr.data_ptr(), d_y.data_ptr(), raw.data_ptr(),
                    *val_args, self.max_leaf_nodes, self.max_depth, self.min_samples_leaf, self.l2_regularization,
                    self.learning_rate, self.max_iter, nodes.data_ptr(), roots.data_ptr(), scores.data_ptr(),
                    state.data_ptr(), ws.data_ptr(), need, stream)

            step = _TreeStep(call, use_graph)
            n_iter, checked = self.max_iter, 0  # scores[:checked + 1] have been through the stopping rule
            for it in range(1, self.max_iter + 1):
                step()
                if self.early_stopping and (it % check_every == 0 or it == self.max_iter):
                    sc = scores[:it + 1].cpu().numpy()
                    stop = next((k for k in range(checked + 1, it + 1)
                                 if should_stop(sc[:k + 1], self.n_iter_no_change, self.tol)), None)
                    checked = it
                    if stop is not None:
                        n_iter = stop
                        break
            torch.cuda.synchronize(dev)
            self.launch_mode = step.launch_mode
            grown, n_nodes = (int(v) for v in state.cpu().tolist())
            h_roots = roots.cpu().numpy()
            if grown < n_iter:
                raise RuntimeError(f"MOSFitter.fit: {grown} trees on the device, {n_iter} expected")
            total = n_nodes if n_iter == grown else int(h_roots[n_iter])
            packed = nodes[:total * 16].cpu().numpy().view([("v", "<f8"), ("a", "<u4"), ("b", "<u4")])
            val_scores = scores[:n_iter + 1].cpu().numpy() if self.early_stopping else np.zeros(0)
        b = packed["b"]
        forest = MOSForest((b >> 24) & 31, packed["v"], packed["a"], b & 0xFFFFFF, (b >> 29) & 1, (b >> 30) & 1,
                           h_roots[:n_iter], baseline, n_features=F)
        return MOSFit(forest, n_iter, val_scores, thresholds, train_rows, val_rows)


def fit_learned_mos(X, y, validation=None, check_every: int = 16, use_graph=None, device=None, **kw) -> MOSFit:
    """`MOSFitter(**kw).fit(X, y, ...)`: the reference's model fit (build_learned_mos.py:357-369) on the device."""
    return MOSFitter(**kw).fit(X, y, validation=validation, check_every=check_every, use_graph=use_graph, device=device)


def evaluate_learned_mos(forest, X, y, times, table: Optional[dict] = None) -> dict:
    """(`forest`: a `MOSFit`, a `MOSForest` or a bundle.)  Step 4 of build_learned_mos.py (:374-433) on a test table: MAE / RMSE of the raw forecast (zero correction), the
    static (month, hour) table (`fit_mos_table`; None: left out) and the learned forest, overall, per season and per
    hour (every third, as the reference prints them).  The forest runs on the device (`MOSForest.predict`); the
    reductions are float64 on the host."""
    forest = forest.forest if isinstance(forest, MOSFit) else _forest_of(forest)
    y = np.asarray(y, dtype=np.float64)
    times = list(times)
    Xd = X if isinstance(X, torch.Tensor) and X.is_cuda else torch.from_numpy(
        np.ascontiguousarray(X, dtype=np.float64)).to(torch.device("cuda", torch.cuda.current_device()))
    pred = forest.predict(Xd).cpu().numpy()
    month = np.array([t.month for t in times])
    hour = np.array([t.hour for t in times])
    methods = {"raw": np.zeros_like(y), "learned": pred}
    if table is not None:
        methods["static"] = np.array([get_t2m_bias(table, t) for t in times], dtype=np.float64)

    def mae(mask, p):
        return float(np.mean(np.abs(y[mask] - p[mask])))

    every = np.ones(y.shape, dtype=bool)
    out = {"n": int(y.size), "per_season": {}, "per_hour": {}}
    for name, p in methods.items():
        out[name] = {"mae": mae(every, p), "rmse": float(np.sqrt(np.mean((y - p) ** 2)))}
    for name, months in SEASONS.items():
        mask = np.isin(month, months)
        if mask.any():
            out["per_season"][name] = {"n": int(mask.sum()), **{k: mae(mask, p) for k, p in methods.items()}}
    for h in range(0, 24, 3):
        mask = hour == h
        if mask.any():
            out["per_hour"][h] = {"n": int(mask.sum()), **{k: mae(mask, p) for k, p in methods.items()}}
    return out


def save_learned_mos(path, fit, **metadata) -> None:
    """Store a fitted forest (a `MOSFit` or `MOSForest`) with the bundle's metadata keys (build_learned_mos.py:453-464:
    stations_trained, period, split, test_mae, ...; "feature_columns" is added) as an `.npz` that `load_learned_mos`
    reads back without sklearn."""
    forest = fit.forest if isinstance(fit, MOSFit) else _forest_of(fit)
    if not str(path).endswith(".npz"):
        raise ValueError("save_learned_mos writes an .npz (a .joblib bundle is the reference's, written by joblib)")
    meta = {"feature_columns": list(FEATURE_COLUMNS), **metadata}
    np.savez_compressed(path, baseline=np.float64(forest.baseline), n_features=np.int32(forest.n_features),
                        bundle_json=np.array(json.dumps(meta)), **{k: getattr(forest, k) for k in forest._FIELDS})
