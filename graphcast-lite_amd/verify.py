"""Forecast scoring and global -> regional blending on the HIP path: drop-in for the metric and pipeline helpers of the
reference's inference scripts.

* `linspace_lats_lons`, `region_node_indices` (`scripts/predict.py:28-43`): host helpers, unchanged.
* `StreamingMetrics` (`scripts/predict.py:53-122`; with the default arguments also the variant of
  `scripts/predict_pipeline.py:156-191`): same attributes and properties, but the sums live on the GPU in float64.
  `update` takes device tensors and does not synchronise; reading a property costs one copy to the host.
* `ForecastVerifier`: the update block of `scripts/predict.py:574-600` (per method: overall, per horizon, and the same
  for a region's rows) in one statistics call per row set plus one accumulate launch; persistence is read straight
  from the input window through a column map (`Persistence`), never materialised.
* `interpolate_global_to_region` (`scripts/predict_pipeline.py:95-132`) and `interpolate_field_2d`
  (`scripts/interpolate_to_region.py:64-73`): scipy's `RegularGridInterpolator(method="linear", bounds_error=False,
  fill_value=None)` reproduced bit for bit, from tables built once per axes pair with numpy.  Not periodic in
  longitude: targets outside the source axes are extrapolated from the edge cell, as scipy does.
* `build_taper_mask_2d` (`scripts/predict_pipeline.py:135-149`), `taper_blend` (`:326`).
* `GlobalRegionalForecast` (`scripts/predict_pipeline.py:300-329`) and its hipGraph-captured form
  `CapturedGlobalRegionalForecast`.
* `load_scaler_stats`, `inverse_standardize`, `unit_label`, `apply_units`, `compute_stat`
  (`scripts/metrics_maps.py:29-90`): same names and signatures, device tensors; the unit conversion is bit-equal to
  the reference's CPU arithmetic.
* `MetricMaps`, `CapturedMetricMaps`, `metric_maps`: the per-grid-point RMSE / MAE / bias / ACC maps of that script
  (`:143-176`), accumulated batch by batch in a float64 device state, per lead time, optionally on a row subset and
  against persistence.

Kernels: csrc/verify.hip, csrc/maps.hip.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured
from .interp_tables import TableCache, bilinear_corners, device_tables, find_cells  # noqa: F401

_STATE_FIXED = 4  # [sum_se, sum_ae, n, total_elem] ahead of the four per-channel vectors


# ======================================================================================================================
# Host helpers (scripts/predict.py:28-43)
# ======================================================================================================================
def linspace_lats_lons(num_lat: int, num_lon: int):
    """The regular global axes: latitudes -90..90 inclusive, longitudes [0, 360)."""
    return (np.linspace(-90, 90, num_lat, endpoint=True), np.linspace(0, 360, num_lon, endpoint=False))


def region_node_indices(lat_min, lat_max, lon_min, lon_max, lats, lons) -> np.ndarray:
    """int64 grid indices of the nodes inside a lat / lon box (bounds inclusive), longitude-major: for every longitude
    index j in the box, the latitude indices i in the box, as j * len(lats) + i."""
    li = np.nonzero((lats >= lat_min) & (lats <= lat_max))[0]
    lj = np.nonzero((lons >= lon_min) & (lons <= lon_max))[0]
    return (lj[:, None].astype(np.int64) * len(lats) + li[None, :]).reshape(-1)


# ======================================================================================================================
# Streaming metrics
# ======================================================================================================================
class Persistence:
    """The persistence forecast `X[:, -C:].repeat(1, P)` (`scripts/predict.py:469`) as a column map into the input
    window X [G, obs*C] (or [B, G, obs*C]): column c reads X[:, F - C + c % C], nothing is materialised."""

    def __init__(self, X: torch.Tensor, num_channels: int):
        self.X, self.C = X, int(num_channels)
        self._maps = {}

    @property
    def shape(self):
        return self.X.shape

    def column_map(self, K: int) -> torch.Tensor:
        key = (K, self.X.device)
        m = self._maps.get(key)
        if m is None:
            F = self.X.shape[-1]
            m = torch.from_numpy((F - self.C + np.arange(K) % self.C).astype(np.int32)).to(self.X.device)
            self._maps[key] = m
        return m


_JOB_CACHE = {}


def _upload_i64(rows, device) -> torch.Tensor:
    """A small int64 table on the device, uploaded once per distinct content (captured launches keep pointing at it)."""
    arr = np.ascontiguousarray(np.asarray(rows, dtype=np.int64))
    key = (arr.tobytes(), arr.shape, str(device))
    t = _JOB_CACHE.get(key)
    if t is None:
        t = torch.from_numpy(arr).to(device)
        _JOB_CACHE[key] = t
    return t


def _as3(t):
    if isinstance(t, Persistence):
        return t, (t.X if t.X.dim() == 3 else t.X.unsqueeze(0))
    return t, (t if t.dim() == 3 else t.unsqueeze(0))


def _pred_arg(p, K: int, B: int, G: int):
    """(tensor [B, G, W] with unit column stride, int32 column map or None) for a prediction or a Persistence view."""
    if isinstance(p, Persistence):
        X3 = p.X if p.X.dim() == 3 else p.X.unsqueeze(0)
        X3 = hip._rows_view(X3)
        assert X3.shape[0] == B and X3.shape[1] == G, f"persistence window {tuple(X3.shape)} vs truth rows {G}"
        return X3, p.column_map(K)
    P3 = hip._rows_view(p if p.dim() == 3 else p.unsqueeze(0))
    if P3.shape[0] != B or P3.shape[1] != G or P3.shape[2] < K:
        raise ValueError(f"prediction of shape {tuple(p.shape)} does not cover the truth's {B} x {G} x {K}")
    return P3, None


def _cached_stats(B, npred, K, device, owner, key):
    buf = owner.get(key)
    if buf is None:
        buf = torch.empty(B, npred, K, 3, dtype=torch.float64, device=device)
        owner[key] = buf
    return buf


class StreamingMetrics:
    """MSE / MAE / spatial ACC accumulated sample by sample (`scripts/predict.py:53-122`).

    The sums are a float64 device state updated by `gcl_verify_colstats` + `gcl_verify_accumulate` in the reference's
    order; `update` never synchronises (so it can be captured in a hipGraph once the object has been updated eagerly
    with the same shapes).  Properties copy the state to the host once per read and return Python floats and float64 /
    int64 numpy arrays as the reference does.  `device` allocates the state up front (otherwise: on the first update).
    """

    def __init__(self, num_channels: int, exclude_channels: list = None, device=None):
        self.C = int(num_channels)
        self.exclude_channels = set(exclude_channels or [])
        self._state = None
        self._state_base, self._state_off = None, 0
        self._mask = None
        self._scratch = {}
        if device is not None:
            self._ensure(torch.device(device))

    # -- device state --------------------------------------------------------------------------------------------------
    def _mask_host(self) -> np.ndarray:
        m = np.zeros(self.C, dtype=np.uint8)
        for ch in self.exclude_channels:
            if 0 <= ch < self.C:
                m[ch] = 1
        return m

    def _ensure(self, device):
        if self._state is None:
            self._state = torch.zeros(_STATE_FIXED + 4 * self.C, dtype=torch.float64, device=device)
            self._state_base, self._state_off = self._state, 0
            if self.exclude_channels:
                self._mask = torch.from_numpy(self._mask_host()).to(device)
        return self._state

    def _bind(self, base: torch.Tensor, index: int, mask: Optional[torch.Tensor]):
        """Use row `index` of a [n_objects, 4 + 4C] float64 buffer as the state (ForecastVerifier)."""
        self._state = base[index]
        self._state_base, self._state_off, self._mask = base, index * base.shape[1], mask

    def reset(self):
        """Zero every sum and count (not in the reference; lets a captured update start again)."""
        if self._state is not None:
            self._state.zero_()

    def update(self, y_true: torch.Tensor, y_pred):
        """y_true, y_pred: device tensors [G, C*P] or [G, C] (or [B, G, ...]: B updates in order).  y_pred may be a
        `Persistence` view."""
        _, T3 = _as3(y_true)
        T3 = hip._rows_view(T3)
        B, G, K = T3.shape
        dev = T3.device
        self._ensure(dev)
        P3, cmap = _pred_arg(y_pred, K, B, G)
        stats = _cached_stats(B, 1, K, dev, self._scratch, ("stats", B, K, dev))
        hip.verify_colstats(T3, [(P3, cmap)], None, stats)
        jobs = _upload_i64([[0, 3 * K, K, self.C, self._state_off, 0 if self._mask is not None else -1, G, B]], dev)
        hip.verify_accumulate(stats, jobs, self._state_base, self._mask)

    # -- host view -----------------------------------------------------------------------------------------------------
    def _host(self) -> np.ndarray:
        if self._state is None:
            return np.zeros(_STATE_FIXED + 4 * self.C, dtype=np.float64)
        return self._state.detach().cpu().numpy()

    def _split(self):
        h, C = self._host(), self.C
        o = _STATE_FIXED
        return dict(sum_se=float(h[0]), sum_ae=float(h[1]), n=int(h[2]), total_elem=int(h[3]),
                    sum_se_per_ch=h[o:o + C].copy(), sum_acc=h[o + C:o + 2 * C].copy(),
                    elem_per_ch=h[o + 2 * C:o + 3 * C].astype(np.int64), acc_count=h[o + 3 * C:o + 4 * C].astype(np.int64))

    n = property(lambda self: self._split()["n"])
    total_elem = property(lambda self: self._split()["total_elem"])
    sum_se = property(lambda self: self._split()["sum_se"])
    sum_ae = property(lambda self: self._split()["sum_ae"])
    sum_se_per_ch = property(lambda self: self._split()["sum_se_per_ch"])
    elem_per_ch = property(lambda self: self._split()["elem_per_ch"])
    sum_acc = property(lambda self: self._split()["sum_acc"])
    acc_count = property(lambda self: self._split()["acc_count"])

    @property
    def mse(self):
        s = self._split()
        return s["sum_se"] / max(s["total_elem"], 1)

    @property
    def rmse(self):
        return float(np.sqrt(self.mse))

    @property
    def mae(self):
        s = self._split()
        return s["sum_ae"] / max(s["total_elem"], 1)

    @property
    def acc_per_channel(self):
        s = self._split()
        return s["sum_acc"] / np.maximum(s["acc_count"], 1)

    @property
    def rmse_per_channel(self):
        """Normalized RMSE per channel."""
        s = self._split()
        return np.sqrt(s["sum_se_per_ch"] / np.maximum(s["elem_per_ch"], 1))

    @property
    def acc(self):
        apc = self.acc_per_channel
        dyn = [c for c in range(self.C) if c not in self.exclude_channels]
        return float(apc[dyn].mean()) if dyn else 0.0


class ForecastVerifier:
    """The metric set of `scripts/predict.py` (`:424-439` and the update block `:574-600`), filled from one truth and
    named predictions per sample.

    For every method name: `overall[m]` (sm_pred / sm_base), `horizon[m][p]` (sm_pred_h / sm_base_h, `ar_steps`
    objects when ar_steps > 1), and with `region_idxs`: `region[m]`, `region_horizon[m][p]`.  `update(y, pred=out,
    base=Persistence(X, C))`: predictions wider than the truth are trimmed to it (`:579-582`); the horizon objects of
    the first min(ar_steps, truth steps) horizons are updated when that is more than 1, as the reference does.  Costs
    one `gcl_verify_colstats` per row set (all methods and columns at once) and one `gcl_verify_accumulate`."""

    def __init__(self, num_channels: int, ar_steps: int, exclude_channels: list = None,
                 region_idxs: Optional[Sequence[int]] = None, methods: Sequence[str] = ("pred", "base"), device=None):
        if not 1 <= len(methods) <= 4:
            raise ValueError(f"1 to 4 methods per verifier, got {len(methods)}")
        self.C, self.ar_steps, self.methods = int(num_channels), int(ar_steps), tuple(methods)
        self.exclude_channels = sorted(set(exclude_channels or []))
        self.region_idxs = None if region_idxs is None else np.asarray(region_idxs, dtype=np.int64)
        mk = lambda: StreamingMetrics(self.C, exclude_channels=self.exclude_channels)  # noqa: E731
        nh = self.ar_steps if self.ar_steps > 1 else 0
        self.overall = {m: mk() for m in self.methods}
        self.horizon = {m: [mk() for _ in range(nh)] for m in self.methods}
        has_r = self.region_idxs is not None
        self.region = {m: (mk() if has_r else None) for m in self.methods}
        self.region_horizon = {m: ([mk() for _ in range(nh)] if has_r else []) for m in self.methods}
        self._objects = []  # (row set, method index, first column, object)
        for q, m in enumerate(self.methods):
            self._objects.append((0, q, None, self.overall[m]))
            self._objects += [(0, q, p, o) for p, o in enumerate(self.horizon[m])]
            if has_r:
                self._objects.append((1, q, None, self.region[m]))
                self._objects += [(1, q, p, o) for p, o in enumerate(self.region_horizon[m])]
        self._device, self._states, self._mask, self._rows = None, None, None, None
        self._scratch = {}
        if device is not None:
            self._ensure(torch.device(device))

    def _ensure(self, device):
        if self._device is None:
            self._device = device
            self._states = torch.zeros(len(self._objects), _STATE_FIXED + 4 * self.C, dtype=torch.float64,
                                       device=device)
            if self.exclude_channels:
                self._mask = torch.from_numpy(self._objects[0][3]._mask_host()).to(device)
            for i, (_, _, _, o) in enumerate(self._objects):
                o._bind(self._states, i, self._mask)
            if self.region_idxs is not None:
                self._rows = torch.from_numpy(self.region_idxs.astype(np.int32)).to(device)
        elif device != self._device:
            raise ValueError(f"ForecastVerifier lives on {self._device}, got tensors on {device}")

    def reset(self):
        if self._states is not None:
            self._states.zero_()

    def _jobs(self, B: int, K: int, G: int, n_region: int):
        nq = len(self.methods)
        P_eff = min(self.ar_steps, K // self.C)
        rs_stride = B * nq * K * 3
        rows = []
        for i, (rs, q, p, _) in enumerate(self._objects):
            if p is not None and not (P_eff > 1 and p < P_eff):
                continue
            k0, ncols = (0, K) if p is None else (p * self.C, self.C)
            rows.append([rs * rs_stride + (q * K + k0) * 3, nq * K * 3, ncols, self.C,
                         i * (_STATE_FIXED + 4 * self.C), 0 if self._mask is not None else -1,
                         G if rs == 0 else n_region, B])
        return _upload_i64(rows, self._device)

    def update(self, y: torch.Tensor, **preds):
        """y: truth [G, K] (or [B, G, K]) on the device; one keyword per method (tensor or `Persistence`)."""
        if set(preds) != set(self.methods):
            raise ValueError(f"expected predictions {self.methods}, got {tuple(preds)}")
        T3 = hip._rows_view(y if y.dim() == 3 else y.unsqueeze(0))
        B, G, K = T3.shape
        if self.region_idxs is not None and self.region_idxs.size and not (
                0 <= self.region_idxs.min() and self.region_idxs.max() < G):
            raise ValueError(f"region rows outside the truth's {G} rows")
        self._ensure(T3.device)
        args = [_pred_arg(preds[m], K, B, G) for m in self.methods]
        nq = len(self.methods)
        nrs = 2 if self._rows is not None else 1
        key = ("stats", B, K)
        stats = self._scratch.get(key)
        if stats is None:
            stats = torch.empty(nrs, B, nq, K, 3, dtype=torch.float64, device=T3.device)
            self._scratch[key] = stats
        hip.verify_colstats(T3, args, None, stats[0])
        if self._rows is not None:
            hip.verify_colstats(T3, args, self._rows, stats[1])
        n_region = self._rows.numel() if self._rows is not None else 0
        hip.verify_accumulate(stats, self._jobs(B, K, G, n_region), self._states, self._mask)


# ======================================================================================================================
# Regridding (scripts/predict_pipeline.py:95-132, scripts/interpolate_to_region.py:64-73)
# ======================================================================================================================
def regrid_tables(src_lats, src_lons, dst_lats, dst_lons):
    """Host tables of the bilinear regrid from the (src_lons, src_lats) grid onto the targets (dst_lons[j],
    dst_lats[i]), numbered longitude-major (j * len(dst_lats) + i): int32 [nt, 2] cells (lon, lat) and float64 [nt, 4]
    weights of the corners (lon, lat), (lon, lat+1), (lon+1, lat), (lon+1, lat+1), each formed as 1 * w_lon * w_lat."""
    q_lons, q_lats = np.asarray(dst_lons, dtype=np.float64), np.asarray(dst_lats, dtype=np.float64)
    ilon, ilat, w = bilinear_corners(src_lons, src_lats, q_lons[:, None], q_lats[None, :])
    return np.stack([ilon, ilat], axis=1).astype(np.int32), w


def regrid_tables_latlon(src_lats, src_lons, dst_lats, dst_lons):
    """`regrid_tables` for an interpolator whose axes are (lats, lons) (scripts/build_multires_dataset.py:220-224),
    targets (dst_lats[i], dst_lons[j]) numbered latitude-major (i * len(dst_lons) + j): int32 [nt, 2] cells (lat, lon)
    and float64 [nt, 4] weights of the corners (lat, lon), (lat, lon+1), (lat+1, lon), (lat+1, lon+1), each formed as
    (1 * w_lat) * w_lon.  The products equal those of `regrid_tables`; the ORDER of the corners is what differs, and
    with it the float64 sum."""
    q_lats, q_lons = np.asarray(dst_lats, dtype=np.float64), np.asarray(dst_lons, dtype=np.float64)
    ilat, ilon, w = bilinear_corners(src_lats, src_lons, q_lats[:, None], q_lons[None, :])
    return np.stack([ilat, ilon], axis=1).astype(np.int32), w


_TABLES = TableCache()


def _device_tables(src_lats, src_lons, dst_lats, dst_lons, device):
    """The `regrid_tables` of the axes on the device: built and uploaded once, then the same (shared) tensors."""
    axes = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (src_lats, src_lons, dst_lats, dst_lons)]
    key = tuple(TableCache.array_key(a) for a in axes)
    return device_tables(*_TABLES.get(key, lambda: regrid_tables(*axes)), device)


def interpolate_global_to_region(global_pred, global_lats, global_lons, region_lats, region_lons):
    """Bilinear interpolation of a global prediction (G_global, C*P) (or [B, G_global, C*P]) on the device onto the
    regional grid: (G_region, C*P) float32, bit-equal to the reference's scipy evaluation."""
    src3 = global_pred if global_pred.dim() == 3 else global_pred.unsqueeze(0)
    if src3.stride(-1) != 1:
        src3 = src3.contiguous()
    B, Gs, K = src3.shape
    if Gs != len(global_lats) * len(global_lons):
        raise ValueError(f"global prediction has {Gs} rows, the axes give {len(global_lats) * len(global_lons)}")
    cell, w = _device_tables(global_lats, global_lons, region_lats, region_lons, src3.device)
    out = torch.empty(B, cell.shape[0], K, dtype=torch.float32, device=src3.device)
    hip.regrid_blend(src3, len(global_lats), cell, w, K, g3=out)
    return out if global_pred.dim() == 3 else out[0]


def interpolate_field_2d(field_2d, src_lons, src_lats, dst_lons, dst_lats):
    """A field [len(src_lons), len(src_lats)] (float32 or float64, on the device) onto (len(dst_lons), len(dst_lats)),
    float32: the float64 bilinear value rounded once."""
    n_lon, n_lat = field_2d.shape
    if (n_lon, n_lat) != (len(src_lons), len(src_lats)):
        raise ValueError(f"field of shape {tuple(field_2d.shape)} on axes of {len(src_lons)} x {len(src_lats)}")
    src3 = field_2d.contiguous().view(1, n_lon * n_lat, 1)
    cell, w = _device_tables(src_lats, src_lons, dst_lats, dst_lons, src3.device)
    out = torch.empty(1, cell.shape[0], 1, dtype=torch.float32, device=src3.device)
    hip.regrid_blend(src3, n_lat, cell, w, 1, g3=out)
    return out.view(len(dst_lons), len(dst_lats))


# ======================================================================================================================
# Taper blending (scripts/predict_pipeline.py:135-149, :326)
# ======================================================================================================================
def build_taper_mask_2d(n_lat: int, n_lon: int, taper_width: int) -> torch.Tensor:
    """float32 (n_lon * n_lat, 1), longitude-major: 1 inside; a node whose distance to the nearest border along either
    axis is d < taper_width gets (d + 1) / (taper_width + 1) (the smaller of the two).  A width larger than an axis is
    an IndexError, as in the reference."""
    if taper_width > n_lat or taper_width > n_lon:
        raise IndexError(f"taper width {taper_width} exceeds the {n_lon} x {n_lat} grid")

    def ramp(n):
        d = np.minimum(np.arange(n), np.arange(n)[::-1])
        a = np.ones(n, dtype=np.float32)
        edge = d < taper_width
        a[edge] = ((d[edge] + 1) / (taper_width + 1)).astype(np.float32)
        return a
    mask = np.minimum(ramp(n_lon)[:, None], ramp(n_lat)[None, :])
    return torch.from_numpy(np.ascontiguousarray(mask).reshape(-1, 1))


def taper_blend(mask: torch.Tensor, r: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """`mask * r + (1 - mask) * g` on the device (float32, the reference's operation order): mask (G, 1), r and g
    (G, K) (or [B, G, K])."""
    r3 = r if r.dim() == 3 else r.unsqueeze(0)
    g3 = g if g.dim() == 3 else g.unsqueeze(0)
    r3, g3 = hip._rows_view(r3), hip._rows_view(g3)
    if r3.shape != g3.shape:
        raise ValueError(f"taper_blend: r {tuple(r.shape)} and g {tuple(g.shape)} differ")
    m = mask.reshape(-1).to(device=r3.device, dtype=torch.float32).contiguous()
    out = torch.empty(r3.shape, dtype=torch.float32, device=r3.device)
    hip.taper_blend(m, r3, g3, out)
    return out if r.dim() == 3 else out[0]


# ======================================================================================================================
# Global model + regional model + blending (scripts/predict_pipeline.py:300-329)
# ======================================================================================================================
class GlobalRegionalForecast:
    """Plan B of `scripts/predict_pipeline.py`: one forward of the global model, its forecast regridded onto the
    regional grid, one forward of the regional model, the two blended with the taper mask; all trimmed to the common
    `horizons * C` columns.  Returns `(blended, regional, global_interpolated)`.

    global_coords / region_coords: (lats, lons) axes (the regional ones may be descending).  `horizons`: the reference's
    P = min(P_global, P_regional); None takes what both models' outputs cover.  A model whose single forward returns
    fewer than P * C columns is an error (the reference would fail later with a shape error)."""

    def __init__(self, global_model, regional_model, global_coords, region_coords, taper_width: int = 3,
                 horizons: Optional[int] = None, num_channels: Optional[int] = None):
        self.global_model, self.regional_model = global_model, regional_model
        self.g_lats, self.g_lons = (np.asarray(a) for a in global_coords)
        self.r_lats, self.r_lons = (np.asarray(a) for a in region_coords)
        self.C = int(num_channels if num_channels is not None else global_model.num_features)
        self.horizons, self.taper_width = horizons, taper_width
        self.taper_mask = build_taper_mask_2d(len(self.r_lats), len(self.r_lons), taper_width)
        self.device = next(global_model.parameters()).device
        self._mask_dev = self.taper_mask.reshape(-1).to(self.device)
        self._cell, self._w = _device_tables(self.g_lats, self.g_lons, self.r_lats, self.r_lons, self.device)

    def _width(self, g_out, r_out) -> int:
        if self.horizons is None:
            P = min(g_out.shape[-1], r_out.shape[-1]) // self.C
            if P < 1:
                raise ValueError(f"the models return {g_out.shape[-1]} and {r_out.shape[-1]} columns, fewer than "
                                 f"one step of {self.C} channels")
            return P * self.C
        PC = int(self.horizons) * self.C
        for name, o in (("global", g_out), ("regional", r_out)):
            if o.shape[-1] < PC:
                raise ValueError(f"the {name} model returns {o.shape[-1]} columns per forward, fewer than the "
                                 f"{self.horizons} horizons x {self.C} channels = {PC} this forecast blends "
                                 f"(a one-step model needs an autoregressive rollout)")
        return PC

    def forward(self, gX: torch.Tensor, rX: torch.Tensor):
        g_out = self.global_model(gX, attention_threshold=0.0)
        r_out = self.regional_model(rX, attention_threshold=0.0)
        squeeze = g_out.dim() == 2
        g3 = g_out if g_out.dim() == 3 else g_out.unsqueeze(0)
        r3 = r_out if r_out.dim() == 3 else r_out.unsqueeze(0)
        if g3.shape[0] != r3.shape[0]:
            raise ValueError(f"global batch {g3.shape[0]} vs regional batch {r3.shape[0]}")
        if g3.shape[1] != len(self.g_lats) * len(self.g_lons) or r3.shape[1] != len(self.r_lats) * len(self.r_lons):
            raise ValueError("model output rows do not match the grid axes")
        g3, r3 = hip._rows_view(g3), hip._rows_view(r3)
        PC = self._width(g3, r3)
        B, nt = g3.shape[0], self._cell.shape[0]
        g_interp = torch.empty(B, nt, PC, dtype=torch.float32, device=g3.device)
        blended = torch.empty(B, nt, PC, dtype=torch.float32, device=g3.device)
        hip.regrid_blend(g3, len(self.g_lats), self._cell, self._w, PC, g3=g_interp, mask=self._mask_dev, r3=r3,
                         out3=blended)
        regional = r3[..., :PC]
        if squeeze:
            return blended[0], regional[0], g_interp[0]
        return blended, regional, g_interp

    @torch.no_grad()
    def __call__(self, gX: torch.Tensor, rX: torch.Tensor):
        return self.forward(gX, rX)


class CapturedGlobalRegionalForecast(GlobalRegionalForecast, Captured):
    """`GlobalRegionalForecast` replayed from a hipGraph (capture.Captured): both forwards, the regrid and the blend
    cost the host one graph launch.  Returns fresh tensors (copies of the graph's outputs)."""

    def __init__(self, *args, use_graph: bool = True, **kw):
        GlobalRegionalForecast.__init__(self, *args, **kw)
        Captured.__init__(self, use_graph=use_graph, recapture=True)

    def _work(self, gX, rX):
        return self.forward(gX, rX)

    @torch.no_grad()
    def __call__(self, gX: torch.Tensor, rX: torch.Tensor):
        if getattr(self.global_model, "using_sparse_gat", False) or getattr(self.regional_model, "using_sparse_gat",
                                                                            False):
            return self._work(gX, rX)
        out = self._run(gX, rX)
        return tuple(t.clone() for t in out) if out is self._result else out


# ======================================================================================================================
# Per-grid-point error maps (scripts/metrics_maps.py)
# ======================================================================================================================
_MAP_STATS = ("rmse", "mae", "bias", "acc")
_STAT_SUM = {"bias": hip.MAPS_SUM_E, "rmse": hip.MAPS_SUM_SQ, "mae": hip.MAPS_SUM_ABS, "acc": hip.MAPS_SUM_PT}
_STAT_KIND = {"rmse": hip.MAPS_RMSE, "mae": hip.MAPS_MAE, "bias": hip.MAPS_BIAS, "acc": hip.MAPS_ACC}
_CONV_DENORM, _CONV_ZDIV = 1, 2

_UNITS_BY_NAME = {"t2m": ("K", 1.0, 0.0, None), "msl": ("hPa", 1 / 100.0, 0.0, None),
                  "tp": ("mm/6h", 1000.0, 0.0, None)}
_UNITS_BY_NAME.update({w: ("m/s", 1.0, 0.0, None) for w in ("10u", "10v", "u@850", "u@500", "v@850", "v@500")})
_UNITS_BY_PREFIX = (("t@", ("K", 1.0, 0.0, None)), ("z@", ("m", 1.0, 0.0, "z_to_m")),
                    ("q@", ("g/kg", 1000.0, 0.0, "q_to_gkg")))


def unit_label(name: str):
    """(label, factor, offset, special) of a variable (`scripts/metrics_maps.py:46-63`): the physical value is
    `value * factor + offset`, after a division by g0 when special is 'z_to_m' (geopotential -> metres); 'q_to_gkg'
    only names the factor 1000.  Unknown names: ("", 1.0, 0.0, None)."""
    hit = _UNITS_BY_NAME.get(name)
    if hit is not None:
        return hit
    for prefix, units in _UNITS_BY_PREFIX:
        if name.startswith(prefix):
            return units
    return ("", 1.0, 0.0, None)


def load_scaler_stats(dataset_dir):
    """The target scalers of a data set directory (`scripts/metrics_maps.py:29-38`): {"y_mean", "y_scale"} read from
    its `scalers.npz`, or None when the directory has none - `MetricMaps` then scores in standardised units, and a
    RuntimeWarning says so."""
    import os
    import warnings

    path = os.path.join(os.fspath(dataset_dir), "scalers.npz")
    try:
        with np.load(path) as scalers:
            return {key: scalers[key] for key in ("y_mean", "y_scale")}
    except FileNotFoundError:
        warnings.warn(f"{path} is missing: the error maps stay in standardised units", RuntimeWarning)
        return None


def _conv_rows(var_order, y_mean, y_scale, K: int):
    """float32 [K, 4] {scale, mean, factor, offset} and int32 [K] flags of gcl_maps_*; var_order / y_mean / y_scale
    already of length K or None."""
    conv = np.zeros((K, 4), dtype=np.float32)
    conv[:, 0], conv[:, 2] = 1.0, 1.0
    flags = np.zeros(K, dtype=np.int32)
    if y_mean is not None:
        conv[:, 0], conv[:, 1] = np.asarray(y_scale, dtype=np.float32), np.asarray(y_mean, dtype=np.float32)
        flags |= _CONV_DENORM
    if var_order is not None:
        for k, name in enumerate(var_order):
            _, factor, offset, special = unit_label(name)
            conv[k, 2], conv[k, 3] = np.float32(factor), np.float32(offset)
            if special == "z_to_m":
                flags[k] |= _CONV_ZDIV
    return conv, flags


def _device_conv(conv: np.ndarray, flags: np.ndarray, device):
    key = ("conv", conv.tobytes(), flags.tobytes(), str(device))
    t = _JOB_CACHE.get(key)
    if t is None:
        t = (torch.from_numpy(conv).to(device), torch.from_numpy(flags).to(device))
        _JOB_CACHE[key] = t
    return t


def _upload_i32(values, device) -> torch.Tensor:
    arr = np.ascontiguousarray(np.asarray(values, dtype=np.int32))
    key = ("i32", arr.tobytes(), str(device))
    t = _JOB_CACHE.get(key)
    if t is None:
        t = torch.from_numpy(arr).to(device)
        _JOB_CACHE[key] = t
    return t


def _need_gpu_f32(t, who: str):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{who} needs a tensor on the GPU (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: float32 expected, got {t.dtype}")


def inverse_standardize(Y: torch.Tensor, y_mean: np.ndarray, y_scale: np.ndarray) -> torch.Tensor:
    """`Y * y_scale + y_mean` over the last dimension of a float32 device tensor (`scripts/metrics_maps.py:40-44`),
    the product and the sum each rounded to float32 (gcl_maps_convert)."""
    _need_gpu_f32(Y, "inverse_standardize")
    K = Y.shape[-1]
    if np.size(y_mean) != K or np.size(y_scale) != K:
        raise ValueError(f"y_mean / y_scale of {np.size(y_mean)} / {np.size(y_scale)} entries for {K} columns")
    conv, flags = _device_conv(*_conv_rows(None, np.reshape(y_mean, -1), np.reshape(y_scale, -1), K), Y.device)
    return hip.maps_convert(Y, conv, flags)


def apply_units(arr: torch.Tensor, var_name: str):
    """(arr in the physical units of `var_name`, label) (`scripts/metrics_maps.py:65-73`): a true division by g0 for
    z@..., then `* factor + offset`, each rounded on its own, on a float32 device tensor (gcl_maps_convert; bit for bit
    the reference's CPU result)."""
    _need_gpu_f32(arr, "apply_units")
    label = unit_label(var_name)[0]
    conv, flags = _device_conv(*_conv_rows([var_name], None, None, 1), arr.device)
    return hip.maps_convert(arr.reshape(-1, 1), conv, flags).view(arr.shape), label


def _persistence_map(F: int, C: int, K: int, device) -> torch.Tensor:
    return _upload_i32(F - C + np.arange(K) % C, device)


class MetricMaps:
    """RMSE / MAE / bias / ACC at every grid node, per channel and lead time, in physical units: the maps
    `scripts/metrics_maps.py` draws (`compute_stat`, :75-90), accumulated batch by batch in a float64 device state
    instead of stacking the test set on the host.

    `update(y_true, y_pred)` takes device tensors [B, G, leads * C] (or [G, leads * C]); `y_pred` may be a
    `Persistence`.  Every value is de-normalised (`y_mean` / `y_scale`, per channel or per column; None: standardised
    units, the script without --denorm) and converted with `unit_label(var_order[c])` (None: as it is) in float32 exactly
    as the reference does, differences and sums are float64, and `update` never synchronises, so it can be replayed
    from a hipGraph (`CapturedMetricMaps`): the sample count is device state too.  Only the sums of the requested
    `stats` are kept.  `rows` (grid indices, e.g. `region_node_indices`) restricts the maps - and the field statistics
    of ACC - to those rows, in the order given.

    `maps(stat)` -> float32 [leads, rows, C] on the device; `map(stat, channel, lead)` -> [rows]; `skill(reference)`
    -> `1 - rmse / max(rmse_ref, 1e-9)` per element; `units`: the label of every channel; `n`: samples so far."""

    def __init__(self, num_channels: int, num_nodes: int, leads: int = 1, stats: Sequence[str] = _MAP_STATS,
                 var_order: Optional[Sequence[str]] = None, y_mean=None, y_scale=None, rows=None, device=None):
        self.C, self.G, self.leads = int(num_channels), int(num_nodes), int(leads)
        if self.C < 1 or self.G < 1 or self.leads < 1:
            raise ValueError(f"MetricMaps needs positive sizes, got C={self.C}, nodes={self.G}, leads={self.leads}")
        self.K = self.leads * self.C
        stats = (stats,) if isinstance(stats, str) else tuple(stats)
        for s in stats:
            if s not in _MAP_STATS:
                raise ValueError(f"unknown statistic {s!r}: one of {_MAP_STATS}")
        if not stats:
            raise ValueError("MetricMaps needs at least one statistic")
        self.stats = tuple(dict.fromkeys(stats))
        self._sums = 0
        for s in self.stats:
            self._sums |= _STAT_SUM[s]
        self._plane = {s: bin(self._sums & (_STAT_SUM[s] - 1)).count("1") for s in self.stats}
        if var_order is not None and len(var_order) != self.C:
            raise ValueError(f"var_order names {len(var_order)} channels, the maps have {self.C}")
        if (y_mean is None) != (y_scale is None):
            raise ValueError("y_mean and y_scale go together")
        if y_mean is not None:
            y_mean, y_scale = np.reshape(np.asarray(y_mean), -1), np.reshape(np.asarray(y_scale), -1)
            if y_mean.size != y_scale.size or y_mean.size not in (self.C, self.K):
                raise ValueError(f"y_mean / y_scale of {y_mean.size} / {y_scale.size} entries: expected {self.C} "
                                 f"(per channel) or {self.K} (per column)")
            if y_mean.size == self.C:
                y_mean, y_scale = np.tile(y_mean, self.leads), np.tile(y_scale, self.leads)
        self.var_order = None if var_order is None else list(var_order)
        self.units = [unit_label(v)[0] for v in self.var_order] if self.var_order is not None else [""] * self.C
        self._conv_host = None
        if var_order is not None or y_mean is not None:
            names = None if self.var_order is None else self.var_order * self.leads
            self._conv_host = _conv_rows(names, y_mean, y_scale, self.K)
        self.rows = None
        if rows is not None:
            self.rows = np.asarray(rows, dtype=np.int64).reshape(-1)
            if self.rows.size == 0 or self.rows.min() < 0 or self.rows.max() >= self.G:
                raise ValueError(f"rows must be a non-empty list of grid indices below {self.G}")
        self.num_rows = self.G if self.rows is None else int(self.rows.size)
        self.device = None
        self._state = self._count = self._conv = self._flags = self._rows_dev = None
        self._scratch = {}
        if device is not None:
            self._ensure(torch.device(device))

    # -- device state --------------------------------------------------------------------------------------------------
    def _ensure(self, device):
        if self.device is None:
            if device.type != "cuda":
                raise ValueError(f"MetricMaps lives on the GPU (there is no CPU path), got device {device}")
            self.device = device
            self._state = torch.zeros(self.leads, len(self._plane), self.num_rows * self.C, dtype=torch.float64,
                                      device=device)
            self._count = torch.zeros(1, dtype=torch.int64, device=device)
            if self._conv_host is not None:
                self._conv, self._flags = _device_conv(*self._conv_host, device)
            if self.rows is not None:
                self._rows_dev = _upload_i32(self.rows, device)
        elif device != self.device:
            raise ValueError(f"MetricMaps lives on {self.device}, got tensors on {device}")

    def reset(self):
        """Zero every sum and the sample count (in place: a captured update keeps pointing at them)."""
        if self._state is not None:
            self._state.zero_()
            self._count.zero_()

    @property
    def n(self) -> int:
        """Samples accumulated so far, read from the device."""
        return 0 if self._count is None else int(self._count.item())

    def _inputs(self, y_true, y_pred):
        """(truth [B, G, K], prediction or window [B, G, W], column map or None), validated once."""
        persist = isinstance(y_pred, Persistence)
        src = y_pred.X if persist else y_pred
        for name, t in (("y_true", y_true), ("y_pred", src)):
            if not torch.is_tensor(t) or t.dim() not in (2, 3):
                raise ValueError(f"MetricMaps.update: {name} must be a tensor [B, G, K] or [G, K], got "
                                 f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        T3 = y_true if y_true.dim() == 3 else y_true.unsqueeze(0)
        P3 = src if src.dim() == 3 else src.unsqueeze(0)
        width_ok = (P3.shape[2] >= self.C and y_pred.C == self.C) if persist else P3.shape[2] == self.K
        if T3.shape[1:] != (self.G, self.K) or P3.shape[:2] != T3.shape[:2] or not width_ok:
            raise ValueError(f"MetricMaps.update: truth {tuple(y_true.shape)} and prediction {tuple(src.shape)}, "
                             f"expected {self.G} rows of {self.leads} leads x {self.C} channels = {self.K} columns"
                             + (f" (persistence window of {y_pred.C} channels)" if persist else ""))
        if not (T3.is_cuda and P3.is_cuda):
            raise ValueError("MetricMaps.update: y_true and y_pred must be on the GPU (there is no CPU path)")
        T3, P3 = hip._rows_view(T3), hip._rows_view(P3)
        return T3, P3, (_persistence_map(P3.shape[2], self.C, self.K, T3.device) if persist else None)

    def _update3(self, T3, P3, cmap):
        cs = None
        if self._sums & hip.MAPS_SUM_PT:
            B = T3.shape[0]
            cs = self._scratch.get(B)
            if cs is None:
                cs = self._scratch[B] = torch.empty(B, self.K, 4, dtype=torch.float64, device=T3.device)
            hip.maps_colstats(T3, P3, cmap, self._rows_dev, self._conv, self._flags, cs)
        hip.maps_accumulate(T3, P3, cmap, self._rows_dev, self._conv, self._flags, cs, self._sums, self.C, self._state,
                            self._count)

    def update(self, y_true: torch.Tensor, y_pred):
        """Add the B samples of y_true / y_pred [B, G, leads * C] (or one, [G, leads * C]) in order.  No host
        synchronisation."""
        T3, P3, cmap = self._inputs(y_true, y_pred)
        self._ensure(T3.device)
        self._update3(T3, P3, cmap)

    # -- results -------------------------------------------------------------------------------------------------------
    def _need(self, stat: str):
        if stat not in _MAP_STATS:
            raise ValueError(f"unknown statistic {stat!r}: one of {_MAP_STATS}")
        if stat not in self._plane:
            raise ValueError(f"statistic {stat!r} was not accumulated (stats={self.stats})")

    def maps(self, stat: str) -> torch.Tensor:
        """float32 [leads, rows, C]: the statistic at every scored node (zeros before the first update)."""
        self._need(stat)
        out = torch.zeros(self.leads, self.num_rows, self.C, dtype=torch.float32, device=self.device)
        if self._state is not None:
            hip.maps_finalize(self._state, self._count, self._plane[stat], _STAT_KIND[stat], out)
        return out

    def map(self, stat: str, channel: int, lead: int = 0) -> torch.Tensor:
        """[rows]: one channel's field, the `stat_map` the script hands to `plot_field`."""
        return self.maps(stat)[lead, :, channel]

    def skill(self, reference_maps: "MetricMaps") -> torch.Tensor:
        """float32 [leads, rows, C]: `1 - rmse / max(rmse_ref, 1e-9)` per element against another accumulator (e.g.
        persistence), from the two float32 RMSE maps."""
        self._need("rmse")
        reference_maps._need("rmse")
        if (reference_maps.leads, reference_maps.num_rows, reference_maps.C) != (self.leads, self.num_rows, self.C):
            raise ValueError("skill: the two accumulators have different shapes")
        if self._state is None or reference_maps._state is None:
            raise ValueError("skill: both accumulators need at least one update")
        out = torch.empty(self.leads, self.num_rows, self.C, dtype=torch.float32, device=self.device)
        hip.maps_finalize(self._state, self._count, self._plane["rmse"], hip.MAPS_SKILL, out,
                          ref_state=reference_maps._state, ref_count=reference_maps._count,
                          ref_plane=reference_maps._plane["rmse"])
        return out

    @staticmethod
    def to_grid(field, num_lon: int, num_lat: int) -> np.ndarray:
        """The [lat, lon] array `plot_field` hands to imshow (`scripts/metrics_maps.py:94`) for a field [G] numbered
        longitude-major.  Copies to the host; plotting itself is not provided."""
        arr = field.detach().cpu().numpy() if torch.is_tensor(field) else np.asarray(field)
        return arr.reshape(num_lon, num_lat).T


class CapturedMetricMaps(MetricMaps, Captured):
    """`MetricMaps` whose update (field statistics + accumulate) is replayed from a hipGraph (capture.Captured): the
    first two updates of a shape run eagerly, the third captures, later ones copy their inputs into the captured
    buffers and replay.  The sums and the sample count are device state, so a replay counts like an eager update and
    gives the same bits.  Falls back to eager launches if capture is not possible (see `.launch_mode`)."""

    def __init__(self, *args, use_graph: bool = True, **kw):
        MetricMaps.__init__(self, *args, **kw)
        Captured.__init__(self, use_graph=use_graph, recapture=True)
        self._cmap, self._cmap_key = None, None

    def _work(self, T3, P3):
        MetricMaps._update3(self, T3, P3, self._cmap)

    def _update3(self, T3, P3, cmap):
        key = None if cmap is None else cmap.data_ptr()
        if key != self._cmap_key:  # tensor prediction <-> persistence window: another set of launches
            self.reset_graph()
            self._cmap, self._cmap_key = cmap, key
        self._run(T3, P3)


def compute_stat(pred: torch.Tensor, true: torch.Tensor, stat: str) -> torch.Tensor:
    """The one-shot form of `scripts/metrics_maps.py:75-90`: pred / true [N, G] device tensors already in physical
    units -> the statistic at every node [G] (float32), through the kernels of `MetricMaps` (N samples of one
    channel)."""
    if stat not in _MAP_STATS:
        raise ValueError(stat)
    if pred.dim() != 2 or pred.shape != true.shape:
        raise ValueError(f"compute_stat: pred {tuple(pred.shape)} and true {tuple(true.shape)}, expected two [N, G]")
    mm = MetricMaps(1, pred.shape[1], stats=(stat,))
    mm.update(true.unsqueeze(-1), pred.unsqueeze(-1))
    return mm.maps(stat)[0, :, 0]


def metric_maps(model, dataset, indices=None, ar_steps: int = 1, batch_size: int = 8, use_residual: bool = True,
                static_channels=None, forcing_channels=None, persistence: bool = False, captured: bool = True,
                **maps_kw):
    """The evaluation loop of `scripts/metrics_maps.py:143-176` without its host side: for every batch of `indices`
    (None: the whole data set) `dataset.batch(...)` -> `predict.rollout` over `ar_steps` (a `CapturedRollout` with
    `captured`) -> `MetricMaps.update` against the first `ar_steps` steps of the truth.  `maps_kw` go to `MetricMaps`
    (stats, var_order, y_mean, y_scale, rows); channels, nodes and leads come from the data.  Returns the accumulator,
    or with `persistence` the pair (model, persistence) - the second fed by `Persistence` views of the input window.
    Nothing crosses to the host before a map or `n` is read."""
    from . import predict

    idx = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
    if not idx:
        raise ValueError("metric_maps: no samples to score")
    if batch_size < 1 or ar_steps < 1:
        raise ValueError(f"metric_maps: batch_size={batch_size}, ar_steps={ar_steps}")
    cls = CapturedMetricMaps if captured else MetricMaps
    roll = predict.CapturedRollout(model, ar_steps, static_channels=static_channels, forcing_channels=forcing_channels,
                                   use_residual=use_residual) if captured else None
    mm = base = None
    with torch.no_grad():
        for s in range(0, len(idx), batch_size):
            X, Y = dataset.batch(idx[s:s + batch_size])
            C = X.shape[-1] // model.obs_window
            if mm is None:
                if Y.shape[-1] < ar_steps * C:
                    raise ValueError(f"metric_maps: the data set's truth covers {Y.shape[-1] // C} steps, "
                                     f"ar_steps={ar_steps}")
                mm = cls(C, X.shape[1], leads=ar_steps, **maps_kw)
                base = cls(C, X.shape[1], leads=ar_steps, **maps_kw) if persistence else None
            truth = Y[..., :ar_steps * C]
            yf = Y if forcing_channels else None
            if captured:
                pred = roll(X, yf)
            else:
                pred = predict.rollout(model, X, ar_steps, y=yf, static_channels=static_channels,
                                       forcing_channels=forcing_channels, use_residual=use_residual)
            mm.update(truth, pred)
            if base is not None:
                base.update(truth, Persistence(X, C))
    return (mm, base) if persistence else mm


# ======================================================================================================================
# Regional scoring of a saved global forecast (scripts/interpolate_to_region.py)
# ======================================================================================================================
class _Moments:
    """Count, means, centred second moments and co-moment of (t, v) over a set of values; `+` pools two sets with the
    pairwise update of Chan et al., so that the pooled moments are centred on the pooled means (what `compute_acc` of
    interpolate_to_region.py:76-81 does) without ever forming an uncentred sum."""

    def __init__(self, n=0.0, mt=0.0, mv=0.0, m2t=0.0, m2v=0.0, ctv=0.0):
        self.n, self.mt, self.mv, self.m2t, self.m2v, self.ctv = n, mt, mv, m2t, m2v, ctv

    @classmethod
    def of_sums(cls, s):
        """From one (horizon, channel) row of gcl_region_interp_scores: sums of t' = t - tp and v' = v - vp."""
        n, St, Stt, Sv, Svv, Stv, tp, vp = s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10]
        if n == 0:
            return cls()
        return cls(n, tp + St / n, vp + Sv / n, max(Stt - St * (St / n), 0.0), max(Svv - Sv * (Sv / n), 0.0),
                   Stv - St * (Sv / n))

    def __add__(self, o):
        if self.n == 0:
            return o
        if o.n == 0:
            return self
        n = self.n + o.n
        dt, dv = o.mt - self.mt, o.mv - self.mv
        f = self.n * o.n / n
        return _Moments(n, self.mt + dt * (o.n / n), self.mv + dv * (o.n / n), self.m2t + o.m2t + dt * dt * f,
                        self.m2v + o.m2v + dv * dv * f, self.ctv + o.ctv + dt * dv * f)

    @property
    def acc(self) -> float:
        return float(self.ctv / (np.sqrt(self.m2t) * np.sqrt(self.m2v) + 1e-8))


class RegionBundleScores:
    """The scores of scripts/interpolate_to_region.py:204-249 from the float64 sums [P, C, 11] of
    `gcl_region_interp_scores`: `horizon(p)`, `channel(p, c)` and `overall` return dictionaries with rmse, base (the
    persistence RMSE), skill, acc (and mae per horizon).  `n_matched` of `n_samples` samples were inside the regional
    series; `n_nodes` regional nodes."""

    def __init__(self, sums, n_matched: int, n_samples: int, n_nodes: int):
        self.sums = np.asarray(sums, dtype=np.float64)
        self.P, self.C = self.sums.shape[:2]
        self.n_matched, self.n_samples, self.n_nodes = int(n_matched), int(n_samples), int(n_nodes)
        self.interpolated = self.truth = None  # float32 [n_matched, P, n_lon_r, n_lat_r, C] when they were kept

    def _pool(self, cells):
        s = np.stack([self.sums[p, c] for p, c in cells])
        n = s[:, 3].sum()
        rmse, base = float(np.sqrt(s[:, 0].sum() / n)), float(np.sqrt(s[:, 2].sum() / n))
        mom = _Moments()
        for row in s:
            mom = mom + _Moments.of_sums(row)
        return {"rmse": rmse, "base": base, "mae": float(s[:, 1].sum() / n), "skill": 1.0 - rmse / (base + 1e-12),
                "acc": mom.acc, "n": int(n)}

    def horizon(self, p: int) -> dict:
        return self._pool([(p, c) for c in range(self.C)])

    def channel(self, p: int, c: int) -> dict:
        return self._pool([(p, c)])

    @property
    def overall(self) -> dict:
        return self._pool([(p, c) for p in range(self.P) for c in range(self.C)])

    def report(self, variables, per_channel: bool = False, say=print):
        """The script's per-horizon lines, its `--per-channel` rows and its overall block."""
        for p in range(self.P):
            h = self.horizon(p)
            say(f"\n  +{(p + 1) * 6:02d}h: RMSE={h['rmse']:.6f} | base={h['base']:.6f} | skill={h['skill'] * 100:.2f}% | "
                f"MAE={h['mae']:.6f} | ACC={h['acc']:.4f}")
            if per_channel:
                for c in range(self.C):
                    k = self.channel(p, c)
                    say(f"    {c:2d}: {variables[c]:>8s}  RMSE={k['rmse']:.4f} base={k['base']:.4f} "
                        f"skill={k['skill'] * 100:+.1f}% ACC={k['acc']:.4f}")
        o = self.overall
        say(f"\n{'=' * 70}")
        say(f"Overall ({self.n_matched}×{self.P} horizons × {self.n_nodes} nodes × {self.C} ch):")
        say(f"  RMSE={o['rmse']:.6f} | base={o['base']:.6f} | skill={o['skill'] * 100:.2f}% | ACC={o['acc']:.4f}")
        say(f"{'=' * 70}")


def match_regional_steps(sample_offsets, obs_window: int, time_offset: int, P: int, n_time: int) -> np.ndarray:
    """int32 [N]: the regional step of horizon 0 of every sample (local_t + obs_window + time_offset), or -1 where the
    forecast or its persistence step falls outside the regional series (interpolate_to_region.py:169-176)."""
    t0 = np.full(len(sample_offsets), -1, dtype=np.int32)
    for s, local_t in enumerate(sample_offsets):
        start = int(local_t) + obs_window + time_offset
        if start < 0 or start + P > n_time or start - 1 < 0:
            continue
        t0[s] = start
    return t0


def interpolate_to_region(predictions, global_data, region_data, per_channel: bool = False, out=None, device=None,
                          say=print) -> RegionBundleScores:
    """`scripts/interpolate_to_region.py`: the forecasts of a `predictions.pt` bundle (`predict.save_predictions`, or
    the bare tensor of the legacy form) interpolated from the global grid of `global_data` onto the regional grid of
    `region_data` and scored against the regional fp16 series, with persistence (the regional step before the
    forecast) as the baseline.  Samples are matched to regional steps on the host; the regional series is uploaded
    once; every matched sample, horizon, node and channel is interpolated and scored in one launch pair
    (`gcl_region_interp_scores`), with one host read of [P, C, 11] sums.  Prints the script's lines; with `out` writes
    its bundle (interpolated forecasts and regional truth as float32 [n, P, n_lon, n_lat, C])."""
    import json
    import os
    from datetime import datetime

    from .data import _upload_fp16
    from .predict import load_predictions

    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("interpolate_to_region needs a GPU (the HIP path has no CPU fallback)")
        device = "cuda:0"
    device = torch.device(device)
    global_dir, region_dir = str(global_data), str(region_data)
    read_json = lambda d, f: json.load(open(os.path.join(d, f)))  # noqa: E731

    def coords(d):
        z = np.load(os.path.join(d, "coords.npz"))
        return z["latitude"].astype(np.float64), z["longitude"].astype(np.float64)

    g_lats, g_lons = coords(global_dir)
    var_file = os.path.join(global_dir, "variables.json")
    sav = load_predictions(predictions)
    if isinstance(sav, dict):
        preds = sav["predictions"]
        C, P = int(sav["n_features"]), int(sav["ar_steps"])
        n_lon_g, n_lat_g = int(sav["n_lon"]), int(sav["n_lat"])
        OBS = int(sav.get("obs_window", 2))
        offsets = list(sav.get("sample_offsets", range(len(preds))))
    else:  # the bare tensor: the grid and the channel count come from the global data set
        preds = sav
        n_lon_g, n_lat_g = len(g_lons), len(g_lats)
        if not os.path.exists(var_file):
            raise ValueError("a bare prediction tensor needs the global data set's variables.json for its channel count")
        C = len(read_json(global_dir, "variables.json"))
        P, OBS, offsets = preds.shape[-1] // C, 2, list(range(len(preds)))
    N = preds.shape[0]
    if preds.dim() != 3 or preds.shape[1] != n_lon_g * n_lat_g or preds.shape[2] != P * C:
        raise ValueError(f"predictions {tuple(preds.shape)} are not [N, {n_lon_g * n_lat_g}, {P * C}]")
    say(f"Loaded {N} predictions: grid={n_lon_g}×{n_lat_g}, C={C}, P={P}")
    g_info = read_json(global_dir, "dataset_info.json")
    g_start = datetime.strptime(g_info["time_start"], "%Y-%m-%d")
    say(f"Global: {g_info['time_start']}–{g_info['time_end']}  lon=[{g_lons[0]:.2f}..{g_lons[-1]:.2f}]  "
        f"lat=[{g_lats[0]:.2f}..{g_lats[-1]:.2f}]")
    r_lats, r_lons = coords(region_dir)
    scl = np.load(os.path.join(region_dir, "scalers.npz"))
    r_mean, r_std = scl["mean"].astype(np.float64), scl["std"].astype(np.float64)
    r_info = read_json(region_dir, "dataset_info.json")
    r_start = datetime.strptime(r_info["time_start"], "%Y-%m-%d")
    n_lon_r, n_lat_r = int(r_info["n_lon"]), int(r_info["n_lat"])
    n_feat_r = int(r_info.get("n_features", r_info.get("n_feat", C)))
    n_time_r = int(r_info["n_time"])
    G_region = n_lon_r * n_lat_r
    say(f"Region: {r_info['time_start']}–{r_info['time_end']}  lon=[{r_lons[0]:.2f}..{r_lons[-1]:.2f}]  "
        f"lat=[{r_lats[0]:.2f}..{r_lats[-1]:.2f}]  grid={n_lon_r}×{n_lat_r}={G_region}")
    if (len(r_lons), len(r_lats)) != (n_lon_r, n_lat_r) or n_feat_r < C:
        raise ValueError(f"regional data set: axes of {len(r_lons)} x {len(r_lats)} and {n_feat_r} features for a grid of "
                         f"{n_lon_r} x {n_lat_r} and {C} channels")
    time_offset = int((g_start - r_start).total_seconds() / (6 * 3600))
    say(f"Temporal offset: global starts {time_offset} steps after regional")
    raw = np.memmap(os.path.join(region_dir, "data.npy"), dtype=np.float16, mode="r")
    series = _upload_fp16(raw.reshape(n_time_r, G_region, n_feat_r), device)
    say(f"Regional data loaded: {(n_time_r, n_lon_r, n_lat_r, n_feat_r)}")
    variables = read_json(global_dir, "variables.json") if os.path.exists(var_file) else [f"ch{i}" for i in range(C)]
    say(f"\n{'=' * 70}")
    say(f"Interpolating {N} global samples → {n_lon_r}×{n_lat_r} regional grid")
    say(f"{'=' * 70}")
    t0 = match_regional_steps(offsets, OBS, time_offset, P, n_time_r)
    matched = np.nonzero(t0 >= 0)[0]
    say(f"\nMatched samples: {len(matched)}/{N}")
    if len(matched) == 0:
        say("ERROR: no temporal overlap. Check dataset dates.")
        raise SystemExit(1)
    cell, w = _device_tables(g_lats, g_lons, r_lats, r_lons, device)
    pred3 = hip._rows_view(preds.to(device))
    sums = torch.empty(P, C, hip.REGION_NS, dtype=torch.float64, device=device)
    vout = tout = None
    if out:
        vout = torch.empty(N, P, G_region, C, dtype=torch.float32, device=device)
        tout = torch.empty_like(vout)
    hip.region_interp_scores(pred3, n_lat_g, cell, w, series, torch.from_numpy(t0).to(device), int(matched[0]),
                             torch.from_numpy(r_mean[:C].copy()).to(device), torch.from_numpy(r_std[:C].copy()).to(device),
                             P, C, sums, vout, tout)
    res = RegionBundleScores(sums.cpu().numpy(), len(matched), N, G_region)
    res.report(variables, per_channel=per_channel, say=say)
    if out:
        keep = torch.from_numpy(matched).to(device)
        shape = (len(matched), P, n_lon_r, n_lat_r, C)
        res.interpolated = vout.index_select(0, keep).cpu().view(shape)
        res.truth = tout.index_select(0, keep).cpu().view(shape)
        torch.save({"interpolated_predictions": res.interpolated, "regional_ground_truth": res.truth,
                    "variables": variables[:C], "region_lats": r_lats, "region_lons": r_lons, "n_matched": len(matched),
                    "scalers_mean": r_mean[:C], "scalers_std": r_std[:C]}, str(out))
        say(f"Saved interpolated: {out}")
    return res


def build_parser():
    import argparse

    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.verify",
                                 description="Interpolate global predictions to regional grid")
    ap.add_argument("--predictions", required=True, help="predictions .pt saved by graphcast_lite_amd.predict --save")
    ap.add_argument("--global-data", required=True, help="global dataset directory")
    ap.add_argument("--region-data", required=True, help="regional dataset directory")
    ap.add_argument("--per-channel", action="store_true")
    ap.add_argument("--out", default=None, help="save the interpolated predictions as .pt")
    return ap


def main(argv=None, device=None):
    """`python -m graphcast_lite_amd.verify --predictions p.pt --global-data g --region-data r [--per-channel] [--out o.pt]`
    with the options of scripts/interpolate_to_region.py."""
    import sys

    a = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    return interpolate_to_region(a.predictions, a.global_data, a.region_data, per_channel=a.per_channel, out=a.out,
                                 device=device)


if __name__ == "__main__":
    main()
