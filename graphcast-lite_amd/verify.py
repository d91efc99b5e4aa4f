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

Kernels: csrc/verify.hip.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured

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
def find_cells(grid, x):
    """(cell index, normalised distance) of every x on an ascending axis, as scipy's RegularGridInterpolator finds
    them: the cell [grid[i], grid[i+1]) holding x, clipped to [0, n-2] (x below the first node: cell 0, x on or past
    the last node: cell n-2), distance (x - grid[i]) / (grid[i+1] - grid[i]) in float64 (outside [0, 1] when
    extrapolating)."""
    grid = np.asarray(grid, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if grid.ndim != 1 or grid.size < 2 or not np.all(np.diff(grid) > 0):
        raise ValueError("the source axes must be strictly ascending with at least 2 points")
    i = np.clip(np.searchsorted(grid, x, side="right") - 1, 0, grid.size - 2)
    return i.astype(np.int64), (x - grid[i]) / (grid[i + 1] - grid[i])


def regrid_tables(src_lats, src_lons, dst_lats, dst_lons):
    """Host tables of the bilinear regrid from the (src_lons, src_lats) grid onto the targets (dst_lons[j],
    dst_lats[i]), numbered longitude-major (j * len(dst_lats) + i): int32 [nt, 2] cells (lon, lat) and float64 [nt, 4]
    weights of the corners (lon, lat), (lon, lat+1), (lon+1, lat), (lon+1, lat+1), each formed as 1 * w_lon * w_lat."""
    ilon, ylon = find_cells(src_lons, dst_lons)
    ilat, ylat = find_cells(src_lats, dst_lats)
    nj, ni = len(ilon), len(ilat)
    cell = np.empty((nj, ni, 2), dtype=np.int32)
    cell[..., 0] = ilon[:, None]
    cell[..., 1] = ilat[None, :]
    one = np.float64(1.0)
    lon_w = ((one * (1 - ylon))[:, None], (one * ylon)[:, None])
    lat_w = ((1 - ylat)[None, :], ylat[None, :])
    w = np.empty((nj, ni, 4), dtype=np.float64)
    w[..., 0] = lon_w[0] * lat_w[0]
    w[..., 1] = lon_w[0] * lat_w[1]
    w[..., 2] = lon_w[1] * lat_w[0]
    w[..., 3] = lon_w[1] * lat_w[1]
    return cell.reshape(-1, 2), w.reshape(-1, 4)


def regrid_tables_latlon(src_lats, src_lons, dst_lats, dst_lons):
    """`regrid_tables` for an interpolator whose axes are (lats, lons) (scripts/build_multires_dataset.py:220-224),
    targets (dst_lats[i], dst_lons[j]) numbered latitude-major (i * len(dst_lons) + j): int32 [nt, 2] cells (lat, lon)
    and float64 [nt, 4] weights of the corners (lat, lon), (lat, lon+1), (lat+1, lon), (lat+1, lon+1), each formed as
    (1 * w_lat) * w_lon.  The products equal those of `regrid_tables`; the ORDER of the corners is what differs, and
    with it the float64 sum."""
    ilat, ylat = find_cells(src_lats, dst_lats)
    ilon, ylon = find_cells(src_lons, dst_lons)
    ni, nj = len(ilat), len(ilon)
    cell = np.empty((ni, nj, 2), dtype=np.int32)
    cell[..., 0] = ilat[:, None]
    cell[..., 1] = ilon[None, :]
    one = np.float64(1.0)
    lat_w = ((one * (1 - ylat))[:, None], (one * ylat)[:, None])
    lon_w = ((1 - ylon)[None, :], ylon[None, :])
    w = np.empty((ni, nj, 4), dtype=np.float64)
    w[..., 0] = lat_w[0] * lon_w[0]
    w[..., 1] = lat_w[0] * lon_w[1]
    w[..., 2] = lat_w[1] * lon_w[0]
    w[..., 3] = lat_w[1] * lon_w[1]
    return cell.reshape(-1, 2), w.reshape(-1, 4)


_TABLES = {}


def _device_tables(src_lats, src_lons, dst_lats, dst_lons, device):
    axes = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in (src_lats, src_lons, dst_lats, dst_lons)]
    key = tuple((a.tobytes(), a.size) for a in axes) + (str(device),)
    t = _TABLES.get(key)
    if t is None:
        cell, w = regrid_tables(*axes)
        t = (torch.from_numpy(cell).to(device), torch.from_numpy(w).to(device))
        _TABLES[key] = t
    return t


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
