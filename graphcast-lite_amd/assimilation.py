"""Data assimilation on the HIP path: drop-in for the reference's `src/assimilation/` (nudging and optimal
interpolation), plus a captured assimilated rollout.

`from src.assimilation.nudging import X` / `from src.assimilation.optimal_interpolation import X` become
`from graphcast_lite_amd.assimilation import X` with the same names, signatures and results:

* host helpers (`build_feature_mask`, `build_feature_mask_from_indices`, `cosine_taper_2d`,
  `build_boundary_taper_mask`), unchanged;
* `NudgingAssimilator`, `nudge_sequence_offline`, `sequential_nudged_rollout`: the blend is `gcl_nudge`, bit-equal to
  the reference's float32 torch arithmetic.  Tensors on the CPU are processed on the current GPU and returned on the
  CPU, as the reference's callers (`scripts/predict.py:569-571`) expect;
* `OptimalInterpolation`: matrix-free (csrc/assim.hip).  B is never built unless `.B` is read; the station covariance
  is factored once per station set (float64) and cached.

Beyond the reference: `OptimalInterpolation.prepare_network` (a fixed station network, capture-safe),
`assimilated_rollout` (`predict.rollout` with assimilation after each step) and `CapturedAssimilatedRollout`.

The DA grid search (`scripts/da_grid_search.sh`, `da_experiments_v2.sh`, `_v3.sh`, `_merge.sh`: one `predict.py` run
per setting): `DASetting`, `da_grid`, `station_network` and `DASweepAssimilator`, which assimilates every batch row of
one rollout with another setting (`gcl_nudge_rows`, `gcl_oi_analysis_rows`); `pipeline.DaSweep` scores the rows.
"""
import math
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .predict import CapturedRollout, channel_kinds

EARTH_RADIUS_M = 6371000.0


# ======================================================================================================================
# Host helpers (src/assimilation/nudging.py:10-54)
# ======================================================================================================================
def build_feature_mask(all_features: Sequence[str], assimilate_features: Sequence[str], pred_window: int,
                       device) -> torch.Tensor:
    """bool [pred_window * C]: the named features, repeated for every predicted step."""
    C = len(all_features)
    select = torch.zeros(C, dtype=torch.bool)
    name_to_idx = {n: i for i, n in enumerate(all_features)}
    for name in assimilate_features:
        if name in name_to_idx:
            select[name_to_idx[name]] = True
    return select.repeat(pred_window).to(device)


def build_feature_mask_from_indices(indices: Sequence[int], num_features: int, pred_window: int,
                                    device) -> torch.Tensor:
    """bool [pred_window * num_features]: the listed channel indices (out-of-range ones ignored), repeated."""
    C = int(num_features)
    select = torch.zeros(C, dtype=torch.bool)
    for idx in indices:
        if 0 <= idx < C:
            select[idx] = True
    return select.repeat(pred_window).to(device)


def cosine_taper_2d(lon: int, lat: int, border: int) -> torch.Tensor:
    """[lon, lat] outer product of two Hann edge ramps of width `border` (1 inside, 0 at the edges)."""
    if border <= 0:
        return torch.ones(lon, lat)

    def hann(N, b):
        w = np.ones(N, dtype=np.float32)
        t = np.linspace(0, 1, b)
        win = 0.5 * (1 - np.cos(np.pi * t))
        w[:b] = win
        w[-b:] = win[::-1]
        return w

    w_lon, w_lat = hann(lon, border), hann(lat, border)
    return torch.from_numpy(np.outer(w_lon, w_lat)).float()


def build_boundary_taper_mask(height, width, width_x, width_y):
    """Flat [G] blending mask for the boundary."""
    return cosine_taper_2d(width, height, max(width_x, width_y)).ravel()


# ======================================================================================================================
# Nudging (src/assimilation/nudging.py:60-206)
# ======================================================================================================================
def _work_device(t: torch.Tensor) -> torch.device:
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _as3(t: torch.Tensor) -> torch.Tensor:
    """[..., C] -> a [B, G, C] view (B = 1 for 1-D / 2-D input)."""
    if t.dim() == 1:
        return t.view(1, 1, -1)
    if t.dim() == 2:
        return t.unsqueeze(0)
    return t.reshape(-1, t.shape[-2], t.shape[-1])


def _nudge_coeffs(alpha: float):
    """(fl32(1 - alpha), fl32(alpha)): torch CPU rounds the Python scalar to the tensor's dtype."""
    alpha = float(alpha)
    return float(np.float32(1.0 - alpha)), float(np.float32(alpha))


def _nudge(forecast: torch.Tensor, observation: torch.Tensor, alpha: float, form: int, mask_u8=None) -> torch.Tensor:
    home = forecast.device
    dev = _work_device(forecast)
    f = forecast.to(dev, torch.float32).contiguous()
    o = observation.to(dev, torch.float32)
    out = torch.empty_like(f)
    c0, c1 = _nudge_coeffs(alpha)
    if f.numel():
        hip.nudge(_as3(f), _as3(o), _as3(out), c0, c1, form, mask_u8)
    return out.to(home)


class NudgingAssimilator:
    """x_a = x_b + alpha (y - x_b) wherever y is not NaN (and the feature mask, when its length equals the channel
    count, selects the channel).  `apply` accepts any `[..., C]` shape; a shape mismatch returns the forecast."""

    def __init__(self, alpha=0.25, device="cpu", feature_mask_flat=None, **kwargs):
        self.alpha = float(alpha)
        self.device = device
        self.mask_flat = feature_mask_flat
        if self.mask_flat is not None:
            self.mask_flat = self.mask_flat.to(device)
        self._mask_dev = {}

    def _mask_u8(self, C: int, dev: torch.device):
        if self.mask_flat is None or self.mask_flat.shape[0] != C:
            return None
        key = (C, str(dev))
        if key not in self._mask_dev:
            self._mask_dev[key] = self.mask_flat.to(dev, torch.uint8).contiguous()
        return self._mask_dev[key]

    def prepare(self, C: int, device) -> None:
        """Upload the channel mask for C channels on `device` ahead of a captured rollout."""
        self._mask_u8(C, torch.device(device))

    def apply(self, forecast, observation):
        if forecast.shape != observation.shape:
            return forecast
        return _nudge(forecast, observation, self.alpha, 0, self._mask_u8(forecast.shape[-1], _work_device(forecast)))

    def apply_(self, f3: torch.Tensor, o3: torch.Tensor) -> torch.Tensor:
        """In place on a device [B, G, C] view (unit channel stride): the rollout's form, no allocation or sync."""
        c0, c1 = _nudge_coeffs(self.alpha)
        return hip.nudge(f3, o3, f3, c0, c1, 0, self._mask_u8(f3.shape[-1], f3.device))


def nudge_sequence_offline(y_pred, y_obs, alpha=0.25, k=None):
    """(1 - alpha) y_pred + alpha y_obs wherever y_obs is not NaN (`k` is accepted and ignored, as in the reference)."""
    return _nudge(y_pred, y_obs, alpha, 1)


@torch.no_grad()
def sequential_nudged_rollout(model, x0, y_obs, p, alpha=0.25, k=None, device="cpu"):
    """The reference's nudged forecast (nudging.py:104-199), with the same three branches:

    * the model's output has P*C channels (multi-step model): one sequential-form nudge per sample over the
      whole horizon;
    * it has C channels (one-step model): P autoregressive steps, nudged while `k is None or step < k`, the raw output
      (no residual) shifted into the window;
    * any other width: the output unchanged.

    x0 [N, G, T_in, C], y_obs [N, G, P*C].  The model runs on `device`, the nudges on the GPU; returns CPU tensors."""
    N, G, T_in, C = x0.shape
    total_target_channels = y_obs.shape[-1]
    state = x0.to(device).contiguous()
    dev = state.device if state.is_cuda else _work_device(state)
    nudger = NudgingAssimilator(alpha=alpha, device=dev)
    out = model(state.view(N, G, -1), attention_threshold=0.0)
    if out.dim() == 2:
        out = out.unsqueeze(0)
    out = out.to(dev)
    if out.shape[-1] == total_target_channels:
        yo = y_obs.to(dev)
        for i in range(N):
            out[i] = nudger.apply(out[i], yo[i])
        return out.cpu()
    if out.shape[-1] != C:
        return out.cpu()
    yo = y_obs.to(dev).view(N, G, p, C)
    preds = torch.empty(N, G, p, C, dtype=torch.float32, device=dev)
    kinds = torch.zeros(C, dtype=torch.int32, device=dev)
    for step in range(p):
        if step > 0:
            state = hip.ar_advance(state.to(dev).contiguous(), preds[:, :, step - 1], None, kinds, None, 0, False)
            out = model(state.view(N, G, -1), attention_threshold=0.0)
            if out.dim() == 2:
                out = out.unsqueeze(0)
        if k is None or step < k:
            if out.shape == yo[:, :, step].shape:
                hip.nudge(out, yo[:, :, step], preds[:, :, step], *_nudge_coeffs(alpha), 0)
            else:
                preds[:, :, step].copy_(out)
        else:
            preds[:, :, step].copy_(out)
    return preds.view(N, G, p * C).cpu()


# ======================================================================================================================
# Optimal interpolation (src/assimilation/optimal_interpolation.py)
# ======================================================================================================================
def _haversine_m(c1: np.ndarray, c2: np.ndarray) -> np.ndarray:
    """Pairwise great-circle distances in metres (float64), optimal_interpolation.py:46-56."""
    lat1, lon1 = np.radians(c1[:, 0]), np.radians(c1[:, 1])
    lat2, lon2 = np.radians(c2[:, 0]), np.radians(c2[:, 1])
    dlat = lat1[:, None] - lat2[None, :]
    dlon = lon1[:, None] - lon2[None, :]
    a = np.sin(dlat / 2) ** 2 + np.cos(lat1[:, None]) * np.cos(lat2[None, :]) * np.sin(dlon / 2) ** 2
    return EARTH_RADIUS_M * 2 * np.arcsin(np.sqrt(a))


def nearest_oi_node(coords: np.ndarray) -> np.ndarray:
    """int64 [N]: for every OI node, the OI node an observation there maps to - `np.argmin` over float64 haversine
    distances, lowest index on ties.  Its own node is at distance 0 and distinct coordinates are at distance > 0, so
    this is the first node with identical coordinates: O(N) with a hash."""
    first = {}
    out = np.empty(len(coords), dtype=np.int64)
    for i, (la, lo) in enumerate(map(tuple, np.asarray(coords, dtype=np.float64))):
        out[i] = first.setdefault((la, lo), i)
    return out


class _Factor:
    """Cached factor of one station set: positions (OI node order), their nearest nodes, device arrays."""

    def __init__(self, oi, pos: np.ndarray):
        self.pos = pos
        self.m = len(pos)
        J = oi._canon[pos]
        dev = oi._dev
        self.obs_row = torch.from_numpy(oi._rows[pos].astype(np.int32)).to(dev)
        self.node_row = torch.from_numpy(oi._rows[J].astype(np.int32)).to(dev)
        lat = np.radians(oi._oi_coords[J, 0]).astype(np.float64)
        lon = np.radians(oi._oi_coords[J, 1]).astype(np.float64)
        self.stations = (torch.from_numpy(lat).to(dev), torch.from_numpy(lon).to(dev),
                         torch.from_numpy(np.cos(lat).astype(np.float32)).to(dev))
        self.M = hip.oi_factor(self.stations[0], self.stations[1], oi._sb2, oi._rl2, oi._diag)


class OptimalInterpolation:
    """Optimal interpolation with the reference's constructor and `apply` (optimal_interpolation.py), matrix-free.

    grid_lats / grid_lons: axes (nodes in `meshgrid(..., indexing='ij').ravel()` order, latitude-major) or, with
    `flat_grid=True`, per-node coordinates.  `roi_idx`: grid indices of the OI nodes; only their rows are corrected
    and only observations on them are used.  sigma_b / sigma_o: background / observation error; L: correlation length
    in metres.  The constructor builds no B (`.B` builds the reference's dense float32 B on first access)."""

    def __init__(self, grid_lats, grid_lons, sigma_b, sigma_o, L, device, flat_grid=False, roi_idx=None):
        self.sigma_b, self.sigma_o, self.L = sigma_b, sigma_o, L
        self.device = device
        self.roi_idx = roi_idx
        if flat_grid:
            self.grid_coords = np.vstack([grid_lats, grid_lons]).T
        else:
            lat_grid, lon_grid = np.meshgrid(grid_lats, grid_lons, indexing="ij")
            self.grid_coords = np.vstack([lat_grid.ravel(), lon_grid.ravel()]).T
        G = len(self.grid_coords)
        if roi_idx is not None:
            self._rows = np.asarray(roi_idx, dtype=np.int64).reshape(-1)
            self._oi_coords = self.grid_coords[self._rows]
        else:
            self._rows = np.arange(G, dtype=np.int64)
            self._oi_coords = self.grid_coords
        self._canon = nearest_oi_node(self._oi_coords)
        self._B = None
        self._dev = None
        self._nodes = None
        self._node_row = None
        self._cache = {}
        self.factorizations = 0  # number of station-covariance factorisations run so far
        self._sb2 = float(sigma_b) ** 2
        self._rl2 = (EARTH_RADIUS_M / float(L)) ** 2
        self._diag = float(sigma_o) ** 2 + 1e-5
        # weights below exp(-120) are 0 in float32: pairs beyond that angle skip the transcendentals
        th = math.sqrt(120.0 / self._rl2)
        self._th_cut = th if th < math.pi else 10.0
        self._a_cut = math.sin(0.5 * th) ** 2 if th < math.pi else 2.0

    # -- the reference's dense matrices, for callers that read them --------------------------------------------------
    def _dist_matrix(self, coords1, coords2):
        return _haversine_m(coords1, coords2)

    def _build_B(self):
        dists = self._dist_matrix(self._oi_coords, self._oi_coords)
        cov = (self.sigma_b ** 2) * np.exp(-(dists ** 2) / (self.L ** 2))
        return torch.from_numpy(cov).float()

    @property
    def B(self) -> torch.Tensor:
        """The reference's dense float32 background covariance over the OI nodes (built on first access)."""
        if self._B is None:
            self._B = self._build_B().to(self.device)
        return self._B

    # -- device state --------------------------------------------------------------------------------------------------
    def _setup(self):
        dev = torch.device(self.device)
        if dev.type != "cuda":
            dev = torch.device("cuda", torch.cuda.current_device())
        if self._dev == dev:
            return
        self._dev = dev
        lat = np.radians(self._oi_coords[:, 0]).astype(np.float64)
        lon = np.radians(self._oi_coords[:, 1]).astype(np.float64)
        self._nodes = (torch.from_numpy(lat).to(dev), torch.from_numpy(lon).to(dev),
                       torch.from_numpy(np.cos(lat).astype(np.float32)).to(dev))
        self._node_row = torch.from_numpy(self._rows.astype(np.int32)).to(dev) if self.roi_idx is not None else None
        self._cache = {}

    def _factor(self, pos: np.ndarray) -> _Factor:
        """The cached factor of the station set at OI positions `pos` (ascending)."""
        if len(pos) > hip.oi_max_stations():
            raise ValueError(f"optimal interpolation supports at most {hip.oi_max_stations()} stations per station "
                             f"set, got {len(pos)}")
        self._setup()
        key = pos.tobytes()
        fac = self._cache.get(key)
        if fac is None:
            fac = _Factor(self, pos)
            self._cache[key] = fac
            self.factorizations += 1
        return fac

    def _analyse(self, fac: _Factor, obs3, xb3, xa3, chans, rhs, tmp, W):
        hip.oi_innovation(obs3, xb3, fac.obs_row, fac.node_row, chans, rhs)
        hip.oi_solve(fac.M, rhs, tmp, W)
        hip.oi_analysis(xb3, xa3, chans, self._node_row, self._nodes, fac.stations, W, self._sb2, self._rl2,
                        self._th_cut, self._a_cut)

    @torch.no_grad()
    def apply(self, forecast, observations):
        """forecast, observations [..., C] (NaN: not observed) -> analysis of the same shape on the forecast's device.

        Channels are grouped by their station set (the observed OI nodes) and every group is solved against one cached
        factor.  The observation mask is copied to the host once per call to find the groups (the reference syncs
        several times per channel).  A channel without observations is returned unchanged."""
        input_shape = forecast.shape
        C = input_shape[-1]
        x_b = forecast.reshape(-1, C)
        G = x_b.shape[0]
        if G != len(self.grid_coords):
            raise RuntimeError(f"input size {G} does not match the OI grid size {len(self.grid_coords)}")
        self._setup()
        dev = self._dev
        xb = x_b.to(dev, torch.float32)
        yo = observations.reshape(-1, C).to(dev, torch.float32)
        y_oi = yo[self._node_row.long()] if self._node_row is not None else yo
        mask = (~torch.isnan(y_oi)).cpu().numpy()  # the one host sync
        xa = torch.empty_like(xb)
        hip.copy_rows(xb.unsqueeze(0), xa.unsqueeze(0))
        groups = {}
        for c in range(C):
            col = mask[:, c]
            if col.any():
                groups.setdefault(col.tobytes(), (col, []))[1].append(c)
        for col, chans in groups.values():
            fac = self._factor(np.nonzero(col)[0].astype(np.int64))
            n = len(chans)
            rhs = torch.empty(n, fac.m, dtype=torch.float64, device=dev)
            tmp = torch.empty_like(rhs)
            W = torch.empty(n, fac.m, dtype=torch.float32, device=dev)
            ch = torch.tensor(chans, dtype=torch.int32, device=dev)
            self._analyse(fac, yo.unsqueeze(0), xa.unsqueeze(0), xa.unsqueeze(0), ch, rhs, tmp, W)
        return xa.view(input_shape).to(forecast.device)

    def prepare_network(self, station_idx, channels=None) -> "OINetwork":
        """A fixed observation network (`predict.py --obs-sparsity / --obs-channels`): `station_idx` grid indices
        (inside the ROI when one is set), `channels` the observed channel indices (None: all)."""
        st = np.unique(np.asarray(station_idx, dtype=np.int64).reshape(-1))
        if self.roi_idx is not None:
            pos_of = {int(g): p for p, g in enumerate(self._rows)}
            missing = [int(g) for g in st if int(g) not in pos_of]
            if missing:
                raise ValueError(f"{len(missing)} station(s) outside the OI region, e.g. grid index {missing[0]}")
            pos = np.array(sorted(pos_of[int(g)] for g in st), dtype=np.int64)
        else:
            if len(st) and (st[0] < 0 or st[-1] >= len(self.grid_coords)):
                raise ValueError("station index outside the grid")
            pos = st
        if len(pos) == 0:
            raise ValueError("an observation network needs at least one station")
        return OINetwork(self, self._factor(pos), channels)


class OINetwork:
    """OI against one fixed station set and channel list.  `apply(forecast, observations)` takes [G, C] or
    [B, G, C] and equals `OptimalInterpolation.apply` bit for bit on observations that are finite exactly at the
    network's stations and channels.  No host sync; workspaces are allocated on the first call for a shape, later calls
    allocate only the returned tensor (none with `out=`), so a call can be captured in a hipGraph."""

    def __init__(self, oi: OptimalInterpolation, fac: _Factor, channels=None):
        self.oi, self.fac = oi, fac
        self.channels = None if channels is None else [int(c) for c in channels]
        self._ws = {}

    def _workspace(self, B: int, C: int):
        key = (B, C)
        ws = self._ws.get(key)
        if ws is None:
            chans = list(range(C)) if self.channels is None else self.channels
            if any(c < 0 or c >= C for c in chans):
                raise ValueError(f"observed channel outside [0, {C})")
            dev = self.oi._dev
            n = B * len(chans)
            ws = (torch.tensor(chans, dtype=torch.int32, device=dev),
                  torch.empty(n, self.fac.m, dtype=torch.float64, device=dev),
                  torch.empty(n, self.fac.m, dtype=torch.float64, device=dev),
                  torch.empty(n, self.fac.m, dtype=torch.float32, device=dev))
            self._ws[key] = ws
        return ws

    def prepare(self, C: int, B: int = 1) -> None:
        self._workspace(B, C)

    def apply_(self, f3: torch.Tensor, o3: torch.Tensor) -> torch.Tensor:
        """In place on a device [B, G, C] view (unit channel stride)."""
        if f3.shape[1] != len(self.oi.grid_coords):
            raise RuntimeError(f"input size {f3.shape[1]} does not match the OI grid size {len(self.oi.grid_coords)}")
        chans, rhs, tmp, W = self._workspace(f3.shape[0], f3.shape[2])
        if chans.numel():
            self.oi._analyse(self.fac, o3, f3, f3, chans, rhs, tmp, W)
        return f3

    @torch.no_grad()
    def apply(self, forecast: torch.Tensor, observations: torch.Tensor, out: Optional[torch.Tensor] = None):
        squeeze = forecast.dim() == 2
        f3 = forecast.unsqueeze(0) if squeeze else forecast
        o3 = observations.unsqueeze(0) if squeeze else observations
        if out is None:
            out = torch.empty_like(forecast)
        o_3 = out.unsqueeze(0) if squeeze else out
        if o_3.data_ptr() != f3.data_ptr():
            hip.copy_rows(f3.reshape(-1, f3.shape[1], f3.shape[2]), o_3)
        self.apply_(o_3, o3)
        return out


# ======================================================================================================================
# The DA grid search: one setting per batch row
# ======================================================================================================================
@dataclass(frozen=True)
class DASetting:
    """One run of the grid search: `predict.py --assim-method {method} --nudging-alpha {alpha} --oi-sigma-b {sigma_b}
    --oi-sigma-o {sigma_o} --oi-corr-len {corr_len} --obs-sparsity {sparsity}` (defaults as `predict.py:157-162`)."""
    method: str = "none"
    alpha: float = 0.25
    sigma_b: float = 0.8
    sigma_o: float = 0.5
    corr_len: float = 10000.0
    sparsity: Optional[float] = None
    label: str = ""

    def __post_init__(self):
        if self.method not in ("none", "nudging", "oi"):
            raise ValueError(f"Unknown assimilation method: {self.method}")
        if self.method != "none" and (self.sparsity is None or not self.sparsity > 0):
            raise ValueError(f"setting {self.label!r}: {self.method} needs a station density (sparsity > 0)")


def _density_tag(sparsity: float) -> str:
    return f"{sparsity * 100:g}"  # 0.1 -> "10", 0.01 -> "1": parse_da_results.py's oi10 / oi1 / nudg10 / nudg1


def da_grid(nudging_alphas: Sequence[float] = (0.01, 0.05, 0.1, 0.3),
            corr_lens: Sequence[float] = (5000.0, 10000.0, 50000.0), sigma_os: Sequence[float] = (0.3, 0.5),
            sparsities: Sequence[float] = (0.01, 0.1), sigma_b: float = 0.8, oi: Optional[Sequence[tuple]] = None,
            baseline: bool = False) -> list:
    """The settings of the shell drivers, in their order; the defaults are `da_grid_search.sh`'s 8 nudging + 12 OI
    runs: every (density, alpha), then every (density, corr_len, sigma_o).  `oi`: explicit (sparsity, corr_len, sigma_o)
    triples in place of the product (the `run_oi` lists of `da_experiments_v2.sh`, `_v3.sh`, `_merge.sh`); `baseline`
    puts the no-DA run first.  Labels are the names `parse_da_results.py` groups by: `baseline`,
    `nudg{density}_a{alpha}`, `oi{density}_c{corr_len in km}_s{sigma_o}` with the density in percent."""
    out = [DASetting(label="baseline")] if baseline else []
    for sp in sparsities:
        for a in nudging_alphas:
            out.append(DASetting("nudging", alpha=float(a), sparsity=float(sp), label=f"nudg{_density_tag(sp)}_a{a:g}"))
    triples = oi if oi is not None else [(sp, c, so) for sp in sparsities for c in corr_lens for so in sigma_os]
    for sp, c, so in triples:
        out.append(DASetting("oi", sigma_b=float(sigma_b), sigma_o=float(so), corr_len=float(c), sparsity=float(sp),
                             label=f"oi{_density_tag(sp)}_c{c / 1000.0:g}_s{so:g}"))
    return out


def station_network(pool, sparsity: float, seed: int = 42) -> np.ndarray:
    """The inline station draw of `scripts/predict.py:397-406`: max(1, int(len(pool) * sparsity)) grid indices drawn
    from `pool` without replacement by a fresh `RandomState(seed)`, ascending."""
    pool = np.asarray(pool)
    rng = np.random.RandomState(seed)
    n = max(1, int(len(pool) * sparsity))
    st = rng.choice(pool, n, replace=False)
    st.sort()
    return st


def sweep_row_order(settings: Sequence[DASetting]) -> list:
    """The batch rows of a sweep as indices into `settings`: the no-DA rows, the nudging rows, then the OI rows
    grouped by station density (in order of first appearance) and sorted by corr_len inside a group; ties keep the
    order of `settings`."""
    idx = range(len(settings))
    dens = []
    for s in settings:
        if s.method == "oi" and s.sparsity not in dens:
            dens.append(s.sparsity)
    order = [i for i in idx if settings[i].method == "none"] + [i for i in idx if settings[i].method == "nudging"]
    for d in dens:
        order += sorted((i for i in idx if settings[i].method == "oi" and settings[i].sparsity == d),
                        key=lambda i: settings[i].corr_len)
    return order


class DASweepAssimilator:
    """Assimilates batch row `row_of[label]` of a [S, G, C] step with setting `label`, all rows against one truth.

    oi_grid: (lats, lons) as `OptimalInterpolation` takes them (`flat_grid`, `roi_idx` likewise).  pool: the grid
    indices stations are drawn from; every distinct `sparsity` is one `station_network(pool, sparsity, seed)`, shared
    by the nudging and OI settings of that density.  channels: the observed channels (None: all).  Rows are ordered by
    `sweep_row_order`; `settings_by_row[r]` is the setting of row r.

    `apply_(step3, truth3)`: step3 [S, G, C] in place, truth3 [1, G, C] (or [S, G, C]) the unmasked truth - it is read
    at stations and observed channels only.  One `gcl_nudge_rows` covers the nudging rows; per OI density one
    innovation, one solve per setting (against the factor of its (sigma_b, sigma_o, corr_len), cached by the
    `OptimalInterpolation` of that triple) and one `gcl_oi_analysis_rows`.  Every row gets the bits of its own
    `NudgingAssimilator` / `OINetwork` at batch 1 on NaN-masked observations; `per_setting=True` runs exactly those
    instead (A/B and fallback).  No host sync after `prepare(C)` (implied by the first call), so calls can be
    captured."""

    broadcast_obs = True  # assimilated_rollout: observations of batch 1 serve every row

    def __init__(self, oi_grid, settings: Sequence[DASetting], pool, seed: int = 42, channels=None,
                 flat_grid: bool = False, roi_idx=None, device="cuda", per_setting: bool = False):
        self.settings = list(settings)
        labels = [s.label for s in self.settings]
        if not labels or len(set(labels)) != len(labels):
            raise ValueError("DASweepAssimilator: the settings need distinct labels (and at least one)")
        self.device = device
        self.channels = None if channels is None else [int(c) for c in channels]
        self.per_setting = bool(per_setting)
        self.order = sweep_row_order(self.settings)
        self.settings_by_row = [self.settings[i] for i in self.order]
        self.row_of = {s.label: r for r, s in enumerate(self.settings_by_row)}
        self.S = len(self.settings)
        self._oi_args = (oi_grid[0], oi_grid[1], bool(flat_grid), roi_idx)
        self.G = len(oi_grid[0]) if flat_grid else len(oi_grid[0]) * len(oi_grid[1])
        rows = self.settings_by_row
        # one station network per density, shared by nudging and OI
        self.densities = []
        for s in rows:
            if s.method != "none" and s.sparsity not in self.densities:
                self.densities.append(s.sparsity)
        self.networks = {d: station_network(pool, d, seed) for d in self.densities}
        for st in self.networks.values():
            if st.min() < 0 or st.max() >= self.G:
                raise ValueError("station index outside the grid")
        self._nud = [r for r, s in enumerate(rows) if s.method == "nudging"]  # contiguous by construction
        self._groups = []  # OI rows of one density: contiguous, corr_len ascending
        for d in self.densities:
            grp = [r for r, s in enumerate(rows) if s.method == "oi" and s.sparsity == d]
            if grp:
                self._groups.append({"r0": grp[0], "n": len(grp), "density": d})
        self.nudgers, self.oi_nets, self._oi, self._C = {}, {}, {}, None

    def prepare(self, C: int) -> None:
        """Factor the station covariances (one per distinct (network, sigma_b, sigma_o, corr_len), through one
        `OptimalInterpolation` per parameter triple), upload the tables and allocate the workspaces for C channels."""
        if self._C == C:
            return
        dev = torch.device(self.device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        rows = self.settings_by_row
        chans = list(range(C)) if self.channels is None else self.channels
        if any(c < 0 or c >= C for c in chans):
            raise ValueError(f"observed channel outside [0, {C})")
        self._chan_mask, chan_sel = None, None
        if self.channels is not None:
            chan_sel = torch.zeros(C, dtype=torch.bool)
            chan_sel[chans] = True
            self._chan_mask = chan_sel.to(dev, torch.uint8)
        mask = np.zeros((max(len(self.densities), 1), self.G), dtype=np.uint8)
        for n, d in enumerate(self.densities):
            mask[n, self.networks[d]] = 1
        self._station_mask = torch.from_numpy(mask).to(dev)
        if self._nud:
            self._nud_rows = (self._nud[0], self._nud[-1] + 1)
            self._nud_net = torch.tensor([self.densities.index(rows[r].sparsity) for r in self._nud],
                                         dtype=torch.int32).to(dev)
            self._nud_alpha = torch.from_numpy(np.array([_nudge_coeffs(rows[r].alpha)[1] for r in self._nud],
                                                        dtype=np.float32)).to(dev)
            self.nudgers = {r: NudgingAssimilator(alpha=rows[r].alpha, device=dev, feature_mask_flat=chan_sel)
                            for r in self._nud}
            for nud in self.nudgers.values():
                nud.prepare(C, dev)
        lats, lons, flat_grid, roi_idx = self._oi_args
        nch = len(chans)
        for g in self._groups:
            r0, n = g["r0"], g["n"]
            for r in range(r0, r0 + n):
                if r in self.oi_nets:
                    continue
                s = rows[r]
                key = (s.sigma_b, s.sigma_o, s.corr_len)
                if key not in self._oi:
                    self._oi[key] = OptimalInterpolation(lats, lons, s.sigma_b, s.sigma_o, s.corr_len, dev,
                                                         flat_grid=flat_grid, roi_idx=roi_idx)
                self.oi_nets[r] = self._oi[key].prepare_network(self.networks[g["density"]], self.channels)
            nets = [self.oi_nets[r] for r in range(r0, r0 + n)]
            fac = nets[0].fac  # the station set, hence obs_row / node_row / stations, is the group's
            widest = max(nets, key=lambda t: t.oi.L).oi
            g.update(nets=nets, fac=fac, nodes=widest._nodes, node_row=widest._node_row,
                     th_cut=widest._th_cut, a_cut=widest._a_cut,
                     chans=torch.tensor(chans, dtype=torch.int32).to(dev),
                     sb2=torch.from_numpy(np.array([t.oi._sb2 for t in nets], dtype=np.float32)).to(dev),
                     rl2=torch.from_numpy(np.array([t.oi._rl2 for t in nets], dtype=np.float32)).to(dev),
                     rhs=torch.empty(n * nch, fac.m, dtype=torch.float64, device=dev),
                     tmp=torch.empty(n * nch, fac.m, dtype=torch.float64, device=dev),
                     W=torch.empty(n * nch, fac.m, dtype=torch.float32, device=dev))
            for t in nets:
                t.prepare(C, 1)
        # per_setting: the NaN-masked observations each density's nudgers expect (OI reads stations only)
        self._masked = {}
        if self.per_setting and self._nud:
            self._masked = {d: torch.empty(1, self.G, C, dtype=torch.float32, device=dev) for d in self.densities}
            self._nan = torch.full((1, 1, 1), float("nan"), dtype=torch.float32, device=dev)
        self._C = C

    def _apply_per_setting(self, f3, o3):
        for n, d in enumerate(self.densities):
            if d in self._masked:
                assert o3.shape[0] == 1, "per_setting takes one truth for all rows"
                torch.where(self._station_mask[n].bool().view(1, -1, 1), o3, self._nan, out=self._masked[d])
        for r in self._nud:
            self.nudgers[r].apply_(f3[r:r + 1], self._masked[self.settings_by_row[r].sparsity])
        for r, net in self.oi_nets.items():
            net.apply_(f3[r:r + 1], o3 if o3.shape[0] == 1 else o3[r:r + 1])
        return f3

    def apply_(self, f3: torch.Tensor, o3: torch.Tensor) -> torch.Tensor:
        S, G, C = f3.shape
        if S != self.S or G != self.G:
            raise RuntimeError(f"a sweep of {self.S} settings on {self.G} nodes got a step of shape {tuple(f3.shape)}")
        if o3.shape[0] not in (1, S) or tuple(o3.shape[1:]) != (G, C):
            raise RuntimeError(f"observations {tuple(o3.shape)} do not match the step {tuple(f3.shape)}")
        self.prepare(C)
        if self.per_setting:
            return self._apply_per_setting(f3, o3)
        rows_of = (lambda a, b: o3) if o3.shape[0] == 1 else (lambda a, b: o3[a:b])  # noqa: E731
        if self._nud:
            a, b = self._nud_rows
            hip.nudge_rows(f3[a:b], rows_of(a, b), f3[a:b], self._station_mask, self._nud_net, self._nud_alpha,
                           self._chan_mask)
        for g in self._groups:
            if not g["chans"].numel():
                continue
            a, n = g["r0"], g["n"]
            nch = g["chans"].numel()
            fac, fg = g["fac"], f3[a:a + n]
            obs = rows_of(a, a + n)
            hip.oi_innovation(obs.expand(n, G, C) if obs.shape[0] != n else obs, fg, fac.obs_row, fac.node_row,
                              g["chans"], g["rhs"])
            for j, net in enumerate(g["nets"]):
                sl = slice(j * nch, (j + 1) * nch)
                hip.oi_solve(net.fac.M, g["rhs"][sl], g["tmp"][sl], g["W"][sl])
            hip.oi_analysis_rows(fg, fg, g["chans"], g["node_row"], g["nodes"], fac.stations, g["W"], g["sb2"],
                                 g["rl2"], g["th_cut"], g["a_cut"])
        return f3


# ======================================================================================================================
# Assimilated rollout
# ======================================================================================================================
@torch.no_grad()
def assimilated_rollout(model, X: torch.Tensor, ar_steps: int, obs: torch.Tensor, assimilator, k=None,
                        use_residual: bool = True, static_channels=None, forcing_channels=None, y=None,
                        attention_threshold: float = 0.0, kinds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`predict.rollout` with assimilation: each completed step (after the residual, the static carry-forward and the
    forcing) is assimilated against `obs[..., s*C:(s+1)*C]` while `k is None or s < k`, then stored and shifted into
    the window.  `assimilator`: a `NudgingAssimilator` or an `OINetwork`.  X [B, G, obs*C] (or [G, obs*C]), obs
    [B, G, ar_steps*C] on the GPU -> [B, G, ar_steps*C] on the GPU.  With a `DASweepAssimilator` B is its number of
    settings (X the same window in every row) and obs may be the truth once, [1, G, ar_steps*C].

    With use_residual=False and no static or forcing channels this is the reference's sequential-nudging loop
    (nudging.py:159-194) and OI loop (scripts/predict.py:499-510)."""
    squeeze = X.dim() == 2
    if squeeze:
        X, obs = X.unsqueeze(0), obs.unsqueeze(0)
        y = y.unsqueeze(0) if y is not None else None
    B, G, _ = X.shape
    nobs = model.obs_window
    C = X.shape[-1] // nobs
    one_obs = obs.shape[0] == 1 and getattr(assimilator, "broadcast_obs", False)  # one truth for all rows of a sweep
    if (obs.shape[0] != B and not one_obs) or obs.shape[1] != G or obs.shape[2] < ar_steps * C:
        raise ValueError(f"observations {tuple(obs.shape)} do not cover {ar_steps} steps of [{B}, {G}, {C}]")
    state = X.reshape(B, G, nobs, C).contiguous()
    if kinds is None:
        kinds = channel_kinds(C, static_channels, forcing_channels, X.device)
    out = torch.empty(B, G, ar_steps * C, dtype=torch.float32, device=X.device)
    y_steps = y.shape[-1] // C if y is not None else 0
    for s in range(ar_steps):
        delta = model(X=state.view(B, G, nobs * C), attention_threshold=attention_threshold)
        if delta.dim() == 2:
            delta = delta.unsqueeze(0)
        y_step = y[:, :, s * C:(s + 1) * C] if (y is not None and forcing_channels and s < y_steps) else None
        state = hip.ar_advance(state, delta, y_step, kinds, None, 0, use_residual)
        step = state[:, :, nobs - 1, :]
        if k is None or s < k:
            assimilator.apply_(step, obs[:, :, s * C:(s + 1) * C])
        hip.copy_rows(step, out[:, :, s * C:(s + 1) * C])
    return out[0] if squeeze else out


class CapturedAssimilatedRollout(CapturedRollout):
    """`assimilated_rollout` replayed from a hipGraph, as `predict.CapturedRollout` replays `rollout`."""

    def __init__(self, model, ar_steps: int, assimilator, k=None, static_channels=None, forcing_channels=None,
                 use_residual: bool = True):
        super().__init__(model, ar_steps, static_channels, forcing_channels, use_residual)
        self.assimilator, self.k = assimilator, k

    def _work(self, X, obs, y):
        return assimilated_rollout(self.model, X, self.ar_steps, obs, self.assimilator, k=self.k,
                                   use_residual=self.use_residual, static_channels=self.static_channels,
                                   forcing_channels=self.forcing_channels, y=y, kinds=self._channel_kinds(X))

    @torch.no_grad()
    def __call__(self, X: torch.Tensor, obs: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._forecast(X, obs, y)
