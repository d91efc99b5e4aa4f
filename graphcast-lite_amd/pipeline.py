"""The full-pipeline evaluation of `scripts/evaluate_full_pipeline.py` (with `--skip-unet`) on the HIP path:
multires rollout -> ROI rows in physical units -> lapse-rate correction -> learned MOS (stations only / with IDW) ->
OI against simulated station observations, every variant scored per horizon and channel on the regional grid and at the
stations, against persistence.

The expensive stages are the existing device code (`predict.rollout`, `mos.LearnedMOS`, `assimilation.OINetwork`); this
module adds the glue between them (csrc/pipeline.hip) so that a sample never returns to the host:

* `denormalize`, `apply_lapse`, `simulate_station_obs`: the script's helpers with their names and signatures, device
  tensors in and out.
* `evaluation_sample_starts`: the script's sample selection (`:371-387`).
* `FullPipelineEvaluator`: the sample loop of `:449-666` and the tables of `:678-766`.
* `MosIdwSweep`: the IDW parameter sweeps of `scripts/mos_idw_sweep.py` (multires frames, AR rollout) and
  `scripts/mos_idw_sweep_v2.py` (merged data set, +6 h), every setting scored by one kernel (`LearnedMOS.sweep`).
* `DaSweep`, `da_sweep_tables`: the DA grid search of `scripts/da_grid_search.sh` / `da_experiments_v*.sh` and the tables
  of `scripts/parse_da_results.py`: every nudging / OI setting is one batch row of one assimilated rollout.
"""
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .mos import IDW_SWEEP_CONFIGS, LearnedMOS
from .predict import rollout
from .verify import ForecastVerifier, Persistence

VARIANTS = ("GNN", "GNN+lapse", "GNN+MOS", "GNN+lapse+MOS", "GNN+lapse+MOS+IDW", "GNN+lapse+MOS+IDW+OI", "Persistence")


def _dev_f32(a, device) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device, torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def _need_gpu(t, who: str):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{who} needs a GPU tensor (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise ValueError(f"{who}: float32 expected, got {t.dtype}")


def denormalize(data_norm: torch.Tensor, mean, std) -> torch.Tensor:
    """`physical = normalized * std + mean` (`:147-149`) on the device, float32, the product and the sum rounded
    separately as numpy rounds them.  data_norm [..., C]; mean / std [C] (arrays or tensors)."""
    _need_gpu(data_norm, "denormalize")
    C = data_norm.shape[-1]
    x2 = data_norm.reshape(-1, C)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    raw = torch.empty(x2.shape[0], C, dtype=torch.float32, device=x2.device)
    hip.pipeline_roi_phys(x2, None, None, 0, x2.shape[0], _dev_f32(mean, x2.device), _dev_f32(std, x2.device), -1, -1,
                          0.0, False, raw)
    return raw.view(data_norm.shape)


def lapse_in_float64(target_elevation) -> bool:
    """Does numpy 2 evaluate `float32_array - target_elevation` in float64?  A Python scalar is weak (the array's
    float32 wins); a numpy scalar or 0-d array is strong and promotes by its own dtype."""
    if isinstance(target_elevation, (np.generic, np.ndarray)):
        return np.result_type(np.float32, np.asarray(target_elevation).dtype) == np.float64
    if isinstance(target_elevation, torch.Tensor):
        raise TypeError("target_elevation must be a host scalar")
    return False


def apply_lapse(pred_phys: torch.Tensor, var_order: Sequence[str], target_elevation) -> torch.Tensor:
    """Lapse-rate correction of t2m (`:184-200`): `t2m += (z_surf - target_elevation) * 6.5e-3` on pred_phys [G, C]
    or [G, steps, C] (z_surf of step 0 corrects every step).  Returns a new tensor, or pred_phys itself when `t2m` or
    `z_surf` is not in var_order.

    The arithmetic follows the TYPE of target_elevation as numpy 2 does: with a Python float (the script's
    `--lapse-elev 250`) every step is float32; with an `np.float64` (the script's default, `np.mean(...)`) or a 0-d
    float64 array the difference and the product are float64 and only the final add rounds to float32.  The two
    differ in the last bit of t2m in roughly one row in 170."""
    if "t2m" not in var_order or "z_surf" not in var_order:
        return pred_phys
    _need_gpu(pred_phys, "apply_lapse")
    if pred_phys.dim() not in (2, 3) or pred_phys.shape[-1] != len(var_order):
        raise ValueError(f"apply_lapse: [G, C] or [G, steps, C] with C = {len(var_order)} expected, got "
                         f"{tuple(pred_phys.shape)}")
    x3 = (pred_phys if pred_phys.dim() == 3 else pred_phys.unsqueeze(1)).contiguous()
    out = hip.pipeline_lapse(x3, list(var_order).index("t2m"), list(var_order).index("z_surf"), float(target_elevation),
                             lapse_in_float64(target_elevation))
    return out if pred_phys.dim() == 3 else out[:, 0, :]


def station_rows(r_lats, r_lons, stations: Sequence[dict], float32: bool = False) -> np.ndarray:
    """int64 [len(stations)]: the nearest node of the (lat, lon)-major regional grid for every station - the
    squared-degree argmin of the reference, duplicates kept.  float32=False: the float64 search of
    `simulate_station_obs` (`:213-219`); True: the search on float32 coordinates that picks the SCORING rows
    (`:402-410`).  The two can disagree for a station near a cell boundary; the script uses both, so both are kept."""
    lo_m, la_m = np.meshgrid(r_lons, r_lats)
    flat_lats, flat_lons = la_m.ravel(), lo_m.ravel()
    if float32:
        flat_lats, flat_lons = flat_lats.astype(np.float32), flat_lons.astype(np.float32)
    return np.array([int(np.argmin((flat_lats - st["lat"]) ** 2 + (flat_lons - st["lon"]) ** 2)) for st in stations],
                    dtype=np.int64)


def simulate_station_obs(ground_truth_phys: torch.Tensor, r_lats, r_lons, stations: Sequence[dict],
                         var_order: Sequence[str]) -> torch.Tensor:
    """Synthetic station observations for OI (`:203-222`): float32 [G, C], NaN everywhere except the rows of each
    station's nearest grid point, which hold the truth.  r_lats / r_lons are the regional AXES; G = len(r_lats) *
    len(r_lons).  (The reference sizes its field by len(r_lats) alone and fails with an IndexError for a station
    beyond the first len(r_lats) nodes; where it runs, its output is the head of this field.)"""
    _need_gpu(ground_truth_phys, "simulate_station_obs")
    G, C = len(r_lats) * len(r_lons), len(var_order)
    if tuple(ground_truth_phys.shape) != (G, C):
        raise ValueError(f"simulate_station_obs: truth must be [{G}, {C}], got {tuple(ground_truth_phys.shape)}")
    rows = torch.from_numpy(station_rows(r_lats, r_lons, stations).astype(np.int32)).to(ground_truth_phys.device)
    truth = ground_truth_phys if ground_truth_phys.stride(1) == 1 else ground_truth_phys.contiguous()
    return hip.pipeline_station_obs(truth, rows)


def evaluation_sample_starts(T_overlap: int, obs: int, ar: int, max_samples: int) -> list:
    """The script's test samples (`:371-387`): the last 20 % of the overlap, its second half (the first is the
    validation part), every start whose obs + ar frames fit, thinned evenly to at most max_samples."""
    n_test_total = int(T_overlap * 0.2)
    test_start = T_overlap - n_test_total + n_test_total // 2
    valid = list(range(test_start, T_overlap - (obs + ar) + 1))
    n = min(max_samples, len(valid))
    if n < len(valid):
        step = len(valid) // n
        return [valid[i * step] for i in range(n)]
    return valid[:n]


class FullPipelineEvaluator:
    """The evaluation loop of `scripts/evaluate_full_pipeline.py:392-766` without the U-Net cascade.

    model: the one-step forecaster on the multires node set (`model(X=..., attention_threshold=...)`, `.obs_window`).
    dataset: a `MultiresChunkDataset(quantize=False)` - the script normalises the float32 frames (`:452-468`).
    regional_series: fp16 device tensor (T, lon, lat, C), the truth and the persistence baseline in physical units
    (None: the dataset's own regional series, merge mode).  var_order: the C channel names.  y_mean / y_std: the
    scalers.  stations: {"lat", "lon", "elev"} dicts.  lapse_elev: the target elevation; its TYPE selects the
    arithmetic, see `apply_lapse`.  mos: a `mos.MOSForest`, the bundle of `mos.load_learned_mos` or its model (None:
    no MOS variants).  oi: an `assimilation.OptimalInterpolation` on the regional axes (None: no OI variant; the OI
    variant also needs mos, its input is the IDW variant).  idw_power / idw_radius_km: the script's 2.0 / 300.0.
    base_time: forecast start; step h is valid at base_time + 6 h * (h + 1) (`:413`, `:490-493`).

    `update(sample_starts)` runs every sample on the device and adds its squared errors into device accumulators; it
    makes no host synchronisation of its own.  `results()` copies them to the host once."""

    def __init__(self, model, dataset, regional_series, var_order: Sequence[str], y_mean, y_std,
                 stations: Sequence[dict], ar_steps: int, lapse_elev, mos=None, oi=None, use_residual: bool = False,
                 idw_power: float = 2.0, idw_radius_km: float = 300.0, base_time=None, static_names=("z_surf", "lsm")):
        from datetime import datetime, timedelta, timezone

        self.model, self.ds, self.var_order = model, dataset, list(var_order)
        self.device = dataset.device
        self.obs, self.ar, self.use_residual = int(model.obs_window), int(ar_steps), bool(use_residual)
        self.C = len(self.var_order)
        if dataset.n_feat != self.C:
            raise ValueError(f"the dataset serves {dataset.n_feat} features, var_order names {self.C}")
        self.rs = regional_series if regional_series is not None else dataset.region_series
        if self.rs is None:
            raise ValueError("regional_series is needed (the dataset holds none in interpolate mode)")
        if not (self.rs.is_cuda and self.rs.dtype == torch.float16 and self.rs.dim() == 4 and self.rs.is_contiguous()):
            raise ValueError("regional_series must be a contiguous fp16 device tensor (T, lon, lat, C)")
        r_lats, r_lons = dataset.r_lats, dataset.r_lons
        if tuple(self.rs.shape[1:3]) != (len(r_lons), len(r_lats)) or self.rs.shape[3] < self.C:
            raise ValueError(f"regional_series {tuple(self.rs.shape)} does not match the dataset's regional axes")
        self.G, self.n_kept = dataset.n_regional, dataset.n_global_kept
        self.mean, self.std = _dev_f32(y_mean, self.device), _dev_f32(y_std, self.device)
        self._zeros = torch.zeros(self.C, dtype=torch.float32, device=self.device)
        self._ones = torch.ones(self.C, dtype=torch.float32, device=self.device)
        self.stations = list(stations)
        self.lapse_elev, self.lapse_f64 = float(lapse_elev), lapse_in_float64(lapse_elev)
        has_lapse = "t2m" in self.var_order and "z_surf" in self.var_order
        self.t_idx = self.var_order.index("t2m") if has_lapse else -1
        self.z_idx = self.var_order.index("z_surf") if has_lapse else -1
        self.static_channels = {self.var_order.index(n) for n in static_names if n in self.var_order}

        self.score_rows = station_rows(r_lats, r_lons, self.stations, float32=True)
        self._score = torch.from_numpy(self.score_rows.astype(np.int32)).to(self.device)
        self.variants = ["GNN", "GNN+lapse"]
        self._mos_stn = self._mos_idw = self._oi_net = None
        if mos is not None and "t2m" in self.var_order:
            lo_m, la_m = np.meshgrid(r_lons, r_lats)
            lat32, lon32 = la_m.ravel().astype(np.float32), lo_m.ravel().astype(np.float32)  # :402-404
            self._mos_stn = LearnedMOS(mos, self.var_order, lat32, lon32, self.stations, False, device=self.device)
            self._mos_idw = LearnedMOS(mos, self.var_order, lat32, lon32, self.stations, True, idw_power,
                                       idw_radius_km, device=self.device)
            base = base_time if base_time is not None else datetime(2020, 6, 1, 0, 0, 0, tzinfo=timezone.utc)
            # one valid time per step (:550), uploaded once
            self._tfeat = [self._mos_stn.time_features([base + timedelta(hours=6 * (h + 1))]) for h in range(self.ar)]
            self.variants += ["GNN+MOS", "GNN+lapse+MOS", "GNN+lapse+MOS+IDW"]
            if oi is not None:
                self.sim_rows = station_rows(r_lats, r_lons, self.stations)
                self._sim = torch.from_numpy(self.sim_rows.astype(np.int32)).to(self.device)
                self._oi_net = oi.prepare_network(self.sim_rows)
                self._oi_net.prepare(self.C)
                self._obs = torch.empty(self.G, self.C, dtype=torch.float32, device=self.device)
                self.variants.append("GNN+lapse+MOS+IDW+OI")
        self.variants.append("Persistence")
        V = len(self.variants)
        self._buf = torch.empty(V - 1, self.G, self.C, dtype=torch.float32, device=self.device)
        self._acc_grid = torch.zeros(V, self.ar, self.C, dtype=torch.float64, device=self.device)
        self._acc_stn = torch.zeros(V, self.ar, self.C, dtype=torch.float64, device=self.device)
        self.count_grid, self.count_stn = [0] * self.ar, [0] * self.ar

    def reset(self):
        self._acc_grid.zero_()
        self._acc_stn.zero_()
        self.count_grid, self.count_stn = [0] * self.ar, [0] * self.ar

    def _step(self, pred2: torch.Tensor, truth2: torch.Tensor, h: int):
        """Every model variant of one step from the normalised output rows pred2 [N, C] into self._buf."""
        buf = self._buf
        hip.pipeline_roi_phys(pred2, None, None, self.n_kept, self.G, self.mean, self.std, self.t_idx, self.z_idx,
                              self.lapse_elev, self.lapse_f64, buf[0], buf[1])
        if self._mos_stn is not None:
            tf = self._tfeat[h]
            as3 = lambda t: t.view(self.G, 1, self.C)  # noqa: E731  ((G, 1, C): one step per call, :536-539)
            self._mos_stn.apply(as3(buf[0]), tf, out=as3(buf[2]))
            self._mos_stn.apply(as3(buf[1]), tf, out=as3(buf[3]))
            self._mos_idw.apply(as3(buf[1]), tf, out=as3(buf[4]))
            if self._oi_net is not None:
                hip.pipeline_station_obs(truth2, self._sim, out=self._obs)
                self._oi_net.apply(buf[4], self._obs, out=buf[5])

    @torch.no_grad()
    def update(self, sample_starts: Sequence[int], keep: bool = False):
        """Run the samples starting at the frames `sample_starts` (`:449-666`).  keep=True also returns, per sample and
        step, a copy of the variant stack [V, G, C] (the order of `self.variants`) and of the truth [G, C]."""
        starts = [int(t) for t in sample_starts]
        T = min(self.ds.total_time, self.rs.shape[0])
        if any(t < 0 or t + self.obs + self.ar > T for t in starts):
            raise ValueError(f"a sample needs {self.obs + self.ar} frames inside the {T} common ones")
        t0_all = torch.tensor(starts, dtype=torch.int64).to(self.device)
        C, ar, V = self.C, self.ar, len(self.variants)
        kept = []
        for i in range(len(starts)):
            t0 = t0_all[i:i + 1]
            X, _ = self.ds.windows(t0, self.obs, 0, C)
            out = rollout(self.model, X, ar, use_residual=self.use_residual)  # [1, N, ar * C], the script's gnn_out
            # the last observed regional frame and the ar truths, physical units, (lat, lon)-major: (x - 0) / 1 is exact
            phys, _ = hip.window_pack(self.rs, t0 + (self.obs - 1), self._zeros, self._ones, C, 1 + ar, 0)
            persist = phys[:, :, :C]
            for h in range(ar):
                truth = phys[0, :, (1 + h) * C:(2 + h) * C]
                self._step(out[0, :, h * C:(h + 1) * C], truth, h)
                hip.pipeline_sqerr(self._buf, truth, self._score, h, self._acc_grid[:V - 1], self._acc_stn[:V - 1])
                hip.pipeline_sqerr(persist, truth, self._score, h, self._acc_grid[V - 1:], self._acc_stn[V - 1:])
                self.count_grid[h] += self.G
                self.count_stn[h] += len(self.score_rows)
                if keep:
                    kept.append((i, h, torch.cat([self._buf, persist]), truth.clone()))
        return kept if keep else None

    def results(self) -> dict:
        """The accumulated sums and the script's tables (`:678-766`, `:811-827`), host values:
        mse_grid / mse_stn [variant][h] -> float64 [C] sums of squared errors, count_grid / count_stn [h],
        rmse_grid / rmse_stn [variant] -> [ar, C], t2m_rmse_grid / t2m_rmse_stn [variant] -> the ar horizons and their
        mean, skill [variant] -> percent against persistence averaged over the non-static channels, the ar horizons and
        their mean."""
        grid, stn = self._acc_grid.cpu().numpy(), self._acc_stn.cpu().numpy()
        ng = np.maximum(np.array(self.count_grid, dtype=np.float64), 1)[:, None]
        ns = np.maximum(np.array(self.count_stn, dtype=np.float64), 1)[:, None]
        res = {"variants": list(self.variants), "count_grid": list(self.count_grid), "count_stn": list(self.count_stn),
               "mse_grid": {}, "mse_stn": {}, "rmse_grid": {}, "rmse_stn": {}, "t2m_rmse_grid": {}, "t2m_rmse_stn": {},
               "skill": {}}
        for v, name in enumerate(self.variants):
            res["mse_grid"][name], res["mse_stn"][name] = list(grid[v]), list(stn[v])
            res["rmse_grid"][name], res["rmse_stn"][name] = np.sqrt(grid[v] / ng), np.sqrt(stn[v] / ns)
            if "t2m" in self.var_order:
                t = self.var_order.index("t2m")
                for key in ("rmse_grid", "rmse_stn"):
                    vals = [float(x) for x in res[key][name][:, t]]
                    res["t2m_" + key][name] = vals + [float(np.mean(vals))]
        dyn = [c for c in range(self.C) if c not in self.static_channels]
        rp = res["rmse_grid"]["Persistence"]
        for name in self.variants[:-1]:
            rm = res["rmse_grid"][name]
            vals = [float(np.mean([(1.0 - rm[h, c] / rp[h, c]) * 100 if rp[h, c] > 1e-8 else 0 for c in dyn]))
                    for h in range(self.ar)]
            res["skill"][name] = vals + [float(np.mean(vals))]
        return res


SWEEP_BASE_VARIANTS = ("Persistence", "GNN_raw", "GNN+lapse", "GNN+lapse+MOS_station")


def sweep_variant_names(configs=IDW_SWEEP_CONFIGS) -> list:
    """The rows of the sweep scripts' tables (`all_cfgs`, mos_idw_sweep.py:303-304): persistence, the three variants
    without IDW, then one per setting."""
    return list(SWEEP_BASE_VARIANTS) + [f"GNN+lapse+MOS+IDW_{c[2]}" for c in configs]


def sweep_tables(se: dict, count: Sequence[int], configs=IDW_SWEEP_CONFIGS) -> dict:
    """The tables the sweep scripts print (mos_idw_sweep.py:293-357, mos_idw_sweep_v2.py:319-375) from the t2m
    squared-error sums `se[variant][h]` and the counts `count[h]`: rmse [variant] -> the horizons and their mean,
    skill [variant] -> percent against persistence, the horizons and their mean, best [h] -> (label, rmse) of the IDW
    setting with the smallest RMSE (the first one on a tie)."""
    names = sweep_variant_names(configs)
    H = len(count)
    rmse = {n: [float(np.sqrt(se[n][h] / max(count[h], 1))) for h in range(H)] for n in names}
    res = {"variants": names, "count": list(count), "se_t2m": {n: [float(v) for v in se[n]] for n in names},
           "rmse": {n: v + [float(np.mean(v))] for n, v in rmse.items()}, "skill": {}, "best": []}
    pr = rmse["Persistence"]
    for n in names[1:]:
        vals = [float((1.0 - rmse[n][h] / pr[h]) * 100) if pr[h] > 1e-8 else 0.0 for h in range(H)]
        res["skill"][n] = vals + [float(np.mean(vals))]
    for h in range(H):
        best, best_rmse = None, 9999.0
        for c in configs:
            r = rmse[f"GNN+lapse+MOS+IDW_{c[2]}"][h]
            if r < best_rmse:
                best, best_rmse = c[2], r
        res["best"].append((best, best_rmse))
    return res


class MosIdwSweep:
    """The MOS/IDW parameter sweep of the reference's two scripts on the device: per sample and horizon the t2m squared
    error on the regional rows of persistence, the raw forecast, the lapse-corrected one, the station-only MOS and
    every IDW setting of `configs` ((power, radius_km, label), default `mos.IDW_SWEEP_CONFIGS`).  The station forest
    runs once for all settings and one kernel scores them (`LearnedMOS.sweep`); no corrected field is stored.

    mode="multires" (`scripts/mos_idw_sweep.py:196-282`): dataset is a `MultiresChunkDataset(quantize=False)`,
    regional_series the fp16 device series (T, lon, lat, C) that gives truth and persistence in physical units (None:
    the dataset's own, merge mode); an AR rollout of `ar_steps`; the lapse is `apply_lapse` (the TYPE of lapse_elev
    selects its arithmetic); the MOS coordinates are the (lat, lon)-major regional grid in float32.

    mode="merged" (`scripts/mos_idw_sweep_v2.py:229-304`): dataset is any `batch(indices) -> (X, Y)` data set of the
    merged node set (z-scored `[B, N, obs * C]`, `[B, N, >= C]`), region_rows the indices of the regional rows (default:
    `dataset.is_regional`), coordinates the per-node (lats, lons) (default: `dataset.coordinates`), used in float32.
    Truth and persistence are Y and the last X frame de-normalised, one horizon; the lapse is v2's formula
    `t2m + 6.5e-3 * (z_surf / 9.80665 - lapse_elev)` in float32 with the forecast's own z_surf.

    `update(samples)` (frame starts in multires mode, data-set indices in merged mode) makes no host synchronisation;
    `results()` copies the sums to the host once and returns `sweep_tables` of them."""

    def __init__(self, model, dataset, var_order: Sequence[str], y_mean, y_std, stations: Sequence[dict], lapse_elev,
                 mos, mode: str = "multires", regional_series=None, ar_steps: int = 1, region_rows=None,
                 coordinates=None, configs=IDW_SWEEP_CONFIGS, use_residual: bool = False, base_time=None):
        from datetime import datetime, timedelta, timezone

        if mode not in ("multires", "merged"):
            raise ValueError(f"Unknown mode: {mode}")
        self.mode, self.model, self.ds, self.var_order = mode, model, dataset, list(var_order)
        if "t2m" not in self.var_order:
            raise ValueError("MosIdwSweep scores t2m: it is not in var_order")
        self.configs = [(float(c[0]), float(c[1]), str(c[2])) for c in configs]
        if not self.configs or len({c[2] for c in self.configs}) != len(self.configs):
            raise ValueError("MosIdwSweep: the settings need distinct labels (and at least one)")
        self.device = torch.device(dataset.device)
        self.obs, self.use_residual = int(model.obs_window), bool(use_residual)
        self.C = len(self.var_order)
        self.ar = int(ar_steps) if mode == "multires" else 1
        if mode == "merged" and int(ar_steps) != 1:
            raise ValueError("merged mode scores one horizon (+6 h): the data set holds no later truth")
        self.t_idx = self.var_order.index("t2m")
        self.z_idx = self.var_order.index("z_surf") if "z_surf" in self.var_order else -1
        self.lapse_elev = float(lapse_elev)
        self.mean, self.std = _dev_f32(y_mean, self.device), _dev_f32(y_std, self.device)
        if self.mean.numel() != self.C or self.std.numel() != self.C:
            raise ValueError(f"y_mean / y_std must hold {self.C} values")
        self.stations = list(stations)
        if mode == "multires":
            if dataset.n_feat != self.C:
                raise ValueError(f"the dataset serves {dataset.n_feat} features, var_order names {self.C}")
            self.rs = regional_series if regional_series is not None else dataset.region_series
            if self.rs is None:
                raise ValueError("regional_series is needed (the dataset holds none in interpolate mode)")
            if not (self.rs.is_cuda and self.rs.dtype == torch.float16 and self.rs.dim() == 4 and self.rs.is_contiguous()):
                raise ValueError("regional_series must be a contiguous fp16 device tensor (T, lon, lat, C)")
            r_lats, r_lons = dataset.r_lats, dataset.r_lons
            if tuple(self.rs.shape[1:3]) != (len(r_lons), len(r_lats)) or self.rs.shape[3] < self.C:
                raise ValueError(f"regional_series {tuple(self.rs.shape)} does not match the dataset's regional axes")
            self.G, self.n_kept, self._rows = dataset.n_regional, dataset.n_global_kept, None
            self.lapse_f64 = lapse_in_float64(lapse_elev)
            lo_m, la_m = np.meshgrid(r_lons, r_lats)
            lat32, lon32 = la_m.ravel().astype(np.float32), lo_m.ravel().astype(np.float32)  # mos_idw_sweep.py:111-113
            self._zeros = torch.zeros(self.C, dtype=torch.float32, device=self.device)
            self._ones = torch.ones(self.C, dtype=torch.float32, device=self.device)
        else:
            lats, lons = coordinates if coordinates is not None else dataset.coordinates
            rows = np.asarray(region_rows if region_rows is not None else np.where(np.asarray(dataset.is_regional))[0])
            if rows.ndim != 1 or rows.size == 0 or rows.min() < 0 or rows.max() >= len(lats):
                raise ValueError("region_rows must be a non-empty list of node indices")
            lat32 = np.asarray(lats).astype(np.float32)[rows]  # mos_idw_sweep_v2.py:119-120, :217-218
            lon32 = np.asarray(lons).astype(np.float32)[rows]
            self.G, self.n_kept = int(rows.size), 0
            self._rows = torch.from_numpy(rows.astype(np.int32)).to(self.device)
            self.lapse_f64 = False
        forest = mos
        self._mos_stn = LearnedMOS(forest, self.var_order, lat32, lon32, self.stations, False, device=self.device)
        self._mos_idw = LearnedMOS(forest, self.var_order, lat32, lon32, self.stations, True, device=self.device)
        base = base_time if base_time is not None else datetime(2020, 6, 1, 0, 0, 0, tzinfo=timezone.utc)
        self._tfeat = [self._mos_stn.time_features([base + timedelta(hours=6 * (h + 1))]) for h in range(self.ar)]
        self.variants = sweep_variant_names(self.configs)
        G, C = self.G, self.C
        self._buf = torch.empty(3, G, C, dtype=torch.float32, device=self.device)  # raw, lapse, station MOS
        self._truth = torch.empty(2, G, C, dtype=torch.float32, device=self.device)  # merged mode: persistence, truth
        self._acc = torch.zeros(4, self.ar, C, dtype=torch.float64, device=self.device)  # raw, lapse, MOS, persistence
        self._acc_idw = torch.zeros(len(self.configs), self.ar, dtype=torch.float64, device=self.device)
        self.count = [0] * self.ar

    def reset(self):
        self._acc.zero_()
        self._acc_idw.zero_()
        self.count = [0] * self.ar

    def _score(self, truth2: torch.Tensor, persist2: torch.Tensor, h: int):
        """Station MOS, the error sums of the four plain variants and the sweep, from self._buf[0:2]."""
        buf, G, C = self._buf, self.G, self.C
        tf = self._tfeat[h]
        as3 = lambda t: t.view(G, 1, C)  # noqa: E731  ((G, 1, C): one step per call)
        self._mos_stn.apply(as3(buf[1]), tf, out=as3(buf[2]))
        hip.pipeline_sqerr(buf, truth2, None, h, self._acc[:3])
        hip.pipeline_sqerr(persist2.unsqueeze(0), truth2, None, h, self._acc[3:])
        self._mos_idw.sweep(as3(buf[1]), tf, truth2[:, self.t_idx:self.t_idx + 1], self.configs, self._acc_idw, h)
        self.count[h] += G

    @torch.no_grad()
    def update(self, samples: Sequence[int]):
        """Add the samples: frame starts (multires; a sample needs obs + ar_steps frames) or data-set indices (merged)."""
        C, ar, buf = self.C, self.ar, self._buf
        ids = [int(t) for t in samples]
        if self.mode == "merged":
            if any(i < 0 or i >= len(self.ds) for i in ids):
                raise ValueError(f"a sample index outside the {len(self.ds)} samples of the data set")
            for i in ids:
                X, Y = self.ds.batch([i])
                out = rollout(self.model, X, 1, use_residual=self.use_residual)  # [1, N, C]
                hip.pipeline_roi_phys(out[0, :, :C], None, self._rows, 0, self.G, self.mean, self.std, -1, -1, 0.0,
                                      False, buf[0])
                if self.z_idx >= 0:
                    hip.pipeline_lapse_geopotential(buf[0].view(self.G, 1, C), self.t_idx, self.z_idx, self.lapse_elev,
                                                    out=buf[1].view(self.G, 1, C))
                else:
                    buf[1].copy_(buf[0])
                hip.pipeline_roi_phys(X[0, :, (self.obs - 1) * C:self.obs * C], None, self._rows, 0, self.G, self.mean,
                                      self.std, -1, -1, 0.0, False, self._truth[0])
                hip.pipeline_roi_phys(Y[0, :, :C], None, self._rows, 0, self.G, self.mean, self.std, -1, -1, 0.0, False,
                                      self._truth[1])
                self._score(self._truth[1], self._truth[0], 0)
            return
        T = min(self.ds.total_time, self.rs.shape[0])
        if any(t < 0 or t + self.obs + ar > T for t in ids):
            raise ValueError(f"a sample needs {self.obs + ar} frames inside the {T} common ones")
        t0_all = torch.tensor(ids, dtype=torch.int64).to(self.device)
        z = self.z_idx
        for i in range(len(ids)):
            t0 = t0_all[i:i + 1]
            X, _ = self.ds.windows(t0, self.obs, 0, C)
            out = rollout(self.model, X, ar, use_residual=self.use_residual)
            phys, _ = hip.window_pack(self.rs, t0 + (self.obs - 1), self._zeros, self._ones, C, 1 + ar, 0)
            persist = phys[0, :, :C]
            for h in range(ar):
                truth = phys[0, :, (1 + h) * C:(2 + h) * C]
                hip.pipeline_roi_phys(out[0, :, h * C:(h + 1) * C], None, None, self.n_kept, self.G, self.mean, self.std,
                                      self.t_idx if z >= 0 else -1, z, self.lapse_elev, self.lapse_f64, buf[0], buf[1])
                self._score(truth, persist, h)

    def results(self) -> dict:
        """`sweep_tables` of the accumulated sums (host values): variants, count [h], se_t2m / rmse / skill [variant]
        and best [h] -> (label, rmse)."""
        plain, idw = self._acc.cpu().numpy()[:, :, self.t_idx], self._acc_idw.cpu().numpy()
        se = {"GNN_raw": plain[0], "GNN+lapse": plain[1], "GNN+lapse+MOS_station": plain[2], "Persistence": plain[3]}
        for p, c in enumerate(self.configs):
            se[f"GNN+lapse+MOS+IDW_{c[2]}"] = idw[p]
        return sweep_tables(se, self.count, self.configs)


# ======================================================================================================================
# The DA grid search (scripts/da_grid_search.sh, da_experiments_v2.sh / _v3.sh / _merge.sh, parse_da_results.py)
# ======================================================================================================================
def _scores(pred, base) -> dict:
    """The figures `predict.py` prints for one pair of StreamingMetrics (`:636`, `:651-652`, `:723-740`)."""
    sp, sb = pred._split(), base._split()
    rmse = float(np.sqrt(sp["sum_se"] / max(sp["total_elem"], 1)))
    base_rmse = float(np.sqrt(sb["sum_se"] / max(sb["total_elem"], 1)))
    dyn = [c for c in range(pred.C) if c not in pred.exclude_channels]

    def acc(s):
        apc = s["sum_acc"] / np.maximum(s["acc_count"], 1)
        return float(apc[dyn].mean()) if dyn else 0.0

    return {"rmse": rmse, "base_rmse": base_rmse, "skill": float((1.0 - rmse / (base_rmse + 1e-12)) * 100),
            "acc": acc(sp), "base_acc": acc(sb),
            "rmse_per_channel": [float(v) for v in np.sqrt(sp["sum_se_per_ch"] / np.maximum(sp["elem_per_ch"], 1))]}


def da_sweep_tables(verifiers: Sequence[ForecastVerifier], settings) -> dict:
    """The tables of the grid search from one `ForecastVerifier` (methods "pred", "base") per setting, in the order of
    `settings` (host only).

    per_setting[label]: the setting's fields, `global` (overall scores; `global["skill"]` is `predict.py`'s "Skill"),
    `global_horizon` [h], and with a region `region`, `region_horizon` [h] - each a dict of rmse, base_rmse, skill
    (percent against persistence), acc, base_acc and rmse_per_channel - plus `skill_6h`: the skill of the first
    horizon on the region (the whole grid without one; the overall figure when there is a single horizon), the
    figure `parse_da_results.py` tabulates.
    oi_tables[density]: its corr_len x sigma_o table of skill_6h (`make_oi_table`): corr_lens_km and sigma_os
    ascending, `skill[i][j]` or None where that pair was not run (the last one run wins when a pair repeats).
    best[(method, density)]: the label with the largest skill_6h, the first on a tie.  Densities are percent strings
    ("10", "1") as in the labels."""
    from .assimilation import _density_tag

    settings = list(settings)
    if len(verifiers) != len(settings):
        raise ValueError(f"{len(verifiers)} verifiers for {len(settings)} settings")
    res = {"settings": [s.label for s in settings], "per_setting": {}, "oi_tables": {}, "best": {}}
    for s, v in zip(settings, verifiers):
        row = {"method": s.method, "sparsity": s.sparsity, "alpha": s.alpha, "sigma_b": s.sigma_b,
               "sigma_o": s.sigma_o, "corr_len": s.corr_len,
               "global": _scores(v.overall["pred"], v.overall["base"]),
               "global_horizon": [_scores(p, b) for p, b in zip(v.horizon["pred"], v.horizon["base"])]}
        scope, scope_h = row["global"], row["global_horizon"]
        if v.region["pred"] is not None:
            row["region"] = scope = _scores(v.region["pred"], v.region["base"])
            row["region_horizon"] = scope_h = [_scores(p, b) for p, b in
                                               zip(v.region_horizon["pred"], v.region_horizon["base"])]
        row["skill_6h"] = (scope_h[0] if scope_h else scope)["skill"]
        res["per_setting"][s.label] = row
    for s in settings:
        if s.method == "none":
            continue
        d, skill = _density_tag(s.sparsity), res["per_setting"][s.label]["skill_6h"]
        best = res["best"].get((s.method, d))
        if best is None or skill > res["per_setting"][best]["skill_6h"]:
            res["best"][(s.method, d)] = s.label
    for d in dict.fromkeys(_density_tag(s.sparsity) for s in settings if s.method == "oi"):
        mine = [s for s in settings if s.method == "oi" and _density_tag(s.sparsity) == d]
        corr = sorted({s.corr_len / 1000.0 for s in mine})
        sig = sorted({s.sigma_o for s in mine})
        table = [[None] * len(sig) for _ in corr]
        for s in mine:
            table[corr.index(s.corr_len / 1000.0)][sig.index(s.sigma_o)] = res["per_setting"][s.label]["skill_6h"]
        res["oi_tables"][d] = {"corr_lens_km": corr, "sigma_os": sig, "skill": table}
    return res


class DaSweep:
    """The DA grid search on the device: per sample ONE assimilated rollout whose batch rows are the settings (the
    input window replicated, the truth passed once as the observations), every row scored by its own
    `verify.ForecastVerifier` against the truth and persistence - the reference starts `scripts/predict.py` once per
    setting and rolls the same samples through the same network each time.

    dataset: any `batch(indices) -> (X [B, G, obs*C], Y [B, G, >= ar_steps*C])` data set on the GPU.  settings:
    `assimilation.DASetting`s (`assimilation.da_grid`).  pool: the grid indices stations are drawn from
    (`--obs-roi-only`: region_idxs); region_idxs: the scored region and, as in `predict.py:382-386`, the OI nodes.
    exclude_channels: left out of the aggregate metrics (static + forcing); obs_channels: the observed channel
    indices (None: all); k: assimilate the first k steps only.  coordinates: the (lats, lons) of the grid in the
    `OptimalInterpolation` convention (default `dataset.coordinates`), flat_grid: per-node coordinates (default
    `dataset.flat_grid`, else False).  capture: replay the rollout from a hipGraph.

    `update(sample_indices)` makes no host synchronisation; `results()` copies the sums to the host and returns
    `da_sweep_tables`."""

    def __init__(self, model, dataset, settings, ar_steps: int, pool, region_idxs=None, exclude_channels=None,
                 obs_channels=None, k=None, use_residual: bool = False, static_channels=None, forcing_channels=None,
                 seed: int = 42, capture: bool = True, coordinates=None, flat_grid=None):
        from .assimilation import CapturedAssimilatedRollout, DASweepAssimilator

        self.model, self.ds, self.settings, self.ar = model, dataset, list(settings), int(ar_steps)
        self.device = torch.device(dataset.device)
        self.obs = int(model.obs_window)
        self.k, self.use_residual = k, bool(use_residual)
        self.static_channels, self.forcing_channels = static_channels, forcing_channels
        coords = coordinates if coordinates is not None else dataset.coordinates
        flat = bool(getattr(dataset, "flat_grid", False)) if flat_grid is None else bool(flat_grid)
        self.region_idxs = None if region_idxs is None else np.asarray(region_idxs, dtype=np.int64)
        self.assimilator = DASweepAssimilator(coords, self.settings, pool, seed, channels=obs_channels, flat_grid=flat,
                                              roi_idx=self.region_idxs, device=self.device)
        self.S = len(self.settings)
        self._rows = [self.assimilator.row_of[s.label] for s in self.settings]
        self._rollout = CapturedAssimilatedRollout(model, self.ar, self.assimilator, k=k,
                                                   static_channels=static_channels,
                                                   forcing_channels=forcing_channels, use_residual=self.use_residual)
        self._rollout.use_graph = bool(capture)
        self._exclude = exclude_channels
        self.verifiers, self._persist, self.n = None, None, 0

    @property
    def graph_active(self) -> bool:
        return self._rollout.graph_active

    def reset(self):
        self.n = 0
        for v in self.verifiers or []:
            v.reset()

    @torch.no_grad()
    def update(self, sample_indices: Sequence[int]):
        """Add the samples (data-set indices), one rollout of all settings each."""
        ids = [int(i) for i in sample_indices]
        if any(i < 0 or i >= len(self.ds) for i in ids):
            raise ValueError(f"a sample index outside the {len(self.ds)} samples of the data set")
        for i in ids:
            X, Y = self.ds.batch([i])
            C = X.shape[-1] // self.obs
            if Y.shape[-1] < self.ar * C:
                raise ValueError(f"the data set holds {Y.shape[-1] // C} target steps, the sweep assimilates {self.ar}")
            if self.verifiers is None:
                self.verifiers = [ForecastVerifier(C, self.ar, exclude_channels=self._exclude,
                                                   region_idxs=self.region_idxs, device=self.device)
                                  for _ in self.settings]
                self._persist = Persistence(X[0], C)
            truth = Y[:, :, :self.ar * C]
            XS = X.expand(self.S, -1, -1)
            yS = Y.expand(self.S, -1, -1) if self.forcing_channels else None
            out = self._rollout(XS, truth, yS)
            self._persist.X = X[0]
            for v, r in zip(self.verifiers, self._rows):
                v.update(truth[0], pred=out[r], base=self._persist)
            self.n += 1

    def results(self) -> dict:
        if self.verifiers is None:
            raise RuntimeError("DaSweep.results() before any update()")
        res = da_sweep_tables(self.verifiers, self.settings)
        res["n"] = self.n
        return res
