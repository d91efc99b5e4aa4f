"""Autoregressive rollout / inference caller of the hot path.

Mirrors the AR branch of the reference's inference script (`scripts/predict.py:499-538`; the same
steps appear in the training loop, `src/train.py:203-228`): the one-step model predicts a delta,
the residual is added, static channels are carried forward from the last input step, forcing
channels are taken from the known future (`y`), the step is stored and the observation window is
shifted.  Here the whole per-step glue is one kernel (`gcl_ar_advance`) and the window never
leaves the device.

The script's entry point is here too: `python -m graphcast_lite_amd.predict <experiment_dir> [options]` (`main`,
`build_parser`) with the options of `scripts/predict.py:126-177` and `--batch-size`; `predict_experiment` is its loop
(`:448-614`) for any model with `.obs_window` and any data set with `batch(indices)`, `inference_tables` its summary
(`:634-803`), `PredictRun` what the loop returns.  `assimilation`, `verify`, `main` and `data` are imported inside
those functions (`assimilation` imports this module).
"""
from typing import Optional, Sequence

import torch

from . import hip
from .capture import Captured


def channel_kinds(C: int, static_channels: Optional[Sequence[int]], forcing_channels: Optional[Sequence[int]], device):
    """int32 [C]: 0 predicted, 1 static (carry forward), 2 forcing (from y).  Forcing wins over
    static when a channel is listed twice, as the reference applies the forcing overwrite last."""
    kind = torch.zeros(C, dtype=torch.int32)
    for ch in static_channels or []:
        kind[ch] = 1
    for ch in forcing_channels or []:
        kind[ch] = 2
    return kind.to(device)


@torch.no_grad()
def rollout(model, X: torch.Tensor, ar_steps: int, y: Optional[torch.Tensor] = None, static_channels=None,
            forcing_channels=None, use_residual: bool = True, attention_threshold: float = 0.0,
            kinds: Optional[torch.Tensor] = None) -> torch.Tensor:
    """X [B,G,obs*C] (or [G,obs*C]) on the GPU -> predictions [B,G,ar_steps*C].

    `y` [B,G,P*C] supplies the forcing channels for the steps it covers (`ar_step < P`), exactly as
    `scripts/predict.py:527-529` does; later steps keep the model's own value."""
    squeeze = X.dim() == 2
    if squeeze:
        X = X.unsqueeze(0)
        y = y.unsqueeze(0) if y is not None else None
    B, G, _ = X.shape
    obs = model.obs_window
    C = X.shape[-1] // obs
    state = X.reshape(B, G, obs, C).contiguous()
    if kinds is None:  # (a caller that captures the rollout uploads this once, outside the capture)
        kinds = channel_kinds(C, static_channels, forcing_channels, X.device)
    out = torch.empty(B, G, ar_steps * C, dtype=torch.float32, device=X.device)
    y_steps = y.shape[-1] // C if y is not None else 0
    for s in range(ar_steps):
        delta = model(X=state.view(B, G, obs * C), attention_threshold=attention_threshold)
        if delta.dim() == 2:
            delta = delta.unsqueeze(0)
        y_step = y[:, :, s * C:(s + 1) * C] if (y is not None and forcing_channels and s < y_steps) else None
        state = hip.ar_advance(state, delta, y_step, kinds, out, s * C, use_residual)
    return out[0] if squeeze else out


class CapturedRollout(Captured):
    """`rollout` replayed from a hipGraph: the whole K-step autoregressive forecast (K model forwards
    + K window advances, a few hundred launches at batch 1) costs the host one graph launch.

    The first two calls for a given input signature run eagerly (graph handles, workspaces and
    allocator pools get set up), the third captures, later calls copy the inputs into the captured
    buffers and replay.  Falls back to eager launches if capture is not possible (see `.launch_mode`)."""

    def __init__(self, model, ar_steps: int, static_channels=None, forcing_channels=None, use_residual: bool = True):
        self.model, self.ar_steps = model, ar_steps
        self.static_channels, self.forcing_channels, self.use_residual = static_channels, forcing_channels, use_residual
        self._kinds = None
        super().__init__(recapture=True)

    enabled = property(lambda self: self.use_graph)  # False after a failed capture

    def _channel_kinds(self, X):
        """`channel_kinds`, uploaded once (outside the capture) and kept while X's channel count and device stay."""
        C = X.shape[-1] // self.model.obs_window
        if self._kinds is None or self._kinds.numel() != C or self._kinds.device != X.device:
            self._kinds = channel_kinds(C, self.static_channels, self.forcing_channels, X.device)
        return self._kinds

    def _work(self, X, y):
        return rollout(self.model, X, self.ar_steps, y=y, static_channels=self.static_channels,
                       forcing_channels=self.forcing_channels, use_residual=self.use_residual,
                       kinds=self._channel_kinds(X))

    def _forecast(self, *args):
        if getattr(self.model, "using_sparse_gat", False):
            return self._work(*args)
        out = self._run(*args)
        return out.clone() if out is self._result else out  # the next replay overwrites the graph's output

    @torch.no_grad()
    def __call__(self, X: torch.Tensor, y: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._forecast(X, y)


PREDICTION_KEYS = ("predictions", "ground_truth", "n_features", "ar_steps", "obs_window", "n_lon", "n_lat",
                   "sample_offsets", "data_dir")


def save_predictions(path, preds: torch.Tensor, truth: torch.Tensor, n_features: int, ar_steps: int, obs_window: int,
                     n_lon: int, n_lat: int, sample_offsets=None, data_dir="") -> dict:
    """Write the `predictions.pt` bundle of scripts/predict.py:617-631: normalised forecasts and truth [N, G, C * P] as
    host tensors plus the integers and strings the comparison scripts read back.  sample_offsets: the temporal offset
    of every sample (default 0 .. N-1).  Returns the dictionary written."""
    if preds.dim() != 3 or preds.shape != truth.shape:
        raise ValueError(f"save_predictions: predictions {tuple(preds.shape)} and truth {tuple(truth.shape)}, expected "
                         "two [N, G, C * P]")
    if preds.shape[2] != int(n_features) * int(ar_steps):
        raise ValueError(f"save_predictions: {preds.shape[2]} columns are not {n_features} features x {ar_steps} steps")
    offsets = list(range(preds.shape[0])) if sample_offsets is None else [int(o) for o in sample_offsets]
    if len(offsets) != preds.shape[0]:
        raise ValueError(f"save_predictions: {len(offsets)} offsets for {preds.shape[0]} samples")
    bundle = {"predictions": preds.detach().cpu(), "ground_truth": truth.detach().cpu(), "n_features": int(n_features),
              "ar_steps": int(ar_steps), "obs_window": int(obs_window), "n_lon": int(n_lon), "n_lat": int(n_lat),
              "sample_offsets": offsets, "data_dir": str(data_dir)}
    torch.save(bundle, str(path))
    return bundle


def load_predictions(path):
    """What `save_predictions` (or the reference's predict.py) wrote, on the host: the dictionary, or the bare tensor
    of the legacy form."""
    return torch.load(str(path), map_location="cpu", weights_only=True)


# ======================================================================================================================
# The inference entry point (scripts/predict.py:125-803)
# ======================================================================================================================
def build_parser():
    """The options of scripts/predict.py:126-177 with the reference's names, types, defaults, nargs and choices, plus
    `--batch-size`."""
    import argparse

    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.predict")
    ap.add_argument("experiment_dir", help="e.g. experiments/demo")
    ap.add_argument("--data-dir", default=None)
    ap.add_argument("--ckpt", default=None, help="path of the .pth (default: <experiment_dir>/best_model.pth)")
    ap.add_argument("--save", default=None)
    ap.add_argument("--no-save", action="store_true")
    ap.add_argument("--max-samples", type=int, default=None, help="test samples to run (default: 200 for chunked data)")
    ap.add_argument("--region", nargs=4, type=float, metavar=("LAT_MIN", "LAT_MAX", "LON_MIN", "LON_MAX"))
    ap.add_argument("--prune-mesh", action="store_true",
                    help="prune the mesh to the bounding box of the data plus a buffer (regional data sets)")
    ap.add_argument("--mesh-buffer", type=float, default=15.0, help="buffer in degrees around the data with --prune-mesh")
    ap.add_argument("--per-channel", action="store_true")
    ap.add_argument("--ar-steps", type=int, default=None,
                    help="autoregressive steps: a one-step model is fed its own output, e.g. 4 for +24h")
    ap.add_argument("--no-residual", action="store_true",
                    help="the model predicts the full field, not the increment: do not add the last input step")
    ap.add_argument("--split", default="test_only", choices=["test_only", "val", "test", "train", "all"],
                    help="which split of a chunked data set to run")
    ap.add_argument("--assim-method", default="none", choices=["none", "nudging", "oi"])
    ap.add_argument("--obs-path", type=str, default=None)
    ap.add_argument("--nudging-alpha", type=float, default=0.25)
    ap.add_argument("--nudging-mode", default="sequential", choices=["sequential", "offline"])
    ap.add_argument("--nudge-first-k", type=int, default=None)
    ap.add_argument("--oi-sigma-b", type=float, default=0.8)
    ap.add_argument("--oi-sigma-o", type=float, default=0.5)
    ap.add_argument("--oi-corr-len", type=float, default=10000.0)
    ap.add_argument("--boundary-blending", action="store_true")
    ap.add_argument("--background-path", type=str, default=None)
    ap.add_argument("--taper-width", type=int, default=5)
    ap.add_argument("--obs-sparsity", type=float, default=None,
                    help="share of the nodes that are stations (0.01 = 1%%): sparse observations are cut from the truth "
                         "in the loop, no observation file needed")
    ap.add_argument("--obs-seed", type=int, default=42, help="seed of the station draw with --obs-sparsity")
    ap.add_argument("--obs-roi-only", action="store_true", help="stations inside the scored region only")
    ap.add_argument("--obs-channels", type=str, default=None,
                    help="comma-separated names of the observed variables (default: all)")
    ap.add_argument("--batch-size", type=int, default=8, help="samples per rollout call")
    return ap


def resolve_data_dir(data_dir, exp_cfg, repo_root=None):
    """scripts/predict.py:192-212: `--data-dir`, else the configuration's `data_dir`, else the first that exists of
    data/datasets/<name without _v2> and data/datasets/<name>, each relative to the working directory and then to
    `repo_root` (default: the directory above the package); none exists: the first candidate."""
    from pathlib import Path

    if data_dir:
        return Path(data_dir)
    if getattr(exp_cfg, "data_dir", None):
        return Path(exp_cfg.data_dir)
    import os

    root = Path(repo_root) if repo_root is not None else Path(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    name = str(getattr(exp_cfg.data.dataset_name, "value", exp_cfg.data.dataset_name))
    physical = name.replace("_v2", "")
    candidates = [Path("data") / "datasets" / physical, root / "data" / "datasets" / physical,
                  Path("data") / "datasets" / name, root / "data" / "datasets" / name]
    for c in candidates:
        if c.exists():
            return c
    return candidates[0]


def is_chunked_dir(data_dir) -> bool:
    import os

    return os.path.exists(os.path.join(str(data_dir), "data.npy")) or os.path.exists(
        os.path.join(str(data_dir), "dataset_info.json"))


def scored_rows(region, boundary_mask_width: int, meta, data_dir, G: int, say=print):
    """scripts/predict.py:335-375: (int64 grid rows the regional scores run over or None, their label for the table).
    In order of precedence: the inner zone of `boundary_mask_width` (regular grids without `--region`); `--region` on
    coords.npz (axes through `region_node_indices`, per-node coordinates through the box test); `meta.is_regional`;
    `--region` on the linspace axes."""
    import os

    import numpy as np

    from .verify import linspace_lats_lons, region_node_indices

    rows = None
    flat = getattr(meta, "flat_grid", False)
    bmw = int(boundary_mask_width or 0)
    coords_npz = os.path.join(str(data_dir), "coords.npz")
    if bmw > 0 and not region and not flat:
        n_lon, n_lat = meta.num_longitudes, meta.num_latitudes
        j = np.arange(bmw, n_lon - bmw, dtype=np.int64)
        i = np.arange(bmw, n_lat - bmw, dtype=np.int64)
        rows = (j[:, None] * n_lat + i[None, :]).reshape(-1)
        say(f"[boundary-mask] boundary_mask_width={bmw}: inner {n_lon - 2 * bmw}×{n_lat - 2 * bmw} = {len(rows)}/{G} "
            f"points (regional scores on the inner zone only)")
    if region and os.path.exists(coords_npz):
        z = np.load(coords_npz)
        c_lats, c_lons = z["latitude"].astype(np.float32), z["longitude"].astype(np.float32)
        lat_min, lat_max, lon_min, lon_max = region
        if c_lats.ndim == 1 and len(c_lats) != G:
            rows = region_node_indices(lat_min, lat_max, lon_min, lon_max, c_lats, c_lons)
        else:
            rows = np.where((c_lats >= lat_min) & (c_lats <= lat_max) & (c_lons >= lon_min) & (c_lons <= lon_max))[0]
        say(f"[Region] {len(rows)} nodes (--region [{lat_min},{lat_max}]N x [{lon_min},{lon_max}]E)")
    elif getattr(meta, "is_regional", None) is not None and rows is None:
        rows = np.where(meta.is_regional)[0]
        say(f"[Region] {len(rows)} nodes (from is_regional mask)")
    elif region and rows is None:
        rows = region_node_indices(*region, *linspace_lats_lons(meta.num_latitudes, meta.num_longitudes))
        say(f"[Region] {len(rows)} nodes")
    if rows is None:
        return None, None
    if region:
        label = f"[{region[0]},{region[1]}]N x [{region[2]},{region[3]}]E"
    elif bmw > 0:
        label = f"inner zone (boundary_mask_width={bmw})"
    else:
        label = "is_regional mask"
    return np.asarray(rows, dtype=np.int64), label


def station_pool(obs_roi_only: bool, region_rows, meta, G: int):
    """scripts/predict.py:398-403: the nodes the inline station draw picks from."""
    import numpy as np

    if obs_roi_only and region_rows is not None:
        return region_rows
    if getattr(meta, "is_regional", None) is not None:
        return np.where(meta.is_regional)[0]
    return np.arange(G)


def observed_channels(obs_channels: str, variables, C: int, say=print):
    """scripts/predict.py:411-421: the indices of the comma-separated names in `variables`; unknown names are
    reported and left out."""
    requested = [v.strip() for v in obs_channels.split(",")]
    idx = []
    for v in requested:
        if v in variables:
            idx.append(list(variables).index(v))
        else:
            say(f"[WARN] variable '{v}' not found in {list(variables)}")
    say(f"[Obs-channels] observing {len(idx)}/{C} channels: {requested}")
    return idx


class _PerSampleOI:
    """`OptimalInterpolation.apply` sample by sample, for observation files whose NaN pattern changes from sample to
    sample (one host read per call, as `apply` documents; not capturable)."""

    def __init__(self, oi):
        self.oi = oi

    def apply_(self, f3, o3):
        for b in range(f3.shape[0]):
            f3[b].copy_(self.oi.apply(f3[b], o3[b]))
        return f3


class PredictRun:
    """What `predict_experiment` returns: the `ForecastVerifier` (device state) and host snapshots of its objects as
    (prediction, persistence) `regional_train.RegionScores` pairs - `overall`, `horizons` (one pair per horizon when
    there is more than one), `region` and `region_horizons` (None / [] without scored rows) - plus what the tables
    print around them and, when the forecasts were kept, `predictions` / `ground_truth` [N, G, K] on the host with
    their `sample_offsets`."""

    def __init__(self, verifier, grid, G: int, C: int, ar_steps: int, region_label=None, n_region: int = 0):
        self.verifier, self.grid, self.G, self.C, self.ar_steps = verifier, tuple(grid), int(G), int(C), int(ar_steps)
        self.region_label, self.n_region = region_label, int(n_region)
        self.overall = self.region = None
        self.horizons, self.region_horizons = [], []
        self.predictions = self.ground_truth = self.sample_offsets = None
        self.n_samples = 0

    def snapshot(self):
        """One copy of the verifier's whole state to the host; every pair is read from it."""
        from .regional_train import RegionScores
        from .verify import StreamingMetrics

        ver = self.verifier
        host = ver._states.detach().cpu() if ver._states is not None else None

        def of(obj):
            sm = StreamingMetrics(ver.C, exclude_channels=ver.exclude_channels)
            if host is not None:
                sm._state = host[[o for _, _, _, o in ver._objects].index(obj)]
            return RegionScores.of(sm)

        pair = lambda a, b: (of(a), of(b))  # noqa: E731
        self.overall = pair(ver.overall["pred"], ver.overall["base"])
        self.horizons = [pair(a, b) for a, b in zip(ver.horizon["pred"], ver.horizon["base"])]
        if ver.region["pred"] is not None:
            self.region = pair(ver.region["pred"], ver.region["base"])
            self.region_horizons = [pair(a, b) for a, b in zip(ver.region_horizon["pred"], ver.region_horizon["base"])]
        self.n_samples = self.overall[0].n
        return self


@torch.no_grad()
def predict_experiment(model, dataset, num_channels: int, ar_steps: int, pred_window: int = 1, max_samples=None,
                       batch_size: int = 8, use_residual: bool = True, static_channels=None, forcing_channels=None,
                       region_rows=None, region_label=None, grid=(0, 0), assim_method: str = "none",
                       nudging_mode: str = "sequential", nudging_alpha: float = 0.25, nudge_first_k=None, oi=None,
                       observations=None, station_rows=None, obs_channels=None, boundary_mask=None, background=None,
                       keep: bool = False, use_graph=None, device=None, say=print) -> PredictRun:
    """The inference loop of scripts/predict.py:448-614 over the first `max_samples` samples of `dataset` (anything with
    `batch(indices)` -> (X [B, G, obs*C], y [B, G, steps*C]) on the device), `batch_size` samples per call, for any
    `model` with `.obs_window`.  `pred_window`: the steps the model returns per call (P_model).

    Forecast branches, each as the reference has it: sequential nudging and OI run the bare model loop
    (`assimilated_rollout(use_residual=False)` without channel kinds; a model that returns all `ar_steps` steps at once
    has each step of that one output assimilated); `ar_steps == pred_window == 1` gives `x_last + pred` (or `pred`
    without `use_residual`) with no static carry-forward; `ar_steps <= pred_window` the model's output as it is;
    otherwise `rollout` with the residual, static and forcing channels.  Then offline nudging, then the boundary blend
    (`boundary_mask` float32 [G] on the device, `background` [N, G, K] on the host, indexed by the sample's position).

    Observations: cut from the truth at `station_rows` / `obs_channels` on the device (`sparse_observations`), else
    `observations` [N, G, K] (host, NaN = not observed, indexed by position), else the truth.  `oi`: the
    `OptimalInterpolation` of `assim_method == "oi"`; with `station_rows` it works on that fixed network, against the
    whole truth on every node of its region, against an observation file sample by sample.

    Rollouts go through `CapturedRollout` / `CapturedAssimilatedRollout` (`use_graph` as elsewhere).  Scores: one
    `ForecastVerifier` updated per batch, which adds a batch's samples in order, so every state (and the kept forecasts)
    is bit-equal for any batch size as long as the model's rows are.  No host read inside the loop apart from the
    progress line every 50 samples.  `keep`: collect forecasts and truth in one device buffer, copied once at the end."""
    from .assimilation import CapturedAssimilatedRollout, NudgingAssimilator, _nudge_coeffs
    from .capture import graph_enabled
    from .observations import sparse_observations
    from .verify import ForecastVerifier, Persistence, taper_blend

    C, P, Pm = int(num_channels), int(ar_steps), int(pred_window)
    n_total = len(dataset)
    n_run = n_total if max_samples is None else min(int(max_samples), n_total)
    if batch_size < 1:
        raise ValueError(f"predict_experiment: batch_size={batch_size}")
    static_channels, forcing_channels = list(static_channels or []), list(forcing_channels or [])
    ver = ForecastVerifier(C, P, exclude_channels=sorted(set(static_channels) | set(forcing_channels)),
                           region_idxs=region_rows, device=device)
    run = PredictRun(ver, grid, 0, C, P, region_label, 0 if region_rows is None else len(region_rows))
    graph = graph_enabled(use_graph)
    sequential = assim_method == "nudging" and nudging_mode == "sequential"
    roll = assimilator = None
    offsets, kept = [], None
    done = 0
    model.eval()
    for i0 in range(0, n_run, batch_size):
        idx = list(range(i0, min(i0 + batch_size, n_run)))
        X, y = dataset.batch(idx)
        B, G = X.shape[0], X.shape[1]
        X, y = X.reshape(B, G, -1), y.reshape(B, G, -1)
        dev, K = X.device, y.shape[-1]
        run.G = G
        # --- observations
        obs = y
        if assim_method != "none":
            if station_rows is not None:
                obs = sparse_observations(y, station_rows, channels=obs_channels, num_channels=C)
            elif observations is not None:
                obs = observations[idx[0]:idx[-1] + 1].to(dev, torch.float32).reshape(B, G, -1)
        # --- forecast
        if sequential or assim_method == "oi":
            if assimilator is None:
                if sequential:
                    assimilator = NudgingAssimilator(alpha=nudging_alpha, device=dev)
                elif station_rows is not None:
                    assimilator = oi.prepare_network(station_rows, obs_channels)
                elif observations is None:
                    assimilator = oi.prepare_network(oi._rows)  # the whole truth: every node of the OI region observes
                else:
                    assimilator = _PerSampleOI(oi)
            whole = Pm * C == (K if sequential else P * C)  # the model returns the whole horizon at once
            if whole or (sequential and Pm != 1):
                out = model(X=X, attention_threshold=0.0)
                out = (out.unsqueeze(0) if out.dim() == 2 else out).contiguous()
                if whole and sequential:
                    if out.shape == obs.shape:
                        hip.nudge(out, obs, out, *_nudge_coeffs(nudging_alpha), 0, None)
                elif whole:
                    if obs.shape[-1] < P * C:
                        raise ValueError(f"observations of {obs.shape[-1]} columns do not cover {P} steps of {C} channels")
                    for t in range(P):
                        assimilator.apply_(out[:, :, t * C:(t + 1) * C], obs[:, :, t * C:(t + 1) * C])
            else:
                if Pm != 1:
                    raise ValueError(f"OI needs a model of 1 or {P} steps per call, got {Pm}")
                if roll is None:
                    roll = CapturedAssimilatedRollout(model, P, assimilator, k=nudge_first_k if sequential else None,
                                                      use_residual=False)
                    roll.use_graph = graph and not isinstance(assimilator, _PerSampleOI)
                out = roll(X, obs, None)
        else:
            if P == Pm == 1:
                if roll is None:
                    roll = CapturedRollout(model, 1, use_residual=use_residual)
                    roll.use_graph = graph
                out = roll(X, None)
            elif P <= Pm:
                out = model(X=X, attention_threshold=0.0)
                out = out.unsqueeze(0) if out.dim() == 2 else out
            else:
                if Pm != 1:
                    raise ValueError(f"the autoregressive rollout needs a one-step model, got {Pm} steps per call")
                if roll is None:
                    roll = CapturedRollout(model, P, static_channels=static_channels, forcing_channels=forcing_channels,
                                           use_residual=use_residual)
                    roll.use_graph = graph
                out = roll(X, y if forcing_channels else None)
            if assim_method == "nudging" and nudging_mode == "offline":
                out = out.contiguous()
                hip.nudge(out, obs, out, *_nudge_coeffs(nudging_alpha), 1, None)
        if boundary_mask is not None:
            bg = background[idx[0]:idx[-1] + 1].to(dev, torch.float32).reshape(B, G, -1)
            out = taper_blend(boundary_mask, out, bg)
        # --- scores
        ver.update(y, pred=out, base=Persistence(X, C))
        if keep:
            if kept is None:
                kept = torch.empty(2, n_run, G, K, dtype=torch.float32, device=dev)
            kept[0, idx[0]:idx[-1] + 1].copy_(out[:, :, :K])
            kept[1, idx[0]:idx[-1] + 1].copy_(y)
            pairs = getattr(dataset, "_sample_indices", None)
            offsets += [int(pairs[i][1]) if pairs is not None and i < len(pairs) else i for i in idx]
        if (idx[-1] + 1) // 50 > done // 50:
            sp = ver.overall["pred"]
            say(f"  [{idx[-1] + 1}/{n_run}] RMSE={sp.rmse:.6f} ACC={sp.acc:.4f}")
        done = idx[-1] + 1
    if kept is not None:
        host = kept.cpu()
        run.predictions, run.ground_truth, run.sample_offsets = host[0], host[1], offsets
    return run.snapshot()


def _horizon_header(n: int) -> str:
    return "".join(f" {'+' + str((p + 1) * 6) + 'h':>8s}" for p in range(n))


def _physical(name: str, value: float) -> str:
    """One cell of the key-variable tables: geopotential in metres, temperatures in degrees, the rest as it is."""
    if "z@" in name or name == "z_surf":
        return f" {value / 9.81:8.1f}m"
    if name == "t2m" or name.startswith("t@"):
        return f" {value:7.2f}°C"
    return f" {value:8.2f}"


def inference_tables(results: PredictRun, per_channel: bool = False, variables=None, std=None, say=print):
    """scripts/predict.py:634-803, from the `=====` line before `=== Inference summary` to the end: overall, per horizon,
    with `per_channel` the key-variable table and the overall per-channel table (physical units when `std`, the data
    set's per-channel standard deviations, is given; `variables` None: ch0, ch1, ...), and the region block with its
    per-horizon and per-channel tables."""
    import numpy as np

    from .regional_train import KEY_VARS, UNITS

    sp, sb = results.overall
    C, AR = results.C, results.ar_steps
    skill = 1.0 - (sp.rmse / (sb.rmse + 1e-12))
    say("")
    say("=" * 60)
    say(f"=== Inference summary ({sp.n} samples) ===")
    say(f"Grid: {results.grid[0]}x{results.grid[1]} (G={results.G}) | C={C} | AR={AR} horizons")
    say(f"Overall: MSE={sp.mse:.6f} | RMSE={sp.rmse:.6f} | MAE={sp.mae:.6f}")
    say(f"Baseline: RMSE={sb.rmse:.6f} | MAE={sb.mae:.6f}")
    say(f"Skill: {skill * 100:.2f}%")
    say(f"ACC: {sp.acc:.4f} | base: {sb.acc:.4f} | Δ={sp.acc - sb.acc:+.4f}")

    def horizon_lines(pairs, indent):
        for p, (a, b) in enumerate(pairs):
            sk = 1.0 - (a.rmse / (b.rmse + 1e-12))
            say(f"{indent}+{(p + 1) * 6:02d}h: RMSE={a.rmse:.6f} | base={b.rmse:.6f} | skill={sk * 100:.2f}% | "
                f"ACC={a.acc:.4f} (base {b.acc:.4f})")

    def channel_tables(overall, pairs, indent, key_title, overall_title):
        var_order = list(variables) if variables is not None else [f"ch{c}" for c in range(C)]
        sd = None if std is None else np.asarray(std, dtype=np.float64)[:C]
        if AR > 1 and pairs and sd is not None:
            key_idx = [i for i, v in enumerate(var_order[:C]) if v in KEY_VARS]
            say(key_title)
            say(f"{indent}{'var':>10s} {'unit':>6s}" + _horizon_header(len(pairs)))
            for c in key_idx:
                name = var_order[c]
                row = f"{indent}{name:>10s} {UNITS.get(name, '?'):>6s}"
                for a, _ in pairs:
                    row += _physical(name, a.rmse_per_channel[c] * sd[c])
                say(row)
        rmse_pc, acc_pc = overall.rmse_per_channel, overall.acc_per_channel
        if sd is not None:
            say(overall_title)
            say(f"{indent}{'#':>3s} {'var':>10s} {'ACC':>8s} {'RMSE_norm':>10s} {'RMSE_phys':>12s} {'unit':>8s}")
            for c, name in enumerate(var_order[:C]):
                phys = rmse_pc[c] * sd[c]
                extra = ""
                if "z@" in name or name == "z_surf":
                    extra = f"  (≈{phys / 9.81:.1f} gpm)"
                elif name == "t2m" or name.startswith("t@"):
                    extra = f"  (≈{phys:.2f} °C)"
                say(f"{indent}{c:3d} {name:>10s} {acc_pc[c]:8.4f} {rmse_pc[c]:10.4f} {phys:12.4f} "
                    f"{UNITS.get(name, '?'):>8s}{extra}")
            return False
        return True

    if AR > 1 and results.horizons:
        say("\nPer-horizon:")
        horizon_lines(results.horizons, "  ")
    if per_channel:
        normalized = channel_tables(sp, results.horizons, "  ", "\nPer-horizon per-channel RMSE (physical units):",
                                    f"\nPer-channel metrics overall (physical units, avg over {AR} horizons):")
        if normalized:
            var_order = list(variables) if variables is not None else [f"ch{c}" for c in range(C)]
            say("\nPer-channel ACC & RMSE (normalized):")
            for c, name in enumerate(var_order[:C]):
                say(f"  {c:2d}:{name:>10s}  ACC={sp.acc_per_channel[c]:.4f}  RMSE={sp.rmse_per_channel[c]:.4f}")
    if results.region is not None:
        rp, rb = results.region
        sk_r = 1.0 - (rp.rmse / (rb.rmse + 1e-12))
        say(f"\n--- Region {results.region_label} ({results.n_region} nodes) ---")
        say(f"RMSE={rp.rmse:.6f} | base={rb.rmse:.6f} | skill={sk_r * 100:.2f}%")
        say(f"ACC={rp.acc:.4f} | base={rb.acc:.4f}")
        if AR > 1 and results.region_horizons:
            say("\n  Per-horizon (region):")
            horizon_lines(results.region_horizons, "    ")
        if per_channel:
            channel_tables(rp, results.region_horizons, "    ",
                           f"\n  Per-horizon per-channel RMSE — REGION ({results.n_region} nodes):",
                           f"\n  Per-channel region (physical units, avg over {AR} horizons):")
    say("=" * 60)


def main(argv=None, device=None, use_graph=None):
    """`python -m graphcast_lite_amd.predict <experiment_dir> [options]`: the trained model of an experiment directory
    run over the test split, with the options of scripts/predict.py (and `--batch-size`); prints the inference summary
    and returns the `PredictRun`."""
    import json
    import os
    import sys

    import numpy as np

    from .assimilation import OptimalInterpolation, build_boundary_taper_mask, station_network
    from .config import ExperimentConfig
    from .data import load_chunked_datasets, load_train_and_test_datasets
    from .main import load_model_from_experiment_config
    from .train import FileNames
    from .utils import load_from_json_file
    from .verify import linspace_lats_lons

    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    exp_dir = args.experiment_dir
    cfg_path = os.path.join(exp_dir, FileNames.EXPERIMENT_CONFIG)
    ckpt_path = args.ckpt or os.path.join(exp_dir, FileNames.SAVED_MODEL)
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"no configuration: {cfg_path}")
    if not os.path.exists(ckpt_path):
        raise FileNotFoundError(f"no checkpoint: {ckpt_path}")
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("predict needs a GPU (the HIP path has no CPU fallback)")
        device = "cuda:0"
    device = torch.device(device)
    exp_cfg = ExperimentConfig(**load_from_json_file(cfg_path))
    data_dir = resolve_data_dir(args.data_dir, exp_cfg)
    chunked = is_chunked_dir(data_dir)
    C, P_model, OBS = exp_cfg.data.num_features_used, exp_cfg.data.pred_window_used, exp_cfg.data.obs_window_used
    AR = args.ar_steps if args.ar_steps else P_model
    print(f"[predict] data_dir={data_dir} (chunked={chunked}, pred_steps={AR})")
    if chunked:
        _, _, test_ds, meta = load_chunked_datasets(data_path=str(data_dir), obs_window=OBS, pred_steps=AR, n_features=C,
                                                    test_split=args.split, device=device)
    else:
        _, _, test_ds, meta = load_train_and_test_datasets(str(data_dir), exp_cfg.data, device=device)
    flat = getattr(meta, "flat_grid", False)
    # --- model
    real_coords = meta.cordinates if flat and hasattr(meta, "cordinates") else None
    region_bounds = None
    coords_file = os.path.join(str(data_dir), "coords.npz")
    if args.prune_mesh and os.path.exists(coords_file):
        z = np.load(coords_file)
        real_lats, real_lons = z["latitude"].astype(np.float32), z["longitude"].astype(np.float32)
        real_coords = (real_lats, real_lons)
        region_bounds = (float(real_lats.min()), float(real_lats.max()), float(real_lons.min()), float(real_lons.max()))
        print(f"[prune-mesh] data coordinates: lat=[{real_lats.min():.2f},{real_lats.max():.2f}] "
              f"lon=[{real_lons.min():.2f},{real_lons.max():.2f}]")
    model = load_model_from_experiment_config(exp_cfg, device, meta, coordinates=real_coords, region_bounds=region_bounds,
                                              mesh_buffer=args.mesh_buffer, flat_grid=flat)
    state = torch.load(ckpt_path, map_location=device, weights_only=True)
    if region_bounds is not None:  # the pruned mesh has edge features of its own
        state = {k: v for k, v in state.items() if not k.startswith("_processing_edge_features")}
    model.load_state_dict(state, strict=False)
    model = model.to(device)
    model.eval()
    G = meta.num_grid_nodes if flat else meta.num_longitudes * meta.num_latitudes
    if AR > P_model:
        print(f"[AR-rollout] the model returns {P_model} step(s); {AR} steps are run autoregressively")
    static_ch, forcing_ch = list(exp_cfg.static_channels or []), list(exp_cfg.forcing_channels or [])
    if static_ch:
        print(f"[static] channels {static_ch}: static, carried forward in the rollout")
    if forcing_ch:
        print(f"[forcing] channels {forcing_ch}: forcing, taken from the truth in the rollout")
    if args.max_samples is not None:
        max_samples = args.max_samples
    else:
        max_samples = min(len(test_ds), 200) if chunked else len(test_ds)
    print(f"[predict] device={device} | grid={meta.num_longitudes}x{meta.num_latitudes} | {max_samples}/{len(test_ds)} "
          f"test samples")
    # --- observations, background
    observations = None
    if args.assim_method != "none" and args.obs_path:
        observations = torch.load(args.obs_path, map_location="cpu", weights_only=True)
    elif args.assim_method != "none" and not chunked:
        print("[DA] the targets of the test split are the observations")
    boundary_mask = background = None
    if args.boundary_blending:
        if args.background_path:
            background = torch.load(args.background_path, map_location="cpu", weights_only=True)
            if background.dim() == 4:
                background = background.view(background.shape[0], -1, background.shape[-1])
        elif not chunked:
            background = test_ds.y.reshape(len(test_ds), G, -1)
        else:
            print("[Boundary] ERROR: a chunked data set needs --background-path")
            raise SystemExit(1)
        # viewed flat as [G] exactly as the reference views it, although the nodes are longitude-major
        boundary_mask = build_boundary_taper_mask(meta.num_latitudes, meta.num_longitudes, args.taper_width,
                                                  args.taper_width).reshape(G).float().to(device)
    # --- scored rows, OI, stations
    rows, label = scored_rows(args.region, getattr(exp_cfg, "boundary_mask_width", 0), meta, data_dir, G)
    oi = None
    if args.assim_method == "oi":
        if os.path.exists(coords_file):
            z = np.load(coords_file)
            lats, lons = z["latitude"].astype(np.float32), z["longitude"].astype(np.float32)
        else:
            lats, lons = linspace_lats_lons(meta.num_latitudes, meta.num_longitudes)
        roi_idx = rows
        if roi_idx is None and flat and getattr(meta, "is_regional", None) is not None:
            roi_idx = np.where(meta.is_regional)[0]
        oi = OptimalInterpolation(lats, lons, args.oi_sigma_b, args.oi_sigma_o, args.oi_corr_len, device, flat_grid=flat,
                                  roi_idx=roi_idx)
    stations = None
    if args.obs_sparsity is not None and args.assim_method != "none":
        pool = station_pool(args.obs_roi_only, rows, meta, G)
        stations = station_network(pool, args.obs_sparsity, args.obs_seed)
        print(f"[Inline-obs] {len(stations)} stations ({args.obs_sparsity * 100:.1f}% of {len(pool)} nodes, "
              f"seed={args.obs_seed})")
    obs_ch = None
    if args.obs_channels is not None:
        with open(os.path.join(str(data_dir), "variables.json")) as fh:
            obs_ch = observed_channels(args.obs_channels, json.load(fh), C)
    no_loss = sorted(set(static_ch) | set(forcing_ch))
    if no_loss:
        print(f"[metrics] left out of the aggregate scores: channels {no_loss} (static + forcing)")
    keep = bool(args.save) and not args.no_save
    print(f"[Main] inference ({max_samples} samples, DA={args.assim_method}, batch {args.batch_size})...")
    run = predict_experiment(model, test_ds, C, AR, pred_window=P_model, max_samples=max_samples,
                             batch_size=args.batch_size, use_residual=not args.no_residual, static_channels=static_ch,
                             forcing_channels=forcing_ch, region_rows=rows, region_label=label,
                             grid=(meta.num_longitudes, meta.num_latitudes), assim_method=args.assim_method,
                             nudging_mode=args.nudging_mode, nudging_alpha=args.nudging_alpha,
                             nudge_first_k=args.nudge_first_k, oi=oi, observations=observations, station_rows=stations,
                             obs_channels=obs_ch, boundary_mask=boundary_mask, background=background, keep=keep,
                             use_graph=use_graph, device=device)
    if keep:
        save_predictions(args.save, run.predictions, run.ground_truth, C, AR, OBS, meta.num_longitudes, meta.num_latitudes,
                         sample_offsets=run.sample_offsets, data_dir=str(data_dir))
        print(f"\n[Save] predictions → {args.save} (pred={tuple(run.predictions.shape)}, "
              f"gt={tuple(run.ground_truth.shape)})")
    variables = std = None
    if args.per_channel:
        var_path, scalers_path = os.path.join(str(data_dir), "variables.json"), os.path.join(str(data_dir), "scalers.npz")
        if os.path.exists(var_path):
            with open(var_path) as fh:
                variables = json.load(fh)
        if os.path.exists(scalers_path):
            std = np.load(scalers_path)["std"].astype(np.float64)[:C]
    inference_tables(run, per_channel=args.per_channel, variables=variables, std=std)
    return run


if __name__ == "__main__":
    main()
