"""The regional U-Net forecaster's inference scripts (`src/unet/predict.py`, `src/unet/predict_v2.py`) on the HIP path.

The two scripts differ in the model they build only.  Each takes windows of the fp16 series as 2-D grids, rolls the network
out autoregressively with carry-forward of the static and forcing channels, and scores every horizon against persistence:
RMSE in physical and normalised units, skill and the spatial anomaly correlation, printed as three tables.

Here the series stays in HBM.  A batch of windows is one `gcl_grid_window_pack` launch, and every autoregressive step is
the network's forward (`WeatherUNet`, `TrainableUNet` in eval mode or `WeatherUNetV2`, with `residual_from`) followed by one
`gcl_grid_forecast_step` (three launches: carry-forward, window shift and all five score families).  The accumulators live
on the device; `GridForecaster.results()` is the only host read.  With graphs enabled a whole batch - pack and every step -
is one hipGraph fed by a device tensor of window starts; a tail batch is padded with skipped rows (start -1).  Because the
samples' scores are added one after the other in batch order, the results do not depend on the batch size, bit for bit.
"""
import json
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .capture import Captured, graph_enabled
from .data import TimeseriesChunkDataset

DYNAMIC, STATIC, FORCING = 0, 1, 2


class Grid2DDataset:
    """`Grid2DDataset` of predict_v2.py:27-40 over a device-resident `data.TimeseriesChunkDataset`: the windows as planar
    grids `[channels, H = n_lat, W = n_lon]`, equal in bits to the reference wrapper's."""

    def __init__(self, chunk_ds: TimeseriesChunkDataset):
        if getattr(chunk_ds, "flat_grid", False) or not (chunk_ds.n_lon and chunk_ds.n_lat):
            raise ValueError("U-Net requires regular grid data")  # the reference's assertion (predict_v2.py:78)
        self.ds = chunk_ds
        self.H, self.W = int(chunk_ds.n_lat), int(chunk_ds.n_lon)

    def __len__(self):
        return len(self.ds)

    @property
    def channels(self) -> int:
        return int(self.ds.n_feat)

    def window_starts(self, indices: Sequence[int]):
        """[(chunk, t0)] of the samples `indices`."""
        n = len(self)
        pairs = []
        for i in indices:
            i = int(i)
            if not -n <= i < n:
                raise IndexError(f"Grid2DDataset: sample index {i} outside [0, {n})")
            pairs.append(self.ds._sample_indices[i])
        return pairs

    def _pack(self, pairs, first: int, frames: int, out=None):
        """Frames first .. first + frames of every window, [B, frames * C, H, W]; one launch per chunk touched."""
        ds = self.ds
        by_chunk = {}
        for pos, (ci, t) in enumerate(pairs):
            by_chunk.setdefault(ci, []).append((pos, t + first))
        shape = (len(pairs), frames * self.channels, self.H, self.W)
        if out is not None and (tuple(out.shape) != shape or not out.is_contiguous()):
            raise ValueError(f"Grid2DDataset.batch: out is a contiguous {list(shape)} tensor, got {tuple(out.shape)}")
        if len(by_chunk) == 1:
            (ci, items), = by_chunk.items()
            t0 = torch.tensor([t for _, t in items], dtype=torch.int64).to(ds.device)
            return hip.grid_window_pack(ds.chunks[ci], t0, ds.mean, ds.std, frames, out=out)
        X = out if out is not None else torch.empty(shape, dtype=torch.float32, device=ds.device)
        for ci, items in by_chunk.items():
            t0 = torch.tensor([t for _, t in items], dtype=torch.int64).to(ds.device)
            pos = torch.tensor([p for p, _ in items], dtype=torch.int64, device=ds.device)
            X.index_copy_(0, pos, hip.grid_window_pack(ds.chunks[ci], t0, ds.mean, ds.std, frames))
        return X

    def batch(self, indices: Sequence[int], out=None) -> torch.Tensor:
        """X [B, obs * C, H, W] of the samples `indices`, one launch per chunk touched."""
        pairs = self.window_starts(indices)
        if not pairs:
            raise ValueError("Grid2DDataset.batch: no samples")
        return self._pack(pairs, 0, self.ds.obs_window, out)

    def __getitem__(self, idx):
        """(X [obs * C, H, W], Y [pred * C, H, W]) on the device."""
        pairs = self.window_starts([idx])
        X = self._pack(pairs, 0, self.ds.obs_window)
        Y = self._pack(pairs, self.ds.obs_window, self.ds.pred_steps)
        return X[0], Y[0]


def channel_kinds(C: int, static_channels=(), forcing_channels=()) -> torch.Tensor:
    """uint8 [C]: 0 dynamic, 1 static, 2 forcing.  A channel in both lists is forcing: the script assigns the forcing
    channels after the static ones (predict_v2.py:142-148)."""
    kind = torch.zeros(C, dtype=torch.uint8)
    for name, chans, k in (("static", static_channels, STATIC), ("forcing", forcing_channels, FORCING)):
        for ch in chans:
            if not 0 <= int(ch) < C:
                raise ValueError(f"{name} channel {ch} outside [0, {C})")
            kind[int(ch)] = k
    return kind


class _ChunkRollout(Captured):
    """Pack + the autoregressive steps of one batch of windows of one chunk; `t0` is the only argument."""

    def __init__(self, owner: "GridForecaster", series, use_graph):
        super().__init__(use_graph=use_graph)
        self.owner, self.series = owner, series

    def _work(self, t0):
        f = self.owner
        ds = f.dataset.ds
        C, obs = f.C, ds.obs_window
        cur, nxt = f._windows
        hip.grid_window_pack(self.series, t0, ds.mean, ds.std, obs, out=cur)
        for step in range(f.steps_run):
            out = f.model(cur, residual_from=((obs - 1) * C, obs * C))
            hip.grid_forecast_step(out, cur, self.series, t0, f._kind, ds.mean, ds.std, step, nxt, f.state, f.acc_count,
                                   f.count, ws=f._ws)
            cur, nxt = nxt, cur
        return None

    def __call__(self, t0):
        return self._run(t0)


class GridForecaster:
    """The loop of predict_v2.py:113-180 for batches of samples.

    model: an eval-mode module of this package that accepts `forward(x, residual_from=...)` (`WeatherUNet`,
    `TrainableUNet`, `WeatherUNetV2`) with in_channels = obs * C and out_channels = C.  ar_steps: the horizons scored
    (default pred_steps); min(ar_steps, pred_steps) steps are run, as in the script.  `update(indices)` runs one batch of
    at most batch_size samples; `results()` reads the accumulators back."""

    def __init__(self, model, dataset: Grid2DDataset, static_channels=(), forcing_channels=(), ar_steps: Optional[int] = None,
                 batch_size: int = 8, use_graph=None):
        ds = dataset.ds
        self.model, self.dataset = model, dataset
        self.C, self.H, self.W = dataset.channels, dataset.H, dataset.W
        if model.training:
            raise ValueError("GridForecaster: the model must be in eval mode")
        if model.in_channels != ds.obs_window * self.C or model.out_channels != self.C:
            raise ValueError(f"GridForecaster: the model maps {model.in_channels} -> {model.out_channels} channels, the data set "
                             f"has obs * C = {ds.obs_window * self.C} and C = {self.C}")
        if batch_size < 1:
            raise ValueError(f"GridForecaster: batch_size {batch_size}")
        self.static_channels = [int(c) for c in static_channels]
        self.forcing_channels = [int(c) for c in forcing_channels]
        self.ar_steps = int(ar_steps) if ar_steps else int(ds.pred_steps)
        if self.ar_steps < 1:
            raise ValueError(f"GridForecaster: ar_steps {ar_steps}")
        self.steps_run = min(self.ar_steps, int(ds.pred_steps))
        self.batch_size = int(batch_size)
        self.use_graph = graph_enabled(use_graph)
        dev = ds.device
        self._kind = channel_kinds(self.C, self.static_channels, self.forcing_channels).to(dev)
        self.state = torch.zeros(self.ar_steps, self.C, 5, dtype=torch.float64, device=dev)
        self.acc_count = torch.zeros(self.ar_steps, self.C, dtype=torch.int64, device=dev)
        self.count = torch.zeros(self.ar_steps, dtype=torch.int64, device=dev)
        shape = (self.batch_size, ds.obs_window * self.C, self.H, self.W)
        self._windows = (torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.float32, device=dev))
        need = int(hip.lib().gcl_grid_forecast_step_ws_bytes(self.batch_size, self.H, self.W, self.C))
        self._ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
        self._rollouts = {}  # chunk -> _ChunkRollout
        self.n_samples = 0

    @property
    def graph_active(self) -> bool:
        return any(r.graph_active for r in self._rollouts.values())

    def update(self, indices: Sequence[int]):
        """Score the samples `indices` (at most batch_size of them)."""
        pairs = self.dataset.window_starts(indices)
        if not 1 <= len(pairs) <= self.batch_size:
            raise ValueError(f"GridForecaster.update: 1 .. {self.batch_size} samples per call, got {len(pairs)}")
        by_chunk = {}
        for ci, t in pairs:
            by_chunk.setdefault(ci, []).append(t)
        for ci, starts in by_chunk.items():
            run = self._rollouts.get(ci)
            if run is None:
                run = self._rollouts[ci] = _ChunkRollout(self, self.dataset.ds.chunks[ci], self.use_graph)
            # a fixed batch: the rows past the samples are skipped by the kernels (start -1)
            t0 = torch.tensor(starts + [-1] * (self.batch_size - len(starts)), dtype=torch.int64)
            run(t0.to(self.dataset.ds.device, non_blocking=True))
        self.n_samples += len(pairs)

    def run(self, n_samples: int):
        """`update` over samples 0 .. n_samples in batches."""
        for first in range(0, n_samples, self.batch_size):
            self.update(range(first, min(first + self.batch_size, n_samples)))
        return self

    def results(self) -> dict:
        """The accumulators (one host read) and the numbers predict_v2.py:188-271 derives from them."""
        state = self.state.cpu().numpy()
        acc = {"sum_se": state[:, :, 0].copy(), "sum_se_base": state[:, :, 1].copy(), "sum_nse": state[:, :, 2].copy(),
               "sum_nse_base": state[:, :, 3].copy(), "sum_acc": state[:, :, 4].copy(),
               "acc_count": self.acc_count.cpu().numpy(), "count": self.count.cpu().numpy(), "n_samples": self.n_samples}
        acc.update(derive(acc, self.static_channels, self.forcing_channels))
        return acc


def derive(acc: dict, static_channels=(), forcing_channels=()) -> dict:
    """The per-horizon and per-channel numbers of predict_v2.py:194-271, formed exactly as there (numpy float64 scalars and
    Python sums), from the accumulators sum_se, sum_se_base, sum_nse, sum_nse_base, sum_acc [AR, C], acc_count [AR, C] and
    count [AR]."""
    sum_se_h, sum_nse_h, sum_nse_base_h = acc["sum_se"], acc["sum_nse"], acc["sum_nse_base"]
    sum_acc_h, acc_count_h, count_h = acc["sum_acc"], acc["acc_count"], [int(n) for n in acc["count"]]
    ar, C = sum_se_h.shape
    no_loss_ch = sorted(set(static_channels) | set(forcing_channels))
    horizon_skill, horizon_acc = [], []
    for h in range(ar):
        skills_h, accs_h = [], []
        for c in range(C):
            if c in no_loss_ch:
                continue
            n = max(count_h[h], 1)
            rmse_c = np.sqrt(sum_nse_h[h][c] / n)
            rmse_b = np.sqrt(sum_nse_base_h[h][c] / n)
            skills_h.append((1.0 - rmse_c / rmse_b) * 100 if rmse_b > 1e-12 else 0)
            if acc_count_h[h][c] > 0:
                accs_h.append(sum_acc_h[h][c] / acc_count_h[h][c])
        horizon_skill.append(sum(skills_h) / max(len(skills_h), 1))
        horizon_acc.append(sum(accs_h) / max(len(accs_h), 1))
    rmse_phys = [[np.sqrt(sum_se_h[h][c] / max(count_h[h], 1)) for c in range(C)] for h in range(ar)]
    channel_rmse, channel_skill, channel_acc = [], [], []
    for c in range(C):
        rmse_vals, skill_vals, acc_vals = [], [], []
        for h in range(ar):
            if count_h[h] > 0:
                rmse_vals.append(np.sqrt(sum_se_h[h][c] / count_h[h]))
                rmse_c = np.sqrt(sum_nse_h[h][c] / count_h[h])
                rmse_b = np.sqrt(sum_nse_base_h[h][c] / count_h[h])
                skill_vals.append((1.0 - rmse_c / rmse_b) * 100 if rmse_b > 1e-12 else 0)
            if acc_count_h[h][c] > 0:
                acc_vals.append(sum_acc_h[h][c] / acc_count_h[h][c])
        channel_rmse.append(sum(rmse_vals) / max(len(rmse_vals), 1))
        channel_skill.append(sum(skill_vals) / max(len(skill_vals), 1))
        channel_acc.append(sum(acc_vals) / max(len(acc_vals), 1))
    dyn = [c for c in range(C) if c not in no_loss_ch]
    return {"horizon_skill": horizon_skill, "horizon_acc": horizon_acc, "rmse_phys": rmse_phys,
            "channel_rmse": channel_rmse, "channel_skill": channel_skill, "channel_acc": channel_acc,
            "mean_skill": sum(channel_skill[c] for c in dyn) / max(len(dyn), 1),
            "mean_acc": sum(channel_acc[c] for c in dyn) / max(len(dyn), 1)}


def _guess_unit(name: str) -> str:
    """predict_v2.py:275-291."""
    name = name.lower()
    if "t2m" in name or "t@" in name:
        return "K"
    if "u" in name or "v" in name:
        return "m/s"
    if "msl" in name or "sp" in name:
        return "Pa"
    if "z@" in name or "z_" in name:
        return "m²/s²"
    if "tp" in name:
        return "m"
    if "tcwv" in name or "q@" in name:
        return "kg/m²"
    if "lsm" in name:
        return "-"
    return "?"


def forecast_tables(results: dict, var_names, static_channels, forcing_channels, H: int, W: int, n_samples: int) -> str:
    """What predict_v2.py:190-272 prints, character for character, from the accumulators (or `GridForecaster.results()`)."""
    d = results if "horizon_skill" in results else derive(results, static_channels, forcing_channels)
    ar, C = np.asarray(results["sum_se"]).shape
    static_ch, forcing_ch = list(static_channels), list(forcing_channels)
    no_loss_ch = sorted(set(static_ch) | set(forcing_ch))
    hours = [6 * (h + 1) for h in range(ar)]
    lines = [f"\n{'=' * 70}", f"=== U-Net Inference ({n_samples} samples, AR={ar}) ===",
             f"Grid: {H}×{W} | C={C} (dynamic={C - len(no_loss_ch)})",
             "\nPer-horizon (dynamic channels, normalized skill):"]
    for h in range(ar):
        lines.append(f"  +{hours[h]:02d}h: avg_skill={d['horizon_skill'][h]:.1f}% | ACC={d['horizon_acc'][h]:.4f}")
    lines.append("\nPer-horizon per-channel RMSE (physical units):")
    lines.append(f"{'var':>10} {'unit':>6}" + "".join(f" {f'+{h}h':>8}" for h in hours))
    for c in range(C):
        if c in no_loss_ch:
            continue
        name = var_names[c] if c < len(var_names) else f"ch{c}"
        vals = []
        for h in range(ar):
            rmse = d["rmse_phys"][h][c]
            if "t2m" in name or "t@" in name:
                vals.append(f"{rmse:.2f}°C")
            elif "z@" in name or "z_" in name:
                vals.append(f"{rmse / 9.80665:.1f}m")
            else:
                vals.append(f"{rmse:.2f}")
        lines.append(f"{name:>10} {_guess_unit(name):>6}" + "".join(f" {v:>8}" for v in vals))
    lines.append(f"\nPer-channel metrics overall (avg over {ar} horizons):")
    lines.append(f"  {'#':>3} {'var':>10} {'ACC':>8} {'skill%':>8} {'RMSE_phys':>12} {'unit':>8}")
    for c in range(C):
        name = var_names[c] if c < len(var_names) else f"ch{c}"
        tag = " (static)" if c in static_ch else " (forcing)" if c in forcing_ch else ""
        lines.append(f"  {c:3d} {name:>10}   {d['channel_acc'][c]:6.4f}   {d['channel_skill'][c]:+6.1f}%   "
                     f"{d['channel_rmse'][c]:10.4f}   {_guess_unit(name):>6}{tag}")
    lines.append(f"\n  >>> MEAN (dynamic): skill={d['mean_skill']:.1f}% | ACC={d['mean_acc']:.4f}")
    lines.append("=" * 70)
    return "\n".join(lines) + "\n"


def detect_arch(state_dict, in_channels: int, out_channels: int, base_filters: int) -> str:
    """"v1" when the checkpoint's key set is `WeatherUNet`'s, else "v2"."""
    from .unet import WeatherUNet

    with torch.device("meta"):
        keys = set(WeatherUNet(in_channels, out_channels, base_filters).state_dict().keys())
    return "v1" if set(state_dict.keys()) == keys else "v2"


def predict_unet(experiment_dir: str, ckpt: Optional[str] = None, ar_steps: Optional[int] = None, max_samples: int = 200,
                 data_dir: Optional[str] = None, arch: str = "auto", batch_size: int = 8, device="cuda:0", use_graph=None):
    """`main()` of predict.py / predict_v2.py: the experiment's checkpoint run over the `test_only` split.  Returns
    `GridForecaster.results()` with the printed tables under "tables" (and "arch", "H", "W", "var_names")."""
    from .unet import WeatherUNet
    from .unet_v2 import WeatherUNetV2

    if arch not in ("auto", "v1", "v2"):
        raise ValueError(f"predict_unet: arch {arch!r} (auto, v1 or v2)")
    with open(os.path.join(experiment_dir, "config.json")) as fh:
        cfg = json.load(fh)
    data_dir = data_dir or cfg["data_dir"]
    C = cfg["num_features"]
    obs_window, pred_steps = cfg.get("obs_window", 2), cfg.get("pred_steps", 4)
    base_filters = cfg.get("base_filters", 64)
    static_ch, forcing_ch = cfg.get("static_channels", []), cfg.get("forcing_channels", [])
    ar_steps_eval = ar_steps or cfg.get("max_ar_steps", pred_steps)

    raw = TimeseriesChunkDataset(data_dir, obs_window, pred_steps, split="test_only", n_features=C, device=device)
    ds = Grid2DDataset(raw)
    n = min(max_samples, len(ds))

    ckpt_path = ckpt or os.path.join(experiment_dir, "best_model.pth")
    sd = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    if arch == "auto":
        arch = detect_arch(sd, obs_window * C, C, base_filters)
    if arch == "v1":
        model = WeatherUNet(obs_window * C, C, base_filters)
    else:
        model = WeatherUNetV2(obs_window * C, C, base_filters, cfg.get("attn_heads", 4), cfg.get("spectral_modes", 4))
    model.load_state_dict(sd, strict=True)
    model = model.to(device).eval()

    var_path = os.path.join(data_dir, "variables.json")
    if os.path.exists(var_path):
        with open(var_path) as fh:
            var_names = json.load(fh)
    else:
        var_names = [f"ch{i}" for i in range(C)]

    res = GridForecaster(model, ds, static_ch, forcing_ch, ar_steps_eval, batch_size, use_graph).run(n).results()
    res.update(arch=arch, H=ds.H, W=ds.W, var_names=var_names,
               tables=forecast_tables(res, var_names, static_ch, forcing_ch, ds.H, ds.W, n))
    return res


def build_parser():
    """The options of predict.py / predict_v2.py:45-50 with the scripts' names, types and defaults, plus `--arch` and
    `--batch-size`."""
    import argparse

    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.unet_predict")
    ap.add_argument("experiment_dir", help="e.g. experiments/unet_region_krsk")
    ap.add_argument("--ckpt", default=None, help="path to .pth (default: best_model.pth)")
    ap.add_argument("--ar-steps", type=int, default=None, help="AR rollout steps (default: from config)")
    ap.add_argument("--max-samples", type=int, default=200)
    ap.add_argument("--data-dir", default=None, help="override data_dir from config")
    ap.add_argument("--arch", default="auto", choices=["auto", "v1", "v2"],
                    help="WeatherUNet (v1) or WeatherUNetV2 (v2); auto: by the checkpoint's keys")
    ap.add_argument("--batch-size", type=int, default=8, help="samples per rollout call")
    return ap


def main(argv=None, device="cuda:0", use_graph=None):
    args = build_parser().parse_args(argv)
    res = predict_unet(args.experiment_dir, ckpt=args.ckpt, ar_steps=args.ar_steps, max_samples=args.max_samples,
                       data_dir=args.data_dir, arch=args.arch, batch_size=args.batch_size, device=device, use_graph=use_graph)
    print(res["tables"], end="")
    return res


if __name__ == "__main__":
    main()
