"""The training objective, the scores and the loop of the U-Net downscaler: what `scripts/train_downscaler.py` does on
either side of the network, on the device.

The reference evaluates `masked_mse_loss`, `spectral_loss` and `gradient_loss` (:189-220) as about twenty torch ops and
two `rfft2` per step; here the three terms and `d loss / d out` come from `csrc/downscale_loss.hip`
(`gcl_downscale_loss_fwd_bwd`, `gcl_downscale_spectral_fwd_bwd`) in float64 sums with a fixed order, and
`compute_metrics` (:271-310) from `gcl_downscale_metrics`.  `train_epoch`, `validate`, `compute_metrics` and
`fit_downscaler` (the loop of :422-506) take any callable that maps X [B, obs * C + Ns, H, W] to [B, C, H, W]; on the HIP
path that is `unet.TrainableUNet`, whose forward in training mode and backward run on `csrc/unet_train.hip`.
`python -m graphcast_lite_amd.downscale_train <experiment_dir> --data-dir D` (`build_parser`, `main`) is the script's
`main` (:316-420): config defaults, datasets, `TrainableUNet`, AdamW, cosine schedule, `fit_downscaler`.  Differences from the reference: sums in float64 (it sums in float32), the
random draws come from the caller's `torch.Generator` (`iter_batches`), and the losses accept 2 <= H, W <= 256 and
C <= 64 only.
"""
import json
import os
import sys
from datetime import datetime
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip


def _x_last(X, C: int, obs_window: Optional[int], who: str):
    """The view X[:, (obs - 1) * C : obs * C] (never copied); obs_window None: the reference's (X.shape[1] // C)."""
    if X is None:
        raise ValueError(f"{who}: residual needs the input X")
    if X.dim() != 4:
        raise ValueError(f"{who}: X is [B, obs * C + Ns, H, W], got {tuple(X.shape)}")
    obs = int(obs_window) if obs_window is not None else X.shape[1] // C
    if obs < 1 or obs * C > X.shape[1]:
        raise ValueError(f"{who}: {obs} frames of {C} channels in an input of {X.shape[1]} channels")
    if X.requires_grad:
        raise ValueError(f"{who}: an input X that requires grad is not supported")
    if not X.is_contiguous():
        X = X.contiguous()
    return X[:, (obs - 1) * C:obs * C]


def _mask(channel_mask):
    if channel_mask is None:
        return None
    if not isinstance(channel_mask, torch.Tensor):
        channel_mask = torch.as_tensor(channel_mask, dtype=torch.float32)
    return channel_mask


class _DownscalerLoss(torch.autograd.Function):
    """mse_w * mse + sw * spec + gw * grad as one node: forward launches the kernels with dOut requested, backward
    scales the saved dOut by the incoming gradient on the device."""

    @staticmethod
    def forward(ctx, out, Y, x_last, mask, mse_w, sw, gw, want):
        o = out.detach()
        rec = torch.zeros(3, dtype=torch.float64, device=o.device)
        dout = torch.empty_like(o) if want else None
        wrote = mse_w > 0 or gw > 0
        if wrote:
            hip.downscale_loss_fwd_bwd(o, Y, rec, x_last, mask, mse_w, gw, dout)
        if sw > 0:
            hip.downscale_spectral_fwd_bwd(o, Y, rec, x_last, mask, sw, dout, accumulate=wrote)
        total = (mse_w * rec[0] + gw * rec[1] + sw * rec[2]).to(torch.float32)
        ctx.save_for_backward(dout)
        ctx.mark_non_differentiable(rec)
        return total, rec

    @staticmethod
    def backward(ctx, g, _g_rec):
        (dout,) = ctx.saved_tensors
        return (hip.downscale_loss_scale(dout, g.to(torch.float32).contiguous()),) + (None,) * 7


def _loss(pred, target, x_last, channel_mask, mse_w, sw, gw, who):
    if target.requires_grad:
        raise ValueError(f"{who}: a target that requires grad is not supported (the gradient goes into pred only)")
    mask = _mask(channel_mask)
    if not pred.is_contiguous():
        pred = pred.contiguous()
    if not target.is_contiguous():
        target = target.contiguous()
    hip.downscale_loss_check(pred, target, x_last, mask, who)
    if mask is not None and not mask.is_contiguous():
        mask = mask.contiguous()
    want = torch.is_grad_enabled() and pred.requires_grad  # (dOut is formed only when a backward pass can follow)
    return _DownscalerLoss.apply(pred, target, x_last, mask, float(mse_w), float(sw), float(gw), want)


def masked_mse_loss(pred, target, channel_mask=None):
    """`train_downscaler.py:189-193`: mean over all B * C * H * W elements of m_c (pred - target)^2 (masked channels
    stay in the denominator).  A 0-dim float32 GPU tensor with autograd into pred."""
    return _loss(pred, target, None, channel_mask, 1.0, 0.0, 0.0, "masked_mse_loss")[0]


def spectral_loss(pred, target, channel_mask=None):
    """`train_downscaler.py:196-204`: the L1 distance of |rfft2(m_c pred, norm="ortho")| and the same of target, by a
    direct separable DFT in float64 (2 <= H, W <= 256)."""
    return _loss(pred, target, None, channel_mask, 0.0, 1.0, 0.0, "spectral_loss")[0]


def gradient_loss(pred, target, channel_mask=None):
    """`train_downscaler.py:207-220`: the mean squares of the finite differences of pred - target along H and W."""
    return _loss(pred, target, None, channel_mask, 0.0, 0.0, 1.0, "gradient_loss")[0]


def downscaler_loss(out, Y, X=None, obs_window=None, residual=False, channel_mask=None, spectral_weight=0.0,
                    gradient_weight=0.0, return_terms=False):
    """The objective of `train_epoch` (`train_downscaler.py:236-246`) as one autograd node: masked_mse_loss(o, Y) +
    spectral_weight * spectral_loss(o, Y) + gradient_weight * gradient_loss(o, Y) with o = out, or, with residual,
    o = X[:, (obs_window - 1) * C : obs_window * C] + out (the slice is read in place).  A term whose weight is not
    > 0 is skipped.  return_terms: (loss, (mse, spec, grad)), the terms as 0-dim float64 GPU tensors (0 when skipped)."""
    x_last = _x_last(X, int(Y.shape[1]), obs_window, "downscaler_loss") if residual else None
    sw = float(spectral_weight) if spectral_weight > 0 else 0.0
    gw = float(gradient_weight) if gradient_weight > 0 else 0.0
    loss, rec = _loss(out, Y, x_last, channel_mask, 1.0, sw, gw, "downscaler_loss")
    return (loss, (rec[0], rec[2], rec[1])) if return_terms else loss


# ======================================================================================================================
# Scores
# ======================================================================================================================
def metrics_table(rmse_model, rmse_coarse, skill, var_names, static_channels=()):
    """The lines `train_downscaler.py:486-494` logs, character for character."""
    static = set(int(c) for c in static_channels)
    lines = [f"\n{'Variable':>12}  {'RMSE_model':>10}  {'RMSE_coarse':>11}  {'Skill':>8}", "-" * 48]
    for i in range(len(rmse_model)):
        if i in static:
            continue
        lines.append(f"{var_names[i]:>12}  {rmse_model[i]:10.4f}  {rmse_coarse[i]:11.4f}  {skill[i]:>7.1%}")
    mean_skill = np.mean([skill[i] for i in range(len(rmse_model)) if i not in static])
    lines.append(f"\n{'MEAN':>12}  {'':>10}  {'':>11}  {mean_skill:>7.1%}")
    return lines


def downscaler_results(test_loss, rmse_model, skill, var_names, static_channels=()):
    """The dictionary `train_downscaler.py:497-502` writes to results.json."""
    static = set(int(c) for c in static_channels)
    C = len(rmse_model)
    mean_skill = np.mean([skill[i] for i in range(C) if i not in static])
    return {
        "test_loss": float(test_loss),
        "mean_skill_vs_coarse": float(mean_skill),
        "per_channel_rmse": {var_names[i]: float(rmse_model[i]) for i in range(C)},
        "per_channel_skill": {var_names[i]: float(skill[i]) for i in range(C) if i not in static},
    }


class DownscalerMetrics:
    """`compute_metrics` (`train_downscaler.py:271-310`) batch by batch on the device: `update` adds the per-batch means
    of (o - Y)^2 and (x_last - Y)^2 per channel to a float64 state and advances a device-side batch counter (one
    `gcl_downscale_metrics` call, no host sync, replayable from a captured graph); `results` averages them over the
    batches as the reference does, so a short last batch weighs as much as a full one (`coarse_baseline` sums over
    samples instead).  std: the per-channel scale of the physical units."""

    def __init__(self, C: int, std, static_channels: Sequence[int] = ()):
        self.C, self.static_channels = int(C), [int(c) for c in static_channels]
        self.std = np.asarray(std.detach().cpu() if isinstance(std, torch.Tensor) else std).astype(np.float64).reshape(-1)
        if len(self.std) != self.C:
            raise ValueError(f"DownscalerMetrics: a scale of {len(self.std)} channels for {self.C}")
        self.state, self.count = None, None

    def update(self, out, X, Y, residual: bool = False, obs_window: Optional[int] = None):
        if int(Y.shape[1]) != self.C:
            raise ValueError(f"DownscalerMetrics: a target of {Y.shape[1]} channels for {self.C}")
        x_last = _x_last(X, self.C, obs_window, "DownscalerMetrics.update")
        if self.state is None:
            self.state = torch.zeros(self.C, 2, dtype=torch.float64, device=Y.device)
            self.count = torch.zeros(1, dtype=torch.int64, device=Y.device)
        hip.downscale_metrics(out.detach().contiguous(), x_last, Y.contiguous(), residual, self.state, self.count)

    def results(self):
        """(rmse_model, rmse_coarse, skill), float64 [C] each, in physical units."""
        if self.state is None:
            raise ValueError("DownscalerMetrics: no batch was added")
        n = int(self.count.item())
        mse = self.state.cpu().numpy() / n
        rmse_model, rmse_coarse = np.sqrt(mse[:, 0]) * self.std, np.sqrt(mse[:, 1]) * self.std
        return rmse_model, rmse_coarse, 1.0 - rmse_model / (rmse_coarse + 1e-8)

    def table(self, var_names, results=None):
        rmse_model, rmse_coarse, skill = self.results() if results is None else results
        return metrics_table(rmse_model, rmse_coarse, skill, var_names, self.static_channels)


# ======================================================================================================================
# Batches, epochs, the loop
# ======================================================================================================================
def iter_batches(ds, batch_size: int, shuffle: bool = False, drop_last: bool = False, generator=None):
    """(X, Y) batches of a `DownscalerDataset`, one `DownscalerDataset.batch` launch each.  The order (with shuffle), the
    flips (one uniform draw per sample, flipped below 0.5, when the data set flips) and the input noise (standard
    normals [B, obs * C, H, W], when the data set adds noise) all come from `generator`, in that order per epoch and
    per batch, drawn on the generator's device; None: torch's global generator on the CPU."""
    n, bs = len(ds), int(batch_size)
    if bs < 1:
        raise ValueError(f"iter_batches: a batch size of {bs}")
    gdev = generator.device if generator is not None else torch.device("cpu")
    order = torch.randperm(n, generator=generator, device=gdev).tolist() if shuffle else list(range(n))
    dev = ds.coarse.device
    for a in range(0, n, bs):
        idx = order[a:a + bs]
        if drop_last and len(idx) < bs:
            break
        flip = noise = None
        if ds.augment_flip:
            flip = (torch.rand(len(idx), generator=generator, device=gdev) < 0.5).to(dev)
        if ds.input_noise > 0:
            noise = torch.randn(len(idx), ds.obs_window * ds.C, ds.n_lat, ds.n_lon, generator=generator, device=gdev).to(dev)
        yield ds.batch(idx, flip=flip, noise=noise)


def _set_mode(model, training: bool):
    if isinstance(model, torch.nn.Module):
        model.train(training)


def train_epoch(model, batches, optimizer, channel_mask, residual, spectral_weight=0.0, gradient_weight=0.0,
                obs_window=None, per_batch=None):
    """`train_downscaler.py:226-252` over any iterable of (X, Y) device tensors: the mean of the per-batch losses.  The
    objective and its gradient with respect to the network's output are `downscaler_loss`; the backward pass of the
    network is the caller's network's own (`unet.TrainableUNet`: the kernels of csrc/unet_train.hip, through autograd);
    gradient clipping (`clip_grad_norm_`, max norm 1.0) and `optimizer.step()` stay torch calls.  The losses are added on the device (float64) and read once at the end.  per_batch: a list
    that receives every batch's loss as a 0-dim GPU tensor."""
    _set_mode(model, True)
    total, n = None, 0
    params = [p for g in optimizer.param_groups for p in g["params"]]
    for X, Y in batches:
        optimizer.zero_grad()
        out = model(X)
        loss = downscaler_loss(out, Y, X=X, obs_window=obs_window, residual=residual, channel_mask=channel_mask,
                               spectral_weight=spectral_weight, gradient_weight=gradient_weight)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        optimizer.step()
        cur = loss.detach()
        total = cur.double() if total is None else total + cur.double()
        if per_batch is not None:
            per_batch.append(cur)
        n += 1
    if n == 0:
        raise ValueError("train_epoch: no batches")
    return float(total.item()) / n


@torch.no_grad()
def validate(model, batches, channel_mask, residual, C=None, obs_window=None):
    """`train_downscaler.py:255-268`: the mean over the batches of masked_mse_loss."""
    _set_mode(model, False)
    total, n = None, 0
    for X, Y in batches:
        loss = downscaler_loss(model(X), Y, X=X, obs_window=obs_window, residual=residual, channel_mask=channel_mask)
        total = loss.double() if total is None else total + loss.double()
        n += 1
    if n == 0:
        raise ValueError("validate: no batches")
    return float(total.item()) / n


@torch.no_grad()
def compute_metrics(model, batches, channel_mask, residual, C, std, exclude_channels=None, obs_window=None):
    """`train_downscaler.py:271-310`: (rmse_model, rmse_coarse, skill), float64 [C] in physical units (channel_mask and
    exclude_channels are accepted and unused, as in the reference)."""
    _set_mode(model, False)
    m = DownscalerMetrics(C, std)
    for X, Y in batches:
        m.update(model(X), X, Y, residual, obs_window)
    return m.results()


def fit_downscaler(model, optimizer, scheduler, train_ds, val_ds, test_ds, exp_dir, num_epochs, patience,
                   batch_size: int = 32, channel_mask=None, residual: bool = False, spectral_weight: float = 0.0,
                   gradient_weight: float = 0.0, static_channels=None, var_names=None, generator=None,
                   data_dir: str = "", log=print):
    """The loop of `train_downscaler.py:422-506` around a caller-supplied network (`unet.TrainableUNet` on the HIP path;
    any nn.Module that maps X to the output works), optimizer and scheduler: epochs of
    `train_epoch` (shuffled, last short batch dropped) and `validate`, the best state in exp_dir/best_model.pth, early
    stopping after `patience` epochs without a better validation loss, then the best state reloaded, the test loss and
    the table of `compute_metrics`; everything logged to exp_dir/training_log.txt in the reference's format (the
    seconds as measured) and exp_dir/results.json with its four keys.  channel_mask None: ones with the static
    channels zeroed (:409-411).  Returns the results dictionary."""
    os.makedirs(exp_dir, exist_ok=True)
    C, obs = train_ds.C, train_ds.obs_window
    dev = train_ds.coarse.device
    static_ch = [int(c) for c in (train_ds.static_channels if static_channels is None else static_channels)]
    if channel_mask is None:
        m = np.ones(C, dtype=np.float32)
        m[static_ch] = 0.0
        channel_mask = torch.from_numpy(m).to(dev)
    if var_names is None:
        var_names = train_ds.pairs.variables or [f"ch{i}" for i in range(C)]
    ckpt_path, log_path = os.path.join(exp_dir, "best_model.pth"), os.path.join(exp_dir, "training_log.txt")

    def _log(msg):
        if log is not None:
            log(msg)
        with open(log_path, "a") as fh:
            fh.write(msg + "\n")

    sw, gw = spectral_weight, gradient_weight
    _log(f"=== Downscaler training started: {datetime.now().isoformat()} ===")
    _log(f"data_dir={data_dir}  epochs={num_epochs}  batch={batch_size}  lr={optimizer.param_groups[0]['lr']}")
    _log(f"gnn_input={train_ds.coarse is train_ds.pairs.gnn_pred}  spectral_w={sw}  gradient_w={gw}  "
         f"noise={train_ds.input_noise}  flip={train_ds.augment_flip}")
    _log(f"{'epoch':>5}  {'train_loss':>10}  {'val_loss':>10}  {'best':>10}  {'lr':>8}")
    _log("-" * 55)

    best_val_loss, patience_counter = float("inf"), 0
    for epoch in range(num_epochs):
        t0 = datetime.now()
        train_loss = train_epoch(model, iter_batches(train_ds, batch_size, True, True, generator), optimizer,
                                 channel_mask, residual, sw, gw, obs)
        val_loss = validate(model, iter_batches(val_ds, batch_size), channel_mask, residual, C, obs)
        scheduler.step()
        improved = ""
        if val_loss < best_val_loss:
            best_val_loss, patience_counter = val_loss, 0
            torch.save(model.state_dict(), ckpt_path)
            improved = " *"
        else:
            patience_counter += 1
        cur_lr = optimizer.param_groups[0]["lr"]
        dt = (datetime.now() - t0).total_seconds()
        _log(f"{epoch+1:5d}  {train_loss:10.6f}  {val_loss:10.6f}  {best_val_loss:10.6f}  {cur_lr:.1e}{improved}  ({dt:.0f}s)")
        if patience_counter >= patience:
            _log(f"Early stopping at epoch {epoch+1}")
            break

    _log("\n" + "=" * 55)
    _log("[TEST] Loading best model...")
    model.load_state_dict(torch.load(ckpt_path, map_location=dev))
    test_loss = validate(model, iter_batches(test_ds, batch_size), channel_mask, residual, C, obs)
    metrics = DownscalerMetrics(C, train_ds.std_np, static_ch)
    with torch.no_grad():
        for X, Y in iter_batches(test_ds, batch_size):
            metrics.update(model(X), X, Y, residual, obs)
    rmse_model, rmse_coarse, skill = metrics.results()
    _log(f"\n[TEST] loss={test_loss:.6f}")
    for line in metrics.table(var_names, (rmse_model, rmse_coarse, skill)):
        _log(line)
    results = downscaler_results(test_loss, rmse_model, skill, var_names, static_ch)
    with open(os.path.join(exp_dir, "results.json"), "w") as fh:
        json.dump(results, fh, indent=2)
    _log(f"\nResults saved to {exp_dir}")
    return results


# ======================================================================================================================
# The entry point
# ======================================================================================================================
CONFIG_DEFAULTS = {  # train_downscaler.py:344-354
    "num_features": 19, "obs_window": 2, "batch_size": 32, "learning_rate": 1e-3, "num_epochs": 50, "patience": 15,
    "base_filters": 64, "static_context": True, "residual": False, "static_channels": [7, 8], "random_seed": 42,
}
WIND_U_NAMES = ("10u", "u@850", "u@500")  # :366-369: negated on a horizontal flip


def build_parser():
    """The options of scripts/train_downscaler.py:317-330 with the reference's names, types and defaults."""
    import argparse

    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.downscale_train")
    ap.add_argument("experiment_dir", help="e.g. experiments/downscaler_krsk")
    ap.add_argument("--data-dir", required=True, help="Path to downscaler dataset")
    ap.add_argument("--gnn-input", action="store_true", help="Use GNN predictions (gnn_pred.npy) instead of ERA5 coarse")
    ap.add_argument("--spectral-weight", type=float, default=0.0, help="Weight for FFT spectral loss (e.g. 0.1)")
    ap.add_argument("--gradient-weight", type=float, default=0.0, help="Weight for spatial gradient loss (e.g. 0.05)")
    ap.add_argument("--input-noise", type=float, default=0.0, help="Gaussian noise sigma added to input (e.g. 0.05)")
    ap.add_argument("--augment-flip", action="store_true", help="Random horizontal flip augmentation")
    return ap


def load_config(exp_dir: str) -> dict:
    """exp_dir/config.json over `CONFIG_DEFAULTS` (:336-354); a missing file gives the defaults."""
    cfg = dict(CONFIG_DEFAULTS)
    path = os.path.join(exp_dir, "config.json")
    if os.path.exists(path):
        with open(path) as fh:
            cfg.update({k: v for k, v in json.load(fh).items() if k in CONFIG_DEFAULTS})
    return cfg


def wind_u_channels(data_dir: str):
    """:364-369: the indices of the wind-u variables in data_dir/variables.json (none when the file is missing)."""
    path = os.path.join(data_dir, "variables.json")
    if not os.path.exists(path):
        return ()
    with open(path) as fh:
        return tuple(i for i, v in enumerate(json.load(fh)) if v in WIND_U_NAMES)


def main(argv=None, device="cuda:0", log=print):
    """`python -m graphcast_lite_amd.downscale_train <experiment_dir> --data-dir D [options]`: `main` of
    scripts/train_downscaler.py (:316-506) with `unet.TrainableUNet` as the network.  Returns the results dictionary of
    `fit_downscaler`."""
    from .downscale import DownscalerDataset
    from .unet import TrainableUNet

    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    exp_dir = args.experiment_dir
    os.makedirs(exp_dir, exist_ok=True)
    cfg = load_config(exp_dir)
    C, obs, static_ch = cfg["num_features"], cfg["obs_window"], cfg["static_channels"]
    torch.manual_seed(cfg["random_seed"])
    np.random.seed(cfg["random_seed"])
    wind_u = wind_u_channels(args.data_dir)
    if args.augment_flip and wind_u and log is not None:
        log(f"Wind-u channels to negate on flip: {wind_u}")
    kw = dict(obs_window=obs, static_context=cfg["static_context"], use_gnn_input=args.gnn_input, device=device)
    train_ds = DownscalerDataset(args.data_dir, split="train", augment_flip=args.augment_flip, input_noise=args.input_noise,
                                 wind_u_channels=wind_u, **kw)
    val_ds = DownscalerDataset(train_ds.pairs, split="val", **kw)
    test_ds = DownscalerDataset(train_ds.pairs, split="test", **kw)
    n_static = len(static_ch) if cfg["static_context"] else 0
    in_channels = obs * C + n_static
    model = TrainableUNet(in_channels=in_channels, out_channels=C, base_filters=cfg["base_filters"]).to(device)
    if log is not None:
        log(f"WeatherUNet: {model.num_params:,} params | in={in_channels} out={C} filters={cfg['base_filters']}")
        log(f"Grid: {train_ds.n_lat}x{train_ds.n_lon} (HxW) | obs={obs}")
    optimizer = torch.optim.AdamW(model.parameters(), lr=cfg["learning_rate"], weight_decay=1e-5)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=cfg["num_epochs"])
    return fit_downscaler(model, optimizer, scheduler, train_ds, val_ds, test_ds, exp_dir, cfg["num_epochs"], cfg["patience"],
                          batch_size=cfg["batch_size"], residual=cfg["residual"], spectral_weight=args.spectral_weight,
                          gradient_weight=args.gradient_weight, static_channels=static_ch, data_dir=args.data_dir, log=log)


if __name__ == "__main__":
    main()
