"""Train, validate and score the regional heads without leaving the HIP path: the loops of the reference's
`scripts/train_dual_mesh.py` and `scripts/train_roi_residual.py` under their own names.

  GlobalOutputCache     train_dual_mesh.py:548-580  `--precompute`: the frozen global model's outputs of a whole split,
                                                    kept in HBM in the layout the regional kernels read
  DualMeshCacheStep     train_dual_mesh.py:176-193  one cached optimiser step fed by a device slot index
  apply_special_channels  :51-60     overfit_test  :63-135     train_dual_epoch  :138-255     eval_dual  :260-368
  fit_dual_mesh         train_dual_mesh.py:528-656  the training loop, its log, checkpoints and results.json
  train_roi_epoch / eval_roi_epoch / fit_roi_residual   train_roi_residual.py:91-192, 308-367
  predict_dual_mesh, UNITS, regional_tables   predict_dual_mesh.py:37-45, 203-438
  main                  `python -m graphcast_lite_amd.regional_train {dual,roi,predict} <experiment_dir> ...`

How it runs:
  * `GlobalOutputCache.add` is one frozen global forward and ONE `gcl_region_cache_store` per batch: a record per
    sample holds roi_input, the cross senders' mesh rows in the order `_regional` takes them, the ROI rows of the
    global prediction and of the target.  `precompute_global`'s CPU dictionaries are never built (`as_reference`
    rebuilds one from a record, bit for bit, for whoever wants it);
  * `DualMeshCacheStep` is `gcl_region_cache_fetch` (records named by a DEVICE int64 slot array into the step's static
    buffers) followed by the calls `DualMeshCachedStep` makes; captured, an epoch is graph replays that differ in the
    eight bytes of the slot;
  * the standard mode trains on `DualTrainStep`, a `TrainStep(spatial_mask=roi_mask, ar_steps=...)` that scores a step
    after the static / forcing overwrite, as the script does;
  * `eval_dual` advances the corrected and the global-only rollout in lock-step through `gcl_region_eval_pair`, which
    also adds both ROI losses into a float64 device state: one host read per pass.  Step 0 shares one global forward.

What differs from the reference: the `optimizer` argument of the epoch functions is the fused step that owns the Adam
state (`DualTrainStep` or `DualMeshCacheStep`); the cached mode accepts batches of more than one sample; epoch sums are
kept in float64 on the device instead of adding up `.item()`s; wandb and the 4-worker DataLoader are not provided.
"""
import argparse
import json
import os
import sys
import time
from copy import deepcopy

import numpy as np
import torch

from . import hip
from .capture import Captured, graph_enabled
from .roi_residual import ROIComposeFn, _pad4
from .train import (FileNames, FlatParams, FusedAdam, TrainStep, _channel_kinds, allreduce_gradients,
                    weighted_mse_loss)

MAX_PATIENCE = 10  # train_dual_mesh.py:532, train_roi_residual.py:311


def _own_state(model):
    """The state dict without the frozen global model (`best_regional.pth`, `best_head.pth`)."""
    return {k: v for k, v in model.state_dict().items() if not k.startswith("global_model.")}


def _batch(X, y, device):
    y = y.squeeze(0) if y.dim() == 4 else y
    X, y = X.to(device), y.to(device)
    if X.dim() == 2:
        X, y = X.unsqueeze(0), y.unsqueeze(0)
    if X.stride(2) != 1:
        X = X.contiguous()
    if y.stride(2) != 1:
        y = y.contiguous()
    return X, y


# ------------------------------------------------------------------------------------------------------------------
# The cache of global outputs and the cached step
# ------------------------------------------------------------------------------------------------------------------
class GlobalOutputCache:
    """The global outputs of `n_samples` samples on the device, one record each (see gcl_region_cache_record_bytes)."""

    def __init__(self, model, n_samples: int, pred_steps: int = 1):
        self.model = model
        self.device = model.roi_mask.device
        C = model.n_features
        self.rec = hip.RegionRecord(model.n_roi_grid, model._cross.half, C * model.obs_window, model.global_latent_dim,
                                    model.global_latent_dim, C, pred_steps)
        self.data = torch.zeros(int(n_samples), self.rec.nbytes // 4, dtype=torch.float32, device=self.device)
        self.count = 0

    def __len__(self):
        return self.count

    @property
    def nbytes(self) -> int:
        return self.data.numel() * 4

    @torch.no_grad()
    def add(self, X, y):
        """Append the samples of one batch: the frozen global forward, then one store launch.  Returns their slots
        (device int64 [B])."""
        X3, y3 = _batch(X, y, self.device)
        B = X3.shape[0]
        if self.count + B > self.data.shape[0]:
            raise ValueError(f"GlobalOutputCache holds {self.data.shape[0]} samples, {self.count} are in, {B} more do not fit")
        pred3, lat3, mesh3 = self.model._global(X3, 0.0)
        slots = torch.arange(self.count, self.count + B, dtype=torch.int64, device=self.device)
        hip.region_cache_store(self.rec, self.data, slots, pred3, lat3, mesh3, X3, y3, self.model._roi_rows,
                               self.model._cross.snd)
        self.count += B
        return slots

    def fetch(self, slots_dev, out=None):
        """(roi3 [B, n_roi, Sp], send [B, half_E, Dgp], pred [B, n_roi, Cp], y [B, n_roi, Yp]) of the named records."""
        return hip.region_cache_fetch(self.rec, self.data, slots_dev, out=out)

    def sample(self, i: int):
        """(roi_raw [n_roi, obs*C], `precompute_global`'s dictionary, y_roi [n_roi, P*C]) of sample i as CPU tensors:
        what the reference's cached mode feeds `forward_cached` and its loss with, bit for bit."""
        r = self.rec
        roi3, send, pred, y = (t[0].cpu() for t in self.fetch(torch.full((1,), int(i), dtype=torch.int64,
                                                                          device=self.device)))
        cs = torch.empty(r.half_E, r.Dm)
        cs[self.model._cross.order_cpu] = send[:, :r.Dm]  # back from the receiver-sorted order to the reference's
        ref = {"global_pred_roi": pred[:, :r.C].contiguous(), "roi_grid_latent": roi3[:, r.XF:r.XF + r.D].contiguous(),
               "cross_sender_feat": cs}
        return roi3[:, :r.XF].contiguous(), ref, y[:, :r.P * r.C].contiguous()

    def as_reference(self, i: int) -> dict:
        """The dictionary `model.precompute_global` returns for sample i (CPU tensors, the same bits)."""
        return self.sample(i)[1]

    @classmethod
    def build(cls, model, batches, name: str = "train", n_samples=None, log=print):
        """The `_build_cache` loop of train_dual_mesh.py:558-574 over an iterable of (X, y) batches."""
        t0 = time.time()
        if n_samples is None:
            ds = getattr(batches, "dataset", None)
            if ds is None:
                batches = list(batches)
            n_samples = len(ds) if ds is not None else sum(1 if b[0].dim() == 2 else b[0].shape[0] for b in batches)
        cache, n = None, len(batches) if hasattr(batches, "__len__") else None
        for i, (X, y) in enumerate(batches):
            if cache is None:
                y3 = y.squeeze(0) if y.dim() == 4 else y
                cache = cls(model, n_samples, pred_steps=y3.shape[-1] // model.n_features)
            cache.add(X, y)
            if (i + 1) % 500 == 0:
                log(f"  {name}: {i + 1}/{n} ({time.time() - t0:.0f}s)")
        if cache is None:
            raise ValueError(f"GlobalOutputCache.build: no {name} batch to cache")
        torch.cuda.synchronize(cache.device)
        mem_mb = cache.count * cache.rec.nbytes / 1e6
        log(f"  {name}: {cache.count} samples cached in {time.time() - t0:.0f}s ({mem_mb:.0f} MB)")
        return cache


class DualMeshCacheStep(Captured):
    """One optimiser step of the reference's cached mode (scripts/train_dual_mesh.py:176-193) over a
    `GlobalOutputCache`: `__call__(slots)` with a device int64 [B] array of cache slots.  Fetch (one launch), then
    `model._regional`, the composition with the cached global prediction, the ROI loss (with the last input slot added
    first when `use_residual`), backward and Adam: the calls `DualMeshCachedStep` makes, and at B = 1 the same bits.
    `use_graph` as for `TrainStep`; a replay differs from the previous one in the slots only."""

    def __init__(self, model, cache: GlobalOutputCache, lr=1e-3, use_residual: bool = False, use_graph=None):
        if cache.model is not model:
            raise ValueError("DualMeshCacheStep: the cache was built for another model")
        self.model, self.cache = model, cache
        self.flat = FlatParams(model)
        self.opt = FusedAdam(self.flat, lr=lr)
        self.use_residual = use_residual
        self._bufs = {}
        super().__init__(graph_enabled(use_graph), required=use_graph is True)

    def buffers(self, B: int):
        """The static (roi3, send, pred, y) buffers the step of batch size B fetches into."""
        b = self._bufs.get(B)
        if b is None:
            b = self._bufs[B] = self.cache.rec.parts(B, self.cache.device)
        return b

    def _work(self, slots):
        r, m = self.cache.rec, self.model
        roi3, send3, pred3, y3 = self.cache.fetch(slots, out=self.buffers(slots.numel()))
        # a fill kernel, not `flat.zero_grad()`'s stream memset: replays of the captured memset node were seen to leave a
        # 16-byte pattern over the bucket when an eager step of a twin model ran between them; cause unknown
        self.flat.grad.zero_()
        corr = m._regional(roi3, send3)
        out = ROIComposeFn.apply(pred3[..., :r.C], corr, m._roi_ident, m._roi_ident)
        x_last = roi3[..., r.XF - r.C:r.XF] if self.use_residual else None
        loss = weighted_mse_loss(out, y3[..., :r.C], x_last=x_last)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def __call__(self, slots):
        return self._run(slots.to(self.cache.device, torch.int64).reshape(-1)).detach()


# ------------------------------------------------------------------------------------------------------------------
# scripts/train_dual_mesh.py
# ------------------------------------------------------------------------------------------------------------------
def apply_special_channels(out, prev_state, target_step, static_channels=None, forcing_channels=None):
    """train_dual_mesh.py:51-60: carry the static channels forward and inject the known forcing channels (in place).
    The loops here do this inside `gcl_region_eval_pair` / the fused AR step; this is the reference's helper."""
    if static_channels:
        prev_last = prev_state[:, :, -1, :]
        for ch in static_channels:
            out[:, :, ch] = prev_last[:, :, ch]
    if forcing_channels and target_step is not None:
        for ch in forcing_channels:
            out[:, :, ch] = target_step[:, :, ch]
    return out


def _dual_parts(model, X3):
    """(global prediction [B, G, C], corrected prediction [B, G, C]) of one frozen global forward (`forward`'s body)."""
    pred3, lat3, mesh3 = model._global(X3, 0.0)
    B, G = X3.shape[0], X3.shape[1]
    roi3 = hip.roi_gather_rows(model._roi_rows, G, [X3, lat3], _pad4(model.reg_enc_input_dim), B)
    send3 = hip.roi_gather_rows(model._cross.snd, mesh3.shape[1], [mesh3], _pad4(model.global_latent_dim), B)
    corr = model._regional(roi3, send3)
    return pred3, hip.roi_compose(pred3, corr, model._roi_pos)


def _roi_parts(model, X3):
    """The same for `ROIResidualModel`."""
    pred3, lat3 = model._global(X3, 0.0)
    return pred3, hip.roi_compose(pred3, model._head(X3, pred3, lat3), model._roi_pos)


def _parts(model, X3):
    return _dual_parts(model, X3) if hasattr(model, "_regional") else _roi_parts(model, X3)


def _grad_report(model, what: str, say, scale: float = 1.0):
    """The `[GradCheck]` report of train_dual_mesh.py:231-248 from the gradients the last step left in place (`scale`:
    the factor the step applies to them inside Adam, see `DualTrainStep`)."""
    say(f"[GradCheck] {what}.requires_grad: True")
    module_grads = {}
    for name, p in model.named_parameters():
        if p.requires_grad and p.grad is not None:
            module_grads.setdefault(name.split(".")[0], []).append((name, p.grad.norm().item() * scale))
    for module, grads in sorted(module_grads.items()):
        max_gn = max(g for _, g in grads)
        mean_gn = sum(g for _, g in grads) / len(grads)
        top_param = max(grads, key=lambda x: x[1])
        say(f"  [{module}] {len(grads)} params, max_grad={max_gn:.6f}, mean_grad={mean_gn:.6f}")
        say(f"    top: {top_param[0]} = {top_param[1]:.6f}")
    return module_grads


def overfit_test(model, dataloader, device, use_residual=False, n_steps=200, lr=0.01, say=print):
    """train_dual_mesh.py:63-135 (and train_roi_residual.py:32-88, which never adds the residual): `n_steps` fused
    steps on the first batch, the `|correction|` lines every 20 steps, the weights restored afterwards."""
    say("\n" + "=" * 60)
    say("[OverfitTest] 1 sample, {} steps, lr={}...".format(n_steps, lr))
    say("=" * 60)
    X, y = _batch(*next(iter(dataloader)), device)
    C = X.shape[-1] // model.obs_window
    y0 = y[:, :, :C]
    saved_state = deepcopy(_own_state(model))
    model.train()
    model.global_model.eval()
    step = TrainStep(model, lr=lr, spatial_mask=model.roi_mask.view(1, -1, 1).float(), use_residual=use_residual,
                     use_graph=False)
    rows = model._roi_rows.long()
    for i in range(n_steps):
        report = i % 20 == 0 or i == n_steps - 1
        if report:  # the correction of the forward this step's loss comes from (the weights before its update)
            with torch.no_grad():
                glob, out = _parts(model, X)
                correction = (out[:, rows] - glob[:, rows]).abs()
        loss = step(X, y0)
        if report:
            say(overfit_line(i, loss.item(), correction.mean().item(), correction.max().item()))
    current_state = model.state_dict()
    with torch.no_grad():
        for k, v in saved_state.items():
            current_state[k].copy_(v)
    say("=" * 60)
    say("[OverfitTest] DONE. Model weights RESTORED to initial state.")
    say("=" * 60 + "\n")


class DualTrainStep(TrainStep):
    """The standard-mode step of scripts/train_dual_mesh.py:195-229: `TrainStep` with the ROI mask as the spatial mask,
    scored AFTER `apply_special_channels` as the script scores it (`src/train.py`, and so `TrainStep`, scores before).
    After the overwrite a forcing channel equals its target and a static channel is the carried input, so neither
    carries a gradient: the step weighs them out of the fused loss (`channel_mask`), rescales the gradient by
    C_predicted / C inside Adam (the script's mean runs over all C channels) and adds the static channels' carried
    error - a constant of the batch, summed on the device by `gcl_region_eval_pair` - to the reported loss.  Without
    static or forcing channels it is `TrainStep` unchanged."""

    def __init__(self, model, lr=5e-4, use_residual: bool = False, ar_steps: int = 1, static_channels=None,
                 forcing_channels=None, use_graph=None):
        C, dev = model.n_features, model.roi_mask.device
        forcing = set(forcing_channels or [])
        special = sorted(set(static_channels or []) | forcing)
        self._ratio, self._carry_kinds, mask = 1.0, None, None
        if special:
            if len(special) >= C:
                raise ValueError("DualTrainStep: every channel is static or forcing, nothing is left to train on")
            mask = torch.ones(C, dtype=torch.float32)
            mask[special] = 0.0
            mask = mask.to(dev)
            self._ratio = (C - len(special)) / C
            kinds = torch.full((C,), 2, dtype=torch.int32)  # forcing: out = y, no error
            kinds[sorted(set(static_channels or []) - forcing)] = 1  # static: out = the window's last slot
            self._carry_kinds = kinds.to(dev)
            self._carry = torch.zeros(1, dtype=torch.float64, device=dev)
        super().__init__(model, lr=lr, channel_mask=mask, spatial_mask=model.roi_mask.view(1, -1, 1).float(),
                         use_residual=use_residual, ar_steps=ar_steps, use_graph=use_graph,
                         static_channels=static_channels, forcing_channels=forcing_channels)

    def _fwd_bwd(self, X, y, threshold=0.0, epoch=0, batch_num=1):
        loss = super()._fwd_bwd(X, y, threshold, epoch, batch_num)
        if self._carry_kinds is None:
            return loss
        C = self.model.n_features
        steps = max(min(self.ar_steps, y.shape[-1] // C), 1)
        self._carry.zero_()
        for s in range(steps):  # the static channels keep the input's value at every step of the rollout
            ys = y[:, :, s * C:(s + 1) * C]
            hip.region_eval_pair([(ys, X, None, None)], ys, self._carry_kinds, False, self.model._roi_rows, 1.0 / steps,
                                 self._carry, self.model.obs_window)
        return (loss.double() * self._ratio + self._carry[0]).float()

    def _finish(self):
        self.opt.step(grad_scale=allreduce_gradients(self.flat, self.world) * self._ratio)


def train_dual_epoch(model, dataloader, optimizer, device, lat_weights=None, use_residual: bool = False,
                     current_ar_steps: int = 1, static_channels=None, forcing_channels=None, check_grads: bool = False,
                     cache: GlobalOutputCache = None, batch_size: int = 1, say=print):
    """train_dual_mesh.py:138-255: one pass, the loss on the ROI rows only; returns the mean batch loss.

    `optimizer` is the fused step: a `DualTrainStep` in the standard mode (its AR depth is set to `current_ar_steps`,
    which drops a captured graph of another depth; residual and special channels are the step's own and must agree with the arguments),
    a `DualMeshCacheStep` when `cache` is given.  The cached mode reads nothing from `dataloader` (inputs and targets
    are in the records): it walks the cache in order, `batch_size` samples a step.  `lat_weights` is unused, as in the
    reference.  One host read at the end of the pass."""
    model.train()
    model.global_model.eval()
    step = optimizer
    dev = torch.device(device)
    if bool(step.use_residual) != bool(use_residual):
        raise ValueError(f"train_dual_epoch: use_residual={use_residual} but the step was built with {step.use_residual}")
    total = torch.zeros((), dtype=torch.float64, device=dev)
    n_batches = 0
    if cache is not None:
        if not isinstance(step, DualMeshCacheStep) or step.cache is not cache:
            raise ValueError("train_dual_epoch: the cached mode runs on a DualMeshCacheStep over that cache")
        order = torch.arange(len(cache), dtype=torch.int64, device=cache.device)
        for i in range(0, len(cache), batch_size):
            total += step(order[i:i + batch_size])  # before the next call: a replay returns the same static tensor
            if check_grads and n_batches == 0:
                if not _grad_report(model, "out_roi", say):
                    say("  WARNING: все градиенты нулевые!")
            n_batches += 1
    else:
        if (list(step.static_channels or []), list(step.forcing_channels or [])) != (list(static_channels or []),
                                                                                     list(forcing_channels or [])):
            raise ValueError("train_dual_epoch: the step's static / forcing channels differ from the arguments")
        if (static_channels or forcing_channels) and not isinstance(step, DualTrainStep):
            raise ValueError("train_dual_epoch: with static or forcing channels the standard mode needs a DualTrainStep "
                             "(a plain TrainStep scores before the overwrite, the script after)")
        for X, y in dataloader:
            X, y = _batch(X, y, dev)
            C = X.shape[-1] // model.obs_window
            step.ar_steps = min(current_ar_steps, y.shape[-1] // C)
            total += step(X, y)
            if check_grads and n_batches == 0:
                if not _grad_report(model, "out_roi", say, getattr(step, "_ratio", 1.0)):
                    say("  WARNING: все градиенты нулевые!")
            n_batches += 1
    return total.item() / max(n_batches, 1)


@torch.no_grad()
def eval_dual(model, dataloader, device, lat_weights=None, use_residual: bool = False, current_ar_steps: int = 1,
              static_channels=None, forcing_channels=None, cache: GlobalOutputCache = None, batch_size: int = 1):
    """train_dual_mesh.py:260-368: (mean ROI loss, correction skill = 1 - loss / global-only loss).

    Standard mode: the corrected and the global-only rollout advance in lock-step, one `gcl_region_eval_pair` per AR
    step (step_out, both shifted windows and both ROI losses); at step 0 the two windows are equal and share one global
    forward.  Cached mode (`cache`; nothing is read from `dataloader`): fetch, the regional module, and the same kernel
    on the compact ROI rows without window traffic.  Sums stay in a float64 device state until the end of the pass."""
    model.eval()
    dev = torch.device(device)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    n_batches = 0
    obs = model.obs_window
    if cache is not None:
        r = cache.rec
        order = torch.arange(len(cache), dtype=torch.int64, device=cache.device)
        for i in range(0, len(cache), batch_size):
            roi3, send3, pred3, y3 = cache.fetch(order[i:i + batch_size])
            glob = pred3[..., :r.C]
            out = hip.roi_compose(glob, model._regional(roi3, send3), model._roi_ident)
            hip.region_eval_pair([(out, roi3, None, None), (glob, roi3, None, None)], y3[..., :r.C], None, use_residual,
                                 None, 1.0, acc, obs)
            n_batches += 1
    else:
        rows = model._roi_rows
        for X, y in dataloader:
            X, y = _batch(X, y, dev)
            N, G, _ = X.shape
            C = X.shape[-1] // obs
            steps = max(min(current_ar_steps, y.shape[-1] // C), 1)
            kinds = _channel_kinds(C, static_channels, forcing_channels, dev) if (static_channels or forcing_channels) else None
            corr_win = glob_win = X
            for s in range(steps):
                if s == 0:
                    glob, out = _dual_parts(model, X)
                else:
                    out = _dual_parts(model, corr_win)[1]
                    glob = model._global(glob_win, 0.0)[0]
                more = s + 1 < steps
                new_c = torch.empty(N, G, obs, C, dtype=torch.float32, device=dev) if more else None
                new_g = torch.empty(N, G, obs, C, dtype=torch.float32, device=dev) if more else None
                hip.region_eval_pair([(out, corr_win, new_c, None), (glob, glob_win, new_g, None)],
                                     y[:, :, s * C:(s + 1) * C], kinds, use_residual, rows, 1.0 / steps, acc, obs)
                if more:
                    corr_win, glob_win = new_c.view(N, G, obs * C), new_g.view(N, G, obs * C)
            n_batches += 1
    total_loss, total_global_loss = acc.cpu().tolist()  # the one host read of the pass
    avg_loss = total_loss / max(n_batches, 1)
    avg_global_loss = total_global_loss / max(n_batches, 1)
    correction_skill = 1.0 - avg_loss / avg_global_loss if avg_global_loss > 0 else 0.0
    return avg_loss, correction_skill


def fit_loop(model, run_train, run_eval, results_dir, num_epochs: int, header: str, rule: str, line, own_file: str,
             log=None):
    """The epoch loop both scripts share (train_dual_mesh.py:583-626, train_roi_residual.py:319-343): header and rule,
    per epoch `run_train(epoch)` and `run_eval()` -> (val_loss, second score), `best_model.pth` plus `own_file` (the
    state without `global_model.` keys) at every new best, one `line(epoch, train_loss, val_loss, score, best, mark)`,
    patience 10.  Returns the best validation loss."""
    log = log or _file_log(results_dir)
    log(header)
    log(rule)
    best_val_loss, patience = float("inf"), 0
    for epoch in range(num_epochs):
        train_loss = run_train(epoch)
        val_loss, score = run_eval()
        improved = ""
        if val_loss < best_val_loss:
            best_val_loss, patience = val_loss, 0
            torch.save(_own_state(model), os.path.join(results_dir, own_file))
            torch.save(model.state_dict(), os.path.join(results_dir, "best_model.pth"))
            improved = " *"
        else:
            patience += 1
        log(line(epoch, train_loss, val_loss, score, best_val_loss, improved))
        if patience >= MAX_PATIENCE:
            log(f"Early stopping at epoch {epoch + 1}")
            break
    best_ckpt = os.path.join(results_dir, "best_model.pth")
    if os.path.exists(best_ckpt):
        model.load_state_dict(torch.load(best_ckpt, map_location=model.roi_mask.device, weights_only=True))
    return best_val_loss


def _file_log(results_dir):
    log_path = os.path.join(results_dir, "training_log.txt")

    def _log(msg):
        print(msg)
        with open(log_path, "a", encoding="utf-8") as f:
            f.write(msg + "\n")

    return _log


DUAL_HEADER = f"{'epoch':>5}  {'train_loss':>10}  {'val_loss':>10}  {'corr_skill':>10}  {'best':>10}"
ROI_HEADER = f"{'epoch':>5}  {'train_loss':>10}  {'val_loss':>10}  {'val_ACC':>8}  {'best':>10}"


def ar_line(ar_steps):
    """train_dual_mesh.py:582."""
    return f"[AR] training/eval horizon = {ar_steps} step(s) (+{ar_steps * 6}h)"


def dual_test_line(test_loss, test_skill):
    """train_dual_mesh.py:641."""
    return f"\n[TEST] loss={test_loss:.6f}  correction_skill={test_skill:.2%}"


def roi_test_line(test_loss, test_acc):
    """train_roi_residual.py:350."""
    return f"\n[TEST] loss={test_loss:.6f}  regional_ACC={test_acc:.4f}"


def overfit_line(step, loss, mean_abs, max_abs):
    """train_dual_mesh.py:123-125."""
    return f"    step {step:3d}: loss={loss:.6f}  |correction|={mean_abs:.6f}  max={max_abs:.4f}"


def correction_line(mean_abs, max_abs, baseline_mse):
    """train_roi_residual.py:153-157."""
    return f"  [Correction] mean_abs={mean_abs:.6f}, max_abs={max_abs:.4f}, baseline_mse={baseline_mse:.6f}"


def dual_line(epoch, train_loss, val_loss, correction_skill, best_val_loss, improved):
    """train_dual_mesh.py:622."""
    return f"{epoch + 1:5d}  {train_loss:10.6f}  {val_loss:10.6f}  {correction_skill:>9.2%}  {best_val_loss:10.6f}{improved}"


def roi_line(epoch, train_loss, val_loss, val_acc, best_val_loss, improved):
    """train_roi_residual.py:340."""
    return f"{epoch + 1:5d}  {train_loss:10.6f}  {val_loss:10.6f}  {val_acc:8.4f}  {best_val_loss:10.6f}{improved}"


def fit_dual_mesh(model, train_loader, val_loader, test_loader, results_dir, num_epochs: int, lr: float = 5e-4,
                  ar_steps: int = 1, use_residual: bool = False, static_channels=None, forcing_channels=None,
                  precompute: bool = False, overfit: bool = True, reg_mesh_level=None, use_graph=None, batch_size: int = 1):
    """train_dual_mesh.py:528-656 after the model is built: overfit test, optional precompute, the epoch loop with its
    log, `best_regional.pth` (no `global_model.` key) and `best_model.pth`, patience 10, the `[TEST]` line and
    `results.json`.  `precompute` forces `ar_steps = 1` (:436-440).  Returns the results dictionary."""
    device = model.roi_mask.device
    os.makedirs(results_dir, exist_ok=True)
    log = _file_log(results_dir)
    if precompute and ar_steps != 1:
        print(f"WARNING: --precompute requires --ar-steps 1, got {ar_steps}. Forcing ar_steps=1.")
        ar_steps = 1
    if overfit:
        overfit_test(model, train_loader, device, use_residual=use_residual)
    train_cache = val_cache = None
    if precompute:
        print("\n" + "=" * 60)
        print("[Precompute] Caching global model outputs...")
        print("=" * 60)
        model.eval()
        train_cache = GlobalOutputCache.build(model, train_loader, "train")
        val_cache = GlobalOutputCache.build(model, val_loader, "val")
        print("[Precompute] Done. Training will skip global model from now on.\n")
        step = DualMeshCacheStep(model, train_cache, lr=lr, use_residual=use_residual, use_graph=use_graph)
    else:
        step = DualTrainStep(model, lr=lr, use_residual=use_residual, ar_steps=ar_steps, use_graph=use_graph,
                             static_channels=static_channels, forcing_channels=forcing_channels)
    kw = dict(use_residual=use_residual, current_ar_steps=ar_steps, static_channels=static_channels,
              forcing_channels=forcing_channels)
    log(ar_line(ar_steps))
    best_val_loss = fit_loop(
        model, lambda epoch: train_dual_epoch(model, train_loader, step, device, check_grads=(epoch == 0),
                                              cache=train_cache, batch_size=batch_size, **kw),
        lambda: eval_dual(model, val_loader, device, cache=val_cache, batch_size=batch_size, **kw),
        results_dir, num_epochs, DUAL_HEADER, "-" * 59, dual_line, "best_regional.pth", log=log)
    test_loss, test_skill = eval_dual(model, test_loader, device, **kw)
    log(dual_test_line(test_loss, test_skill))
    results = {
        "best_val_loss": best_val_loss,
        "test_loss": test_loss,
        "test_correction_skill": test_skill,
        "roi": list(model.roi),
        "reg_mesh_level": reg_mesh_level,
        "reg_steps": model.reg_processor.num_steps,
        "cross_k": model._cross.half // max(model.n_reg_mesh, 1),
        "hidden_dim": model.reg_encoder.mlp[0].weight.shape[0],
        "ar_steps": ar_steps,
    }
    with open(os.path.join(results_dir, "results.json"), "w") as fh:
        json.dump(results, fh, indent=2)
    log(f"Results saved to {results_dir}")
    return results


# ------------------------------------------------------------------------------------------------------------------
# scripts/train_roi_residual.py
# ------------------------------------------------------------------------------------------------------------------
def train_roi_epoch(model, dataloader, optimizer, device, check_grads: bool = False, say=print):
    """train_roi_residual.py:91-159 (`train_epoch` there): one pass on `optimizer`, a
    `TrainStep(model, spatial_mask=roi_mask, use_residual=False)`; the `[Correction]` line comes from the last batch's
    forward before its update, as in the reference.  Returns the mean batch loss."""
    model.train()
    model.global_model.eval()
    step, dev = optimizer, torch.device(device)
    rows = model._roi_rows.long()
    total = torch.zeros((), dtype=torch.float64, device=dev)
    n_batches = 0
    it = iter(dataloader)
    nxt = next(it, None)
    correction = baseline = None
    while nxt is not None:
        X, y = _batch(*nxt, dev)
        nxt = next(it, None)
        C = X.shape[-1] // model.obs_window
        y0 = y[:, :, :C]
        if nxt is None:
            with torch.no_grad():
                glob, out = _parts(model, X)
                correction = (out[:, rows] - glob[:, rows]).abs()
                baseline = torch.zeros(1, dtype=torch.float64, device=dev)
                hip.region_eval_pair([(glob, X, None, None)], y0, None, False, model._roi_rows, 1.0, baseline,
                                     model.obs_window)
        total += step(X, y0)
        if check_grads and n_batches == 0:
            _grad_report(model, "out", say)
        n_batches += 1
    if n_batches > 0:
        say(correction_line(correction.mean().item(), correction.max().item(), baseline.item()))
    return total.item() / max(n_batches, 1)


@torch.no_grad()
def eval_roi_epoch(model, dataloader, device):
    """train_roi_residual.py:162-192 (`eval_epoch` there): (mean ROI loss, mean ROI ACC).  The loss through
    `gcl_region_eval_pair`, the ACC (`spatial_corr` over the ROI rows) through `gcl_roi_gather_rows` into [B, n_roi, C]
    and the evaluator's `gcl_eval_colstats` / `gcl_eval_accumulate`; one host read at the end."""
    model.eval()
    dev = torch.device(device)
    rows, n = model._roi_rows, model.n_roi_grid
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    state = torch.zeros(4, dtype=torch.float64, device=dev)
    n_batches = 0
    for X, y in dataloader:
        X, y = _batch(X, y, dev)
        B, G, _ = X.shape
        C = X.shape[-1] // model.obs_window
        y0 = y[:, :, :C]
        out = _parts(model, X)[1]
        hip.region_eval_pair([(out, X, None, None)], y0, None, False, rows, 1.0, loss, model.obs_window)
        o_roi = hip.roi_gather_rows(rows, G, [out], _pad4(C), B)[..., :C]
        y_roi = hip.roi_gather_rows(rows, G, [y0], _pad4(C), B)[..., :C]
        stats = torch.empty(B, C, hip.EVAL_NS, dtype=torch.float64, device=dev)
        hip.eval_colstats(o_roi, o_roi, y_roi, None, None, False, stats)
        hip.eval_accumulate(stats, None, None, 1.0 / (B * n * C), n, state)
        n_batches += 1
    return loss.item() / max(n_batches, 1), state[1].item() / max(n_batches, 1)


def fit_roi_residual(model, train_loader, val_loader, test_loader, results_dir, num_epochs: int, lr: float = 1e-3,
                     overfit: bool = True, use_graph=None, extra: dict = None):
    """train_roi_residual.py:303-367 after the model is built: overfit test, the epoch loop with its log,
    `best_head.pth` and `best_model.pth`, patience 10, the `[TEST]` line and `results.json` (`extra`: the driver's
    `pretrained` and `data_dir` entries)."""
    device = model.roi_mask.device
    os.makedirs(results_dir, exist_ok=True)
    log = _file_log(results_dir)
    if overfit:
        overfit_test(model, train_loader, device, use_residual=False)
    step = TrainStep(model, lr=lr, spatial_mask=model.roi_mask.view(1, -1, 1).float(), use_residual=False,
                     use_graph=use_graph)
    best_val_loss = fit_loop(
        model, lambda epoch: train_roi_epoch(model, train_loader, step, device, check_grads=(epoch == 0)),
        lambda: eval_roi_epoch(model, val_loader, device), results_dir, num_epochs, ROI_HEADER, "-" * 55, roi_line,
        "best_head.pth", log=log)
    test_loss, test_acc = eval_roi_epoch(model, test_loader, device)
    log(roi_test_line(test_loss, test_acc))
    results = {
        "best_val_loss": best_val_loss,
        "test_loss": test_loss,
        "test_regional_acc": test_acc,
        "roi": list(model.roi),
        "hidden_dim": model.input_proj[0].weight.shape[0],
        "processor_steps": len(model.processor.steps),
        "roi_k": int(model.roi_edge_index.shape[1] // max(model.n_roi_grid, 1)),
        "lr": lr,
        "pretrained": (extra or {}).get("pretrained"),
        "data_dir": (extra or {}).get("data_dir"),
    }
    with open(os.path.join(results_dir, "results.json"), "w") as fh:
        json.dump(results, fh, indent=2)
    log(f"Results saved to {results_dir}")
    return results


# ------------------------------------------------------------------------------------------------------------------
# scripts/predict_dual_mesh.py
# ------------------------------------------------------------------------------------------------------------------
UNITS = {  # predict_dual_mesh.py:37-45
    "t2m": "K", "10u": "m/s", "10v": "m/s", "msl": "Pa",
    "tp": "m", "sp": "Pa", "tcwv": "kg/m²",
    "z_surf": "m²/s²", "lsm": "-",
    "t@850": "K", "u@850": "m/s", "v@850": "m/s",
    "z@850": "m²/s²", "q@850": "kg/kg",
    "t@500": "K", "u@500": "m/s", "v@500": "m/s",
    "z@500": "m²/s²", "q@500": "kg/kg",
}
KEY_VARS = ["t2m", "10u", "10v", "msl", "z@500", "t@850", "u@850", "v@850", "z@850"]  # predict_dual_mesh.py:324


class RegionScores:
    """A host snapshot of one `StreamingMetrics` object: what the tables of predict_dual_mesh.py (and, with `mse`, of
    predict.py) read from it."""

    def __init__(self, n, rmse, mae, acc, rmse_per_channel, acc_per_channel, mse=None):
        self.n, self.rmse, self.mae, self.acc = int(n), float(rmse), float(mae), float(acc)
        self.mse = float(rmse) ** 2 if mse is None else float(mse)
        self.rmse_per_channel = np.asarray(rmse_per_channel, dtype=np.float64)
        self.acc_per_channel = np.asarray(acc_per_channel, dtype=np.float64)

    @classmethod
    def of(cls, sm):
        return cls(sm.n, sm.rmse, sm.mae, sm.acc, sm.rmse_per_channel, sm.acc_per_channel, mse=sm.mse)


class PredictResults(dict):
    """The dictionary written to `predict_results.json` (predict_dual_mesh.py:407-432) plus, as attributes, what
    `regional_tables` prints from: `overall` = (prediction, persistence) `RegionScores`, `horizons` = one such pair per
    horizon, `G`, `C`, `n_roi`."""

    overall = horizons = None
    G = C = n_roi = 0


def _horizon_label(p):
    return f" {'+' + str((p + 1) * 6) + 'h':>8s}"


def regional_tables(results: PredictResults, variables=None, std=None, say=print):
    """predict_dual_mesh.py:286-404: the inference summary and the per-horizon lines; with `variables` (`--per-channel`)
    also the three per-horizon per-channel tables of the key variables (more than one horizon and `std` given) and the
    overall per-channel table (`std` given).  `std`: the data set's per-channel standard deviations."""
    sp_all, sb_all = results.overall
    AR, C = results["ar_steps"], results.C
    skill_region = 1.0 - sp_all.rmse / (sb_all.rmse + 1e-12)
    say("")
    say("=" * 60)
    say(f"=== Inference summary ({sp_all.n} samples, AR={AR}) ===")
    say(f"Grid: G={results.G} | C={C} | ROI={results.n_roi} points")
    say("")
    say(f"  REGIONAL overall (avg across {AR} horizons):")
    say(f"    RMSE={sp_all.rmse:.6f} | MAE={sp_all.mae:.6f}")
    say(f"    Baseline RMSE={sb_all.rmse:.6f}")
    say(f"    Skill={skill_region * 100:.2f}%")
    say(f"    ACC={sp_all.acc:.4f} | base ACC={sb_all.acc:.4f}")
    say("\n  Per-horizon (regional):")
    for p, (sp, sb) in enumerate(results.horizons):
        if sp.n == 0:
            continue
        sk = 1.0 - sp.rmse / (sb.rmse + 1e-12)
        say(f"    +{(p + 1) * 6:02d}h: RMSE={sp.rmse:.6f} | base={sb.rmse:.6f} | skill={sk * 100:.2f}% | ACC={sp.acc:.4f} "
            f"(base {sb.acc:.4f})")
    say("=" * 60)
    if variables is None:
        return
    var_order = list(variables)
    if std is not None:
        std = np.asarray(std, dtype=np.float64)[:C]
    if AR > 1 and std is not None:
        key_idx = [i for i, v in enumerate(var_order[:C]) if v in KEY_VARS]
        say("\nPer-horizon per-channel RMSE (physical units, regional):")
        say(f"  {'var':>10s} {'unit':>6s}" + "".join(_horizon_label(p) for p in range(AR)))
        for c in key_idx:
            name = var_order[c]
            row = f"  {name:>10s} {UNITS.get(name, '?'):>6s}"
            for sp, _ in results.horizons:
                if sp.n == 0:
                    row += f" {'N/A':>8s}"
                    continue
                phys_rmse = sp.rmse_per_channel[c] * std[c]
                if "z@" in name or name == "z_surf":
                    row += f" {phys_rmse / 9.81:7.1f}m"
                elif name == "t2m" or name.startswith("t@"):
                    row += f" {phys_rmse:6.2f}°C"
                else:
                    row += f" {phys_rmse:8.4f}"
            say(row)
        say("\nPer-horizon per-channel ACC (regional):")
        say(f"  {'var':>10s}" + "".join(_horizon_label(p) for p in range(AR)))
        for c in key_idx:
            row = f"  {var_order[c]:>10s}"
            for sp, _ in results.horizons:
                row += f" {'N/A':>8s}" if sp.n == 0 else f" {sp.acc_per_channel[c]:8.4f}"
            say(row)
        say("\nPer-horizon per-channel Skill (regional):")
        say(f"  {'var':>10s}" + "".join(_horizon_label(p) for p in range(AR)))
        for c in key_idx:
            row = f"  {var_order[c]:>10s}"
            for sp, sb in results.horizons:
                if sp.n == 0:
                    row += f" {'N/A':>8s}"
                    continue
                sk_c = (1 - sp.rmse_per_channel[c] / (sb.rmse_per_channel[c] + 1e-12)) * 100
                row += f" {sk_c:7.2f}%"
            say(row)
    if std is not None:
        say(f"\nPer-channel overall (physical units, avg over {AR} horizons):")
        say(f"  {'#':>3s} {'var':>10s} {'unit':>8s}  {'ACC':>8s}  {'RMSE':>10s} {'RMSE_base':>10s} {'Skill':>7s}")
        for c, name in enumerate(var_order[:C]):
            unit = UNITS.get(name, "?")
            phys_rg = sp_all.rmse_per_channel[c] * std[c]
            phys_bl = sb_all.rmse_per_channel[c] * std[c]
            sk_c = (1 - phys_rg / (phys_bl + 1e-12)) * 100
            extra = ""
            if "z@" in name or name == "z_surf":
                extra = f"  ({phys_rg / 9.81:.1f} gpm)"
            elif name == "t2m" or name.startswith("t@"):
                extra = f"  ({phys_rg:.2f} °C)"
            say(f"  {c:3d} {name:>10s} {unit:>8s}  {sp_all.acc_per_channel[c]:8.4f}  {phys_rg:10.4f} {phys_bl:10.4f} "
                f"{sk_c:6.2f}%{extra}")


def predict_results(overall, horizons, ar_steps: int, roi, G: int, C: int, n_roi: int, variables=None) -> PredictResults:
    """The results of predict_dual_mesh.py:407-432 from (prediction, persistence) `RegionScores` pairs."""
    sp_all, sb_all = overall
    res = PredictResults({
        "n_samples": sp_all.n,
        "ar_steps": ar_steps,
        "roi": list(roi),
        "regional_overall": {"rmse": sp_all.rmse, "mae": sp_all.mae, "acc": sp_all.acc, "baseline_rmse": sb_all.rmse,
                             "skill": 1.0 - sp_all.rmse / (sb_all.rmse + 1e-12)},
        "per_horizon": [],
    })
    for p, (sp, sb) in enumerate(horizons):
        if sp.n == 0:
            continue
        res["per_horizon"].append({"horizon_h": (p + 1) * 6, "rmse": sp.rmse, "acc": sp.acc, "baseline_rmse": sb.rmse,
                                   "skill": 1.0 - sp.rmse / (sb.rmse + 1e-12)})
    if variables is not None:
        res["per_channel"] = {"variables": list(variables)[:C], "regional_rmse_norm": sp_all.rmse_per_channel.tolist(),
                              "regional_acc": sp_all.acc_per_channel.tolist()}
    res.overall, res.horizons, res.G, res.C, res.n_roi = overall, list(horizons), G, C, n_roi
    return res


@torch.no_grad()
def predict_dual_mesh(model, dataset, max_samples: int = 200, ar_steps: int = 1, use_residual: bool = True,
                      per_channel: bool = False, variables=None, std=None, results_path=None, say=print):
    """predict_dual_mesh.py:203-438: the autoregressive rollout of the dual model over the first `max_samples` samples
    of `dataset` (an iterable of (X, y), one sample each), scored on the ROI rows against persistence.  Rollout:
    `predict.rollout` on the device; scores: one `verify.ForecastVerifier(region_idxs=roi)`, whose regional objects are
    the script's overall pair and its pair per horizon (all horizons of a sample in one update, no host read until the
    end apart from the progress line every 50 samples).  Prints the script's tables (`regional_tables`; the per-channel
    ones with `per_channel`, `variables` and `std`) and writes `results_path` when given.  Returns `PredictResults`."""
    from .predict import rollout
    from .verify import ForecastVerifier, Persistence

    dev = model.roi_mask.device
    C, G, n_roi = model.n_features, int(model.roi_mask.numel()), model.n_roi_grid
    n_total = len(dataset) if hasattr(dataset, "__len__") else None
    if n_total is not None:
        max_samples = min(max_samples, n_total)
    say(f"\n[predict] {max_samples}/{n_total} test samples, ROI={n_roi} points")
    say(f"  use_residual={use_residual}, C={C}, G={G}, AR={ar_steps} steps (+{ar_steps * 6}h)")
    ver = ForecastVerifier(C, ar_steps, region_idxs=model._roi_rows.cpu().numpy(), device=dev)
    sm_region, sm_base = ver.region["pred"], ver.region["base"]
    model.eval()
    for i, (X, y) in enumerate(dataset):
        if i >= max_samples:
            break
        X, y = _batch(X, y, dev)
        P = min(ar_steps, y.shape[-1] // C)
        if P != ar_steps and ar_steps > 1 and P == 1:
            raise ValueError(f"predict_dual_mesh: the targets hold one step, ar_steps={ar_steps} (load the data set with "
                             f"pred_steps=ar_steps, as the script does)")
        outs = rollout(model, X, P, use_residual=use_residual)
        ver.update(y[:, :, :P * C], pred=outs, base=Persistence(X, C))
        if (i + 1) % 50 == 0:
            sk_r = 1.0 - sm_region.rmse / (sm_base.rmse + 1e-12)
            say(f"  [{i + 1}/{max_samples}] region RMSE={sm_region.rmse:.6f} ACC={sm_region.acc:.4f} skill={sk_r * 100:.2f}%")
    if ar_steps > 1:
        pairs = list(zip(ver.region_horizon["pred"], ver.region_horizon["base"]))
    else:
        pairs = [(sm_region, sm_base)]  # one horizon: its objects are the overall ones
    horizons = [(RegionScores.of(a), RegionScores.of(b)) for a, b in pairs]
    overall = (RegionScores.of(sm_region), RegionScores.of(sm_base))
    for o in overall:  # the script updates the overall objects once per horizon: its sample count is theirs summed
        o.n = sum(h[0].n for h in horizons)
    res = predict_results(overall, horizons, ar_steps, model.roi, G, C, n_roi, variables if per_channel else None)
    regional_tables(res, variables if per_channel else None, std, say=say)
    if results_path is not None:
        os.makedirs(os.path.dirname(os.path.abspath(results_path)), exist_ok=True)
        with open(results_path, "w") as fh:
            json.dump(res, fh, indent=2)
        say(f"\nSaved to {results_path}")
    return res


# ------------------------------------------------------------------------------------------------------------------
# Command line
# ------------------------------------------------------------------------------------------------------------------
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m graphcast_lite_amd.regional_train")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p, lr):
        p.add_argument("experiment_dir")
        p.add_argument("--pretrained", required=True)
        p.add_argument("--data-dir", default=None)
        p.add_argument("--epochs", type=int, default=None)
        p.add_argument("--lr", type=float, default=lr)
        p.add_argument("--hidden-dim", type=int, default=256)
        p.add_argument("--roi", nargs=4, type=float, required=True, metavar=("LAT_MIN", "LAT_MAX", "LON_MIN", "LON_MAX"))
        p.add_argument("--overfit-only", action="store_true")

    d = sub.add_parser("dual", help="scripts/train_dual_mesh.py")
    common(d, 5e-4)
    d.add_argument("--freeze-global", action="store_true", default=True)  # always on, as in the script
    d.add_argument("--reg-mesh-level", type=int, default=7)
    d.add_argument("--reg-steps", type=int, default=4)
    d.add_argument("--cross-k", type=int, default=3)
    d.add_argument("--reg-buffer", type=float, default=2.0)
    d.add_argument("--resume", action="store_true")  # the script parses it and never reads it: refused here
    d.add_argument("--batch-size", type=int, default=None)
    d.add_argument("--ar-steps", type=int, default=None)
    d.add_argument("--precompute", action="store_true")
    d.add_argument("--subsample", type=int, default=1)
    r = sub.add_parser("roi", help="scripts/train_roi_residual.py")
    common(r, 1e-3)
    r.add_argument("--processor-steps", type=int, default=6)
    r.add_argument("--roi-k", type=int, default=8)
    r.add_argument("--batch-size", type=int, default=1)
    q = sub.add_parser("predict", help="scripts/predict_dual_mesh.py")
    q.add_argument("experiment_dir")
    q.add_argument("--pretrained", required=True)
    q.add_argument("--regional-ckpt", default=None)
    q.add_argument("--data-dir", default=None)
    q.add_argument("--roi", nargs=4, type=float, required=True, metavar=("LAT_MIN", "LAT_MAX", "LON_MIN", "LON_MAX"))
    q.add_argument("--max-samples", type=int, default=200)
    q.add_argument("--reg-mesh-level", type=int, default=7)
    q.add_argument("--reg-steps", type=int, default=4)
    q.add_argument("--cross-k", type=int, default=3)
    q.add_argument("--hidden-dim", type=int, default=256)
    q.add_argument("--no-residual", action="store_true")
    q.add_argument("--per-channel", action="store_true")
    q.add_argument("--ar-steps", type=int, default=1)
    return ap


def resolve_dual_args(args, exp_cfg):
    """The argument rules of train_dual_mesh.py:419-450: (ar_steps the datasets are loaded with, ar_steps trained,
    train shuffle).  The horizon defaults to max(max_ar_steps, pred_window_used); `--precompute` forces one step and
    turns shuffling off (the cache is walked in order)."""
    loaded = args.ar_steps or max(getattr(exp_cfg, "max_ar_steps", 1), getattr(exp_cfg.data, "pred_window_used", 1))
    ar_steps = loaded
    if args.precompute and ar_steps != 1:
        print(f"WARNING: --precompute requires --ar-steps 1, got {ar_steps}. Forcing ar_steps=1.")
        ar_steps = 1
    return loaded, ar_steps, not args.precompute


class _Every:
    """Every `k`-th sample of a device dataset (`--subsample`, train_dual_mesh.py:429-433)."""

    def __init__(self, ds, k):
        self.ds, self.idx = ds, list(range(0, len(ds), k))

    def __len__(self):
        return len(self.idx)

    def batch_shapes(self, B):
        return self.ds.batch_shapes(B)

    def batch(self, indices, out=None):
        return self.ds.batch([self.idx[i] for i in indices], out=out)


def main(argv=None, device=None, use_graph=None):
    """`python -m graphcast_lite_amd.regional_train {dual,roi,predict} <experiment_dir> --pretrained p --roi a b c d ...`
    with the options of the three scripts; returns the results dictionary (None after `--overfit-only`)."""
    from .config import ExperimentConfig
    from .data import DeviceLoader, load_chunked_datasets
    from .main import load_model_from_experiment_config, set_random_seeds
    from .utils import load_from_json_file

    args = build_parser().parse_args(sys.argv[1:] if argv is None else argv)
    if args.command == "dual" and args.resume:
        raise SystemExit("--resume: the script parses this flag and never reads it; there is no checkpoint to resume from")
    cfg_path = os.path.join(args.experiment_dir, FileNames.EXPERIMENT_CONFIG)
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"Config not found: {cfg_path}")
    results_dir = os.path.join(args.experiment_dir, "results")
    os.makedirs(results_dir, exist_ok=True)
    exp_cfg = ExperimentConfig(**load_from_json_file(cfg_path))
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("regional_train needs a GPU (the HIP path has no CPU fallback)")
        device = "cuda:0"
    device = torch.device(device)
    print(f"Device: {device}")
    set_random_seeds(42)
    dual = args.command in ("dual", "predict")
    predict = args.command == "predict"
    data_dir = args.data_dir or getattr(exp_cfg, "data_dir", None)
    if data_dir is None:
        if not dual:
            raise ValueError("data_dir must be provided either in config or via --data-dir")
        data_dir = f"data/datasets/{getattr(exp_cfg.data.dataset_name, 'value', exp_cfg.data.dataset_name)}"
    if predict:
        loaded, ar_steps, shuffle = args.ar_steps, args.ar_steps, False
    else:
        loaded, ar_steps, shuffle = resolve_dual_args(args, exp_cfg) if dual else (1, 1, True)
    train_ds, val_ds, test_ds, meta = load_chunked_datasets(
        data_path=data_dir, obs_window=exp_cfg.data.obs_window_used, pred_steps=loaded,
        n_features=exp_cfg.data.num_features_used, device=device)
    if args.command == "dual" and args.subsample > 1:
        train_ds, val_ds = _Every(train_ds, args.subsample), _Every(val_ds, args.subsample)
        print(f"[Subsample] every {args.subsample}th sample: train={len(train_ds)}, val={len(val_ds)}")
    batch_size = 1 if predict else (args.batch_size or exp_cfg.batch_size)
    train_loader = DeviceLoader(train_ds, batch_size=batch_size, shuffle=shuffle)
    val_loader = DeviceLoader(val_ds, batch_size=batch_size, shuffle=False)
    test_loader = DeviceLoader(test_ds, batch_size=batch_size, shuffle=False)

    real_coords = getattr(meta, "cordinates", None)
    flat_grid = getattr(meta, "flat_grid", False)
    global_model = load_model_from_experiment_config(exp_cfg, device, meta, coordinates=real_coords, flat_grid=flat_grid)
    if not predict:
        print(f"\n>>> Loading pretrained global weights: {args.pretrained}")
    state = torch.load(args.pretrained, map_location=device, weights_only=True)
    missing, unexpected = global_model.load_state_dict(state, strict=False)
    if missing and not predict:
        print(f"  Missing keys ({len(missing)}): {missing[:5]}...")
    if unexpected and not predict:
        print(f"  Unexpected keys ({len(unexpected)}): {unexpected[:5]}...")
    global_model = global_model.to(device)
    if not predict:
        print("[DualTrain] Global model FROZEN." if dual else "[ROIResidualTrain] Global model FROZEN.")
    if flat_grid and real_coords is not None:
        grid_lats, grid_lons = real_coords[0].astype(np.float32), real_coords[1].astype(np.float32)
    else:
        lats = np.linspace(-90, 90, meta.num_latitudes, endpoint=True)
        lons = np.linspace(0, 360, meta.num_longitudes, endpoint=False)
        lon_grid, lat_grid = np.meshgrid(lons, lats)
        grid_lats, grid_lons = lat_grid.flatten().astype(np.float32), lon_grid.flatten().astype(np.float32)
    roi = tuple(args.roi)
    if predict:
        from .dual_mesh import DualMeshModel

        model = DualMeshModel(global_model=global_model, roi=roi, grid_lats=grid_lats, grid_lons=grid_lons, device=device,
                              reg_mesh_level=args.reg_mesh_level, reg_processor_steps=args.reg_steps, cross_k=args.cross_k,
                              hidden_dim=args.hidden_dim)
        ckpt_path = args.regional_ckpt or os.path.join(args.experiment_dir, "results", "best_regional.pth")
        if os.path.exists(ckpt_path):
            reg_state = torch.load(ckpt_path, map_location=device, weights_only=True)
            _, unexpected = model.load_state_dict(reg_state, strict=False)
            print(f"Loaded {len(reg_state) - len(unexpected)} regional weight tensors from {ckpt_path}")
        else:
            print(f"WARNING: Regional checkpoint not found: {ckpt_path}")
        variables = std = None
        if args.per_channel:
            var_path, scalers_path = os.path.join(data_dir, "variables.json"), os.path.join(data_dir, "scalers.npz")
            C = exp_cfg.data.num_features_used
            variables = json.load(open(var_path)) if os.path.exists(var_path) else [f"ch{c}" for c in range(C)]
            if os.path.exists(scalers_path):
                std = np.load(scalers_path)["std"].astype(np.float64)[:C]
        return predict_dual_mesh(model, test_loader, max_samples=args.max_samples, ar_steps=args.ar_steps,
                                 use_residual=not args.no_residual and getattr(exp_cfg, "use_residual", True),
                                 per_channel=args.per_channel, variables=variables, std=std,
                                 results_path=os.path.join(results_dir, "predict_results.json"))
    print(f"\n>>> ROI: {roi}")
    num_epochs = args.epochs or exp_cfg.num_epochs
    if args.command == "dual":
        from .dual_mesh import DualMeshModel

        model = DualMeshModel(global_model=global_model, roi=roi, grid_lats=grid_lats, grid_lons=grid_lons, device=device,
                              reg_mesh_level=args.reg_mesh_level, reg_mesh_buffer=args.reg_buffer,
                              reg_processor_steps=args.reg_steps, cross_k=args.cross_k, hidden_dim=args.hidden_dim)
        n_params = sum(p.numel() for n, p in model.named_parameters() if not n.startswith("global_model.") and p.requires_grad)
        print(f"\n[Optimizer] {n_params:,} trainable regional parameters, lr={args.lr}")
        use_residual = getattr(exp_cfg, "use_residual", False)
        if args.overfit_only:
            overfit_test(model, train_loader, device, use_residual=use_residual)
            print("\n[--overfit-only] Done. Exiting without full training.")
            return None
        return fit_dual_mesh(model, train_loader, val_loader, test_loader, results_dir, num_epochs, lr=args.lr,
                             ar_steps=ar_steps, use_residual=use_residual,
                             static_channels=getattr(exp_cfg, "static_channels", []),
                             forcing_channels=getattr(exp_cfg, "forcing_channels", []), precompute=args.precompute,
                             reg_mesh_level=args.reg_mesh_level, use_graph=use_graph,
                             batch_size=batch_size if args.precompute else 1)
    from .roi_residual import ROIResidualModel

    model = ROIResidualModel(global_model=global_model, roi=roi, grid_lats=grid_lats, grid_lons=grid_lons, device=device,
                             hidden_dim=args.hidden_dim, processor_steps=args.processor_steps, roi_k=args.roi_k)
    n_params = sum(p.numel() for n, p in model.named_parameters() if not n.startswith("global_model.") and p.requires_grad)
    print(f"\n[Optimizer] {n_params:,} trainable ROI parameters, lr={args.lr}")
    if args.overfit_only:
        overfit_test(model, train_loader, device)
        print("\n[--overfit-only] Done. Exiting without full training.")
        return None
    return fit_roi_residual(model, train_loader, val_loader, test_loader, results_dir, num_epochs, lr=args.lr,
                            use_graph=use_graph, extra={"pretrained": args.pretrained, "data_dir": data_dir})


if __name__ == "__main__":
    main()
