"""Autoregressive rollout / inference caller of the hot path.

Mirrors the AR branch of the reference's inference script (`scripts/predict.py:499-538`; the same
steps appear in the training loop, `src/train.py:203-228`): the one-step model predicts a delta,
the residual is added, static channels are carried forward from the last input step, forcing
channels are taken from the known future (`y`), the step is stored and the observation window is
shifted.  Here the whole per-step glue is one kernel (`gcl_ar_advance`) and the window never
leaves the device.
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
