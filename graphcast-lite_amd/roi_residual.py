"""Module API of the reference's `src/roi_residual.py`, executed by hand-written gfx950 kernels.

A frozen, pretrained `WeatherPrediction` and a small trainable correction on the grid points inside a lat/lon box:

  build_roi_knn_graph  src/roi_residual.py:15-59    k-nearest-neighbour graph over the ROI points (host, once)
  ROIResidualHead      src/roi_residual.py:62-79    `mlp.{0,2,4}.*` (Linear, SiLU, Linear, SiLU, Linear)
  ROIResidualModel     src/roi_residual.py:82-185   `input_proj.{0,2}.*`, `processor.*` (InteractionNetProcessor),
                                                    `decoder.mlp.*`, the `roi_*` buffers, `global_model.*`

How the forward runs on the HIP path ("ROI residual head"):
  * the global model runs ONCE under no_grad through `forward_with_latents`, which returns the prediction and the
    encoder's grid latents together (the reference runs the global forward and then the encoder a second time,
    :161-164,151-156; the encoder is deterministic, so both give the same latents);
  * `gcl_roi_gather_rows` builds the skip input `[X | latent | prediction]` of the ROI rows in one kernel, reading the
    latents where the compact pipeline leaves them, on 16-byte rows padded with zero columns;
  * `input_proj` and the head are `gcl_dense_*` launches with the SiLU applied while loading the next layer's input
    (pre-activation buffers, include/gcl.h "Activation chaining"); the head's first Linear over `[state | skip]` is a
    split contraction - one column block of its weight on the processor state, the other on the skip input through the
    epilogue addend - so the concatenation is never materialised;
  * `gcl_roi_compose` writes `prediction + correction` on the ROI rows and copies every other row.

What differs from the reference (new capability, nothing it computes changes):
  * a batch dimension: `[B, G, F]` with B > 1 is B independent samples (the reference asserts B == 1), returning
    `[B, G, C]`; `[1, G, F]` returns the reference's `[G, C]`;
  * the constructor freezes the global model (`requires_grad_(False)`), which the reference's driver does right before
    building the head (scripts/train_roi_residual.py): so `TrainStep(roi_model, ...)` trains the head only.
"""
import sys
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
from scipy.spatial import cKDTree

from . import hip
from .functional import _Grads
from .models import InteractionNetProcessor, _get_activation
from .utils import mesh_edge_features


def build_roi_knn_graph(grid_lats: np.ndarray, grid_lons: np.ndarray, roi: Tuple[float, float, float, float],
                        k: int = 8):
    """`src/roi_residual.py:15-59`: (roi_mask [G] bool, roi_indices [n] int64, edge_index [2, n * (k_eff - 1)] int64,
    edge_features [E, 4] float32).  Senders are the k nearest ROI points of each receiver on the unit sphere (cKDTree,
    itself dropped), receivers are 0,0,...,1,1,...; the box test is the plain `>=` / `<=` one (no wrap at lon 0/360)."""
    lat_min, lat_max, lon_min, lon_max = roi
    roi_mask = (grid_lats >= lat_min) & (grid_lats <= lat_max) & (grid_lons >= lon_min) & (grid_lons <= lon_max)
    roi_indices = np.where(roi_mask)[0]
    if len(roi_indices) == 0:
        raise ValueError(f"No grid points in ROI {roi}")
    roi_lats, roi_lons = grid_lats[roi_indices], grid_lons[roi_indices]
    lat_r, lon_r = np.radians(roi_lats), np.radians(roi_lons)
    xyz = np.stack([np.cos(lat_r) * np.cos(lon_r), np.cos(lat_r) * np.sin(lon_r), np.sin(lat_r)], axis=-1)
    k_eff = min(k + 1, len(roi_indices))
    _, nbr = cKDTree(xyz).query(xyz, k=k_eff)
    if nbr.ndim == 1:
        nbr = nbr[:, None]
    nbr = nbr[:, 1:] if nbr.shape[1] > 1 else nbr[:, :0]
    senders = nbr.reshape(-1)
    receivers = np.repeat(np.arange(len(roi_indices)), nbr.shape[1])
    ei = np.stack([senders, receivers], axis=0).astype(np.int64)
    feats = torch.from_numpy(mesh_edge_features(roi_lats, roi_lons, ei))
    return roi_mask, roi_indices, torch.from_numpy(ei), feats


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


def _dw(dy, x, W, b, G: _Grads, wi: int, act=hip.ACT_NONE, dW=None):
    """dW (+)= dy^T act(x), db (+)= colsum(dy) into the gradient slots wi / wi + 1 (dW: a column block of the slot)."""
    dW = G.dst[wi] if dW is None else dW
    db, acc_w, acc_b = G.dst[wi + 1], G.acc[wi], G.acc[wi + 1]
    if db is not None and acc_b != acc_w:  # the dW kernel shares one accumulate flag between dW and db
        hip.dense_bwd_dw(dy, x, dW, None, acc_w, act)
        hip.colsum(dy, db, acc_b)
    else:
        hip.dense_bwd_dw(dy, x, dW, db, acc_w, act)


class ROIProjFn(torch.autograd.Function):
    """`input_proj` (src/roi_residual.py:118-122, 172): h = SiLU(skip W1^T + b1) W2^T + b2 on the padded skip rows.
    `skip` carries no gradient, so the first layer's backward is dW / db only."""

    @staticmethod
    def forward(ctx, skip3, S: int, W1, b1, W2, b2):
        B, n, Sp = skip3.shape
        H = W1.shape[0]
        k2 = skip3.view(B * n, Sp)
        W1p = hip.pad_rows(W1.detach().unsqueeze(0), H, Sp)[0]  # zero weight columns meet the zero skip columns
        za = hip.dense_fwd(k2, W1p, b1.detach())
        h = hip.dense_fwd(za, W2.detach(), b2.detach(), hip.ACT_SILU)
        ctx.S, ctx.k2, ctx.za = S, k2, za
        ctx.params = (W1, b1, W2, b2)
        return h.view(B, n, H)

    @staticmethod
    def backward(ctx, dh):
        W1, b1, W2, b2 = ctx.params
        G = _Grads(list(ctx.params), list(ctx.needs_input_grad[2:]))
        dh2 = hip.rows2d(dh)
        if G.dst[2] is None:
            G.dst[2] = torch.zeros_like(W2)
        _dw(dh2, ctx.za, W2, b2, G, 2, hip.ACT_SILU)
        dza = hip.dense_bwd_dx(dh2, W2.detach(), ctx.za, hip.ACT_SILU)
        if G.dst[0] is None:
            G.dst[0] = torch.zeros_like(W1)
        _dw(dza, ctx.k2[:, :ctx.S], W1, b1, G, 0)
        return (None, None) + G.out()


class ROIHeadFn(torch.autograd.Function):
    """`ROIResidualHead` (src/roi_residual.py:62-79) on `[state | skip]` without the concatenation: the first Linear
    runs as skip W1[:, H:]^T + b1 (one launch) then state W1[:, :H]^T + that (the addend of a second launch).  The
    last Linear runs Cp = roundup(C, 4) wide (a zero weight row / bias entry) so the correction and its gradient stay
    on 16-byte rows; the returned [B, n, Cp] correction has zero columns beyond C."""

    @staticmethod
    def forward(ctx, state3, skip3, S: int, W1, b1, W2, b2, W3, b3):
        B, n, H = state3.shape
        Sp = skip3.shape[2]
        Cc = W3.shape[0]
        Cp = _pad4(Cc)
        s2 = hip.rows2d(state3.detach())
        k2 = skip3.view(B * n, Sp)
        W1p = hip.pad_rows(W1.detach().unsqueeze(0), W1.shape[0], H + Sp)[0]  # [Hh, H + Sp]: [W_state | W_skip | 0]
        z1 = hip.dense_fwd(k2, W1p[:, H:], b1.detach())
        hip.dense_fwd(s2, W1p[:, :H], None, addend=z1, out=z1)
        z2 = hip.dense_fwd(z1, W2.detach(), b2.detach(), hip.ACT_SILU)
        W3p = hip.pad_rows(W3.detach().unsqueeze(0), Cp, W3.shape[1])[0]
        b3p = hip.pad_rows(b3.detach().view(1, 1, Cc), 1, Cp).view(Cp)
        corr = hip.dense_fwd(z2, W3p, b3p, hip.ACT_SILU)
        ctx.S, ctx.H, ctx.Cc = S, H, Cc
        ctx.s2, ctx.k2, ctx.z1, ctx.z2, ctx.W1p, ctx.W3p = s2, k2, z1, z2, W1p, W3p
        ctx.params = (W1, b1, W2, b2, W3, b3)
        ctx.state_shape = state3.shape
        return corr.view(B, n, Cp)

    @staticmethod
    def backward(ctx, dcorr):
        W1, b1, W2, b2, W3, b3 = ctx.params
        H, Cc = ctx.H, ctx.Cc
        G = _Grads(list(ctx.params), list(ctx.needs_input_grad[3:]))
        dy = hip.rows2d(dcorr)  # [rows, Cp]; the columns beyond C only ever meet the zero weight row
        for wi, W in ((0, W1), (2, W2), (4, W3)):
            if G.dst[wi] is None:
                G.dst[wi] = torch.zeros_like(W)
        _dw(dy[:, :Cc], ctx.z2, W3, b3, G, 4, hip.ACT_SILU)
        dz2 = hip.dense_bwd_dx(dy, ctx.W3p, ctx.z2, hip.ACT_SILU)
        _dw(dz2, ctx.z1, W2, b2, G, 2, hip.ACT_SILU)
        dz1 = hip.dense_bwd_dx(dz2, W2.detach(), ctx.z1, hip.ACT_SILU)
        dW1 = G.dst[0]
        if G.dst[1] is not None and G.acc[1] != G.acc[0]:
            hip.colsum(dz1, G.dst[1], G.acc[1])
            db_args = (None, G.acc[0])
        else:
            db_args = (G.dst[1], G.acc[0])
        hip.dense_bwd_dw(dz1, ctx.k2[:, :ctx.S], dW1[:, H:], db_args[0], db_args[1])
        hip.dense_bwd_dw(dz1, ctx.s2, dW1[:, :H], None, G.acc[0])
        dstate = None
        if ctx.needs_input_grad[0]:
            dstate = hip.dense_bwd_dx(dz1, ctx.W1p[:, :H]).view(ctx.state_shape)
        return (dstate, None, None) + G.out()


class ROIComposeFn(torch.autograd.Function):
    """`global_pred + zeros_like(global_pred).index_add(0, roi, corr)` (src/roi_residual.py:183-185) in one kernel;
    the backward is the row gather d_corr[b, i] = d_out[b, roi[i]] (zero-padded to the correction's Cp columns)."""

    @staticmethod
    def forward(ctx, pred3, corr3, rows, pos):
        ctx.rows, ctx.G, ctx.Cp = rows, pred3.shape[1], corr3.shape[2]
        return hip.roi_compose(pred3, corr3, pos)

    @staticmethod
    def backward(ctx, dout):
        d3 = dout if dout.stride(2) == 1 else dout.contiguous()
        dcorr = hip.roi_gather_rows(ctx.rows, ctx.G, [d3], ctx.Cp, d3.shape[0]) if ctx.needs_input_grad[1] else None
        return None, dcorr, None, None


class ROIResidualHead(nn.Module):
    """`src/roi_residual.py:62-79`: Linear, SiLU, Linear, SiLU, Linear over `[node_state | skip]`; the last Linear
    starts at normal(std=0.01) weights and a zero bias."""

    def __init__(self, input_dim: int, hidden_dim: int, output_dim: int):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.SiLU(), nn.Linear(hidden_dim, hidden_dim),
                                 nn.SiLU(), nn.Linear(hidden_dim, output_dim))
        nn.init.normal_(self.mlp[-1].weight, std=0.01)
        nn.init.zeros_(self.mlp[-1].bias)

    def _corr(self, node_state3, skip3, skip_dim: int):
        """[B, n, Cp] correction from [B, n, H] states and [B, n, Sp] skip rows (Sp = roundup(skip_dim, 4), zero pad)."""
        m = self.mlp
        return ROIHeadFn.apply(node_state3, skip3, skip_dim, m[0].weight, m[0].bias, m[2].weight, m[2].bias,
                               m[4].weight, m[4].bias)

    def forward(self, node_state: torch.Tensor, skip_features: torch.Tensor) -> torch.Tensor:
        squeeze = node_state.dim() == 2
        s3 = node_state if not squeeze else node_state.unsqueeze(0)
        k3 = skip_features if not squeeze else skip_features.unsqueeze(0)
        S = self.mlp[0].weight.shape[1] - s3.shape[-1]
        if k3.shape[-1] != _pad4(S) or not k3.is_contiguous():
            k3 = hip.pad_rows(k3.detach()[..., :S], k3.shape[1], _pad4(S))
        out = self._corr(s3, k3, S)[..., :self.mlp[-1].weight.shape[0]]
        return out[0] if squeeze else out


class ROIResidualModel(nn.Module):
    """`src/roi_residual.py:82-185`."""

    def __init__(self, global_model, roi: Tuple[float, float, float, float], grid_lats: np.ndarray,
                 grid_lons: np.ndarray, device, hidden_dim: int = 256, processor_steps: int = 6, roi_k: int = 8):
        super().__init__()
        self.global_model = global_model
        global_model.requires_grad_(False)  # frozen (the reference's driver does it before building the head)
        self.device = device
        self.roi = roi
        self.n_features = global_model.num_features
        self.obs_window = global_model.obs_window
        self.output_channels = global_model.num_features

        roi_mask, roi_indices, roi_edge_index, roi_edge_features = build_roi_knn_graph(
            grid_lats=grid_lats, grid_lons=grid_lons, roi=roi, k=roi_k)
        self.register_buffer("roi_mask", torch.tensor(roi_mask, dtype=torch.bool))
        self.register_buffer("roi_indices", torch.tensor(roi_indices, dtype=torch.int64))
        self.register_buffer("roi_edge_index", roi_edge_index)
        self.register_buffer("roi_edge_features", roi_edge_features)
        self.n_roi_grid = int(roi_mask.sum())
        # int32 row lists of the two glue kernels (not in the state dict): ROI row -> grid row, grid row -> ROI row | -1
        G = int(roi_mask.shape[0])
        pos = torch.full((G,), -1, dtype=torch.int32)
        pos[torch.as_tensor(roi_indices, dtype=torch.int64)] = torch.arange(self.n_roi_grid, dtype=torch.int32)
        self.register_buffer("_roi_rows", torch.as_tensor(roi_indices, dtype=torch.int64).to(torch.int32), persistent=False)
        self.register_buffer("_roi_pos", pos, persistent=False)

        total_feature_size = self.n_features * self.obs_window
        global_latent_dim = global_model.encoder.output_dim
        self.skip_dim = total_feature_size + global_latent_dim + self.output_channels
        self.input_proj = nn.Sequential(nn.Linear(self.skip_dim, hidden_dim), _get_activation("swish"),
                                        nn.Linear(hidden_dim, hidden_dim))
        self.processor = InteractionNetProcessor(node_dim=hidden_dim, raw_edge_dim=4, edge_latent_dim=hidden_dim,
                                                 hidden_dim=hidden_dim, num_steps=processor_steps, activation="swish",
                                                 use_layer_norm=True)
        self.decoder = ROIResidualHead(input_dim=hidden_dim + self.skip_dim, hidden_dim=hidden_dim,
                                       output_dim=self.output_channels)
        self.to(device)

        n_trainable = sum(p.numel() for name, p in self.named_parameters()
                          if not name.startswith("global_model.") and p.requires_grad)
        deg = torch.bincount(self.roi_edge_index[1].cpu(), minlength=self.n_roi_grid)
        # the reference prints these on stdout; here they go to stderr so that stdout stays clean for callers
        print(f"[ROIResidual] Trainable parameters: {n_trainable:,}", file=sys.stderr)
        print(f"[ROIResidual] ROI grid points: {self.n_roi_grid}", file=sys.stderr)
        print(f"[ROIResidual] ROI graph edges: {self.roi_edge_index.shape[1]}", file=sys.stderr)
        if deg.numel():
            print(f"[ROIResidual] In-degree: min={deg.min().item()} max={deg.max().item()} "
                  f"mean={deg.float().mean().item():.1f}", file=sys.stderr)

    def _global(self, X, attention_threshold=0.0, **kwargs):
        """(prediction [B, G, C], grid latents [B, G, D]) of the frozen global model, one forward, no autograd."""
        with torch.no_grad():
            pred, lat, _ = self.global_model.forward_with_latents(X, attention_threshold, **kwargs)
        if pred.dim() == 2:
            pred, lat = pred.unsqueeze(0), lat.unsqueeze(0)
        return pred, lat

    def _skip(self, X3, pred3, lat3):
        """[B, n, Sp] = [X | latent | prediction] of the ROI rows, zero-padded to Sp = roundup(skip_dim, 4)."""
        G = X3.shape[1]
        return hip.roi_gather_rows(self._roi_rows, G, [X3, lat3, pred3], _pad4(self.skip_dim), X3.shape[0])

    def _head(self, X3, pred3, lat3):
        """The trainable part: correction [B, n, Cp] from the global outputs (separated so that tests can inject them)."""
        skip = self._skip(X3, pred3, lat3)
        ip = self.input_proj
        h = ROIProjFn.apply(skip, self.skip_dim, ip[0].weight, ip[0].bias, ip[2].weight, ip[2].bias)
        h = self.processor(x=h, edge_index=self.roi_edge_index, edge_attr_raw=self.roi_edge_features)
        return self.decoder._corr(h, skip, self.skip_dim)

    def forward(self, X: torch.Tensor, attention_threshold: float = 0.0, **kwargs) -> torch.Tensor:
        X3 = X if X.dim() == 3 else X.unsqueeze(0)
        if X3.shape[-1] != self.n_features * self.obs_window:
            raise ValueError(f"expected {self.n_features * self.obs_window} input channels per grid point, got {X3.shape[-1]}")
        if X3.stride(2) != 1:
            X3 = X3.contiguous()
        pred3, lat3 = self._global(X, attention_threshold, **kwargs)
        corr = self._head(X3, pred3, lat3)
        out = ROIComposeFn.apply(pred3, corr, self._roi_rows, self._roi_pos)
        return out[0] if out.shape[0] == 1 else out
