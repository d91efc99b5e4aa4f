"""Module API of the reference's `src/dual_mesh.py`, executed by hand-written gfx950 kernels.

A frozen, pretrained `WeatherPrediction` and a trainable regional module on a refined icosahedral mesh over a lat/lon
box; the regional correction is added on the grid points inside the box:

  create_regional_mesh            src/dual_mesh.py:43-126   level-`level` vertices in the box + buffer, not in level 6
  build_cross_edges               src/dual_mesh.py:129-204  k nearest global mesh nodes of every regional node
  build_regional_grid_mesh_edges  src/dual_mesh.py:207-297  ROI grid <-> regional mesh kNN edges (+ decoding distances)
  CrossMessageLayer               src/dual_mesh.py:302-361  `g2r_edge_mlp.{0,2}`, `norm_reg` (node-mode LayerNorm)
  RegionalProcessor               src/dual_mesh.py:364-398  `edge_encoder.0`, ONE shared `step` applied num_steps times
  RegionalEncoder / Decoder       src/dual_mesh.py:401-476  `mlp.{0,2}`
  DualMeshModel                   src/dual_mesh.py:479-805  `forward`, `precompute_global`, `forward_cached`, buffers

How the forward runs on the HIP path:
  * the global model runs ONCE under no_grad through `forward_with_latents` (prediction, grid latents, processed mesh
    latents); `gcl_roi_gather_rows` builds `roi_input = [X | latent]` of the ROI rows (zero-padded 16-byte rows) and,
    in a second call, the global mesh rows of the cross-edge senders;
  * encoder: SiLU(roi_input W1^T + b1) is averaged over each regional node's encoding edges FIRST
    (`gcl_segment_wsum`, SiLU applied on load) and W2 then runs on the n_reg rows - every regional node has k_enc >= 1
    encoding edges, so the mean and the Linear commute;
  * cross message: the first g2r Linear over `[h_global[s] | h_reg[r] | edge]` is split by operand (sender rows x W_g,
    regional rows x W_r, encoded cross-edge features x W_e + b, batch-invariant) and combined by `gcl_edge_combine`;
    `gcl_cross_update_fwd` does mean + residual + node LayerNorm in one pass per regional row;
  * processor: `InteractionNetFn` with the shared step's parameters repeated num_steps times; every step's gradient
    lands in the same parameter (summed by autograd, or accumulated in place into a preinstalled `.grad`);
  * decoder: the `[IDW-sum of mesh rows | roi_input]` concatenation is never built: W_skip runs on roi_input, W_mesh on
    the n_reg mesh rows, and the IDW sum of the projected rows takes the skip term as its addend (`gcl_segment_wsum`);
    the last Linear runs Cp = roundup(C, 4) wide (a zero weight row) so that the correction stays on 16-byte rows;
  * `gcl_roi_compose` adds the correction on the ROI rows; every other row is a bit-exact copy of the prediction.

What differs from the reference (new capability, nothing it computes changes):
  * a batch dimension: `[B, G, F]` with B > 1 is B independent samples (the reference asserts B == 1), returning
    `[B, G, C]`; `[1, G, F]` returns the reference's `[G, C]`.  `precompute_global` / `forward_cached` take the same
    batch dimension (B = 1 gives the reference's shapes);
  * the constructor freezes the global model, as the reference's driver does with `--freeze-global` (its default);
  * construction diagnostics go to stderr;
  * the encoder, cross-message and decoder modules are parameter holders with the reference's keys; their compute runs
    inside `DualMeshModel` (the regional processor's own `forward` works standalone);
  * `_get_global_latents` (src/dual_mesh.py:631-661) is not provided: nothing in the reference calls it, and
    `forward_with_latents` returns the same processed mesh latents.
"""
import sys
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
from scipy.spatial import cKDTree

from . import hip
from .capture import Captured, graph_enabled
from .functional import InteractionNetFn, _Grads
from .mesh import TriangularMesh, get_edges_from_faces, get_hierarchy_of_triangular_meshes_for_sphere
from .models import InteractionNetLayer, InteractionNetProcessor, LayerNorm, _act_spec, _get_activation
from .roi_residual import ROIComposeFn, _dw, _pad4
from .utils import mesh_edge_features


def _log(msg: str):
    print(msg, file=sys.stderr)


def _xyz(lats, lons):
    lat_r, lon_r = np.radians(lats), np.radians(lons)
    return np.stack([np.cos(lat_r) * np.cos(lon_r), np.cos(lat_r) * np.sin(lon_r), np.sin(lat_r)], axis=-1)


# ------------------------------------------------------------------------------------------------------------------
# Host graph builders (once, at construction)
# ------------------------------------------------------------------------------------------------------------------
def create_regional_mesh(roi: Tuple[float, float, float, float], level: int = 8, buffer_deg: float = 2.0):
    """`src/dual_mesh.py:43-126`: (TriangularMesh of the kept vertices and the faces whose three vertices survive,
    reg_lats, reg_lons float32).  Kept: level-`level` vertices inside the box + buffer (plain `>=` / `<=`, no wrap at
    0/360) whose index is >= n_global = len(meshes[min(level, 6)].vertices).  A level <= 6 keeps nothing and raises."""
    lat_min, lat_max, lon_min, lon_max = roi
    meshes = get_hierarchy_of_triangular_meshes_for_sphere(splits=level)
    finest = meshes[level]
    vertices = finest.vertices
    lats_deg = np.degrees(np.arcsin(np.clip(vertices[:, 2], -1, 1)))
    lons_deg = np.degrees(np.arctan2(vertices[:, 1], vertices[:, 0])) % 360
    n_global = len(meshes[min(level, 6)].vertices)
    in_roi = ((lats_deg >= lat_min - buffer_deg) & (lats_deg <= lat_max + buffer_deg) &
              (lons_deg >= lon_min - buffer_deg) & (lons_deg <= lon_max + buffer_deg))
    new_only = np.zeros(len(vertices), dtype=bool)
    new_only[n_global:] = True
    kept = np.where(in_roi & new_only)[0]
    if len(kept) == 0:
        raise ValueError(f"create_regional_mesh: no level-{level} vertex beyond the level-{min(level, 6)} prefix lies in "
                         f"ROI {roi} with a {buffer_deg}° buffer (a level <= 6 never has one)")
    old_to_new = np.full(len(vertices), -1, dtype=np.int64)
    old_to_new[kept] = np.arange(len(kept))
    faces = finest.faces
    new_faces = old_to_new[faces[np.all(old_to_new[faces] >= 0, axis=1)]]
    regional_mesh = TriangularMesh(vertices=vertices[kept], faces=new_faces.astype(np.int32))
    reg_lats = lats_deg[kept].astype(np.float32)
    reg_lons = lons_deg[kept].astype(np.float32)
    _log(f"[RegionalMesh] level={level}, ROI={roi}, buffer={buffer_deg}°: {len(vertices)} level-{level} vertices, "
         f"{n_global} global, {len(kept)} regional, {len(new_faces)} faces")
    return regional_mesh, reg_lats, reg_lons


def build_cross_edges(global_lats: np.ndarray, global_lons: np.ndarray, reg_lats: np.ndarray, reg_lons: np.ndarray,
                      k: int = 3):
    """`src/dual_mesh.py:129-204`: (cross_edge_index int64 [2, 2 * n_reg * k], cross_edge_features float32 [E, 4]).
    First half global -> regional (sender: global index, receiver: regional index), second half the reverse; the
    features are `mesh_edge_features` over the unified node list [global | regional]."""
    _, gidx = cKDTree(_xyz(global_lats, global_lons)).query(_xyz(reg_lats, reg_lons), k=k)
    n_reg, n_global = len(reg_lats), len(global_lats)
    reg_indices = np.repeat(np.arange(n_reg), k)
    glob_indices = np.asarray(gidx).reshape(-1)
    senders = np.concatenate([glob_indices, reg_indices])
    receivers = np.concatenate([reg_indices, glob_indices])
    cross_edge_index = torch.tensor(np.stack([senders, receivers], axis=0), dtype=torch.int64)
    all_lats = np.concatenate([global_lats, reg_lats])
    all_lons = np.concatenate([global_lons, reg_lons])
    unified = np.stack([np.concatenate([glob_indices, reg_indices + n_global]),
                        np.concatenate([reg_indices + n_global, glob_indices])], axis=0)
    feats = torch.from_numpy(mesh_edge_features(all_lats, all_lons, unified))
    _log(f"[CrossEdges] {len(senders)} edges ({n_reg}×{k} bidirectional)")
    return cross_edge_index, feats


def build_regional_grid_mesh_edges(grid_lats: np.ndarray, grid_lons: np.ndarray, reg_lats: np.ndarray,
                                   reg_lons: np.ndarray, roi: Tuple[float, float, float, float], k_encode: int = 4,
                                   k_decode: int = 3, **kwargs):
    """`src/dual_mesh.py:207-297`: (roi_mask [G] bool, encoding_edges int64 [2, n_reg * k_enc] = [roi row, mesh node],
    decoding_edges int64 [2, n_roi * k_dec] = [mesh node, roi row], decoding distances float32 [n_roi * k_dec])."""
    lat_min, lat_max, lon_min, lon_max = roi
    roi_mask = (grid_lats >= lat_min) & (grid_lats <= lat_max) & (grid_lons >= lon_min) & (grid_lons <= lon_max)
    roi_indices = np.where(roi_mask)[0]
    n_roi = len(roi_indices)
    if n_roi == 0:
        raise ValueError(f"build_regional_grid_mesh_edges: ROI {roi} holds no grid point")
    reg_xyz = _xyz(reg_lats, reg_lons)
    roi_xyz = _xyz(grid_lats[roi_indices], grid_lons[roi_indices])
    n_mesh = len(reg_lats)
    k_enc = min(k_encode, n_roi)
    _, grid_nb = cKDTree(roi_xyz).query(reg_xyz, k=k_enc)
    grid_nb = np.asarray(grid_nb).reshape(n_mesh, -1)
    encoding_edges = torch.tensor(np.stack([grid_nb.reshape(-1), np.repeat(np.arange(n_mesh), k_enc)], axis=0),
                                  dtype=torch.int64)
    k_dec = min(k_decode, n_mesh)
    dec_d, mesh_nb = cKDTree(reg_xyz).query(roi_xyz, k=k_dec)
    mesh_nb = np.asarray(mesh_nb).reshape(n_roi, -1)
    decoding_edges = torch.tensor(np.stack([mesh_nb.reshape(-1), np.repeat(np.arange(n_roi), k_dec)], axis=0),
                                  dtype=torch.int64)
    dec_dist = torch.tensor(np.asarray(dec_d).reshape(-1), dtype=torch.float32)
    _log(f"[RegionalGridMesh] ROI grid points: {n_roi}; encoding edges {encoding_edges.shape[1]} ({n_mesh}×{k_enc}), "
         f"decoding edges {decoding_edges.shape[1]} ({n_roi}×{k_dec})")
    return roi_mask, encoding_edges, decoding_edges, dec_dist


class _WCSR:
    """A weighted bipartite edge list (src row -> dst row, weight w) as two int32 CSRs on the device: by destination
    (`idx` = source row) for the forward sum, by source (`tidx` = destination row) for its transpose, same weights.
    Both keep the edges of a row in their original order (stable sorts)."""

    def __init__(self, src, dst, w, n_src: int, n_dst: int, device):
        src, dst, w = src.to("cpu", torch.int64), dst.to("cpu", torch.int64), w.to("cpu", torch.float32)
        i32 = lambda t: t.to(torch.int32).to(device)

        def csr(key, n):
            order = torch.sort(key, stable=True).indices
            rowptr = torch.zeros(n + 1, dtype=torch.int64)
            rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)
            return order, i32(rowptr)

        order, self.rowptr = csr(dst, n_dst)
        self.idx, self.w = i32(src[order]), w[order].contiguous().to(device)
        torder, self.trowptr = csr(src, n_src)
        self.tidx, self.tw = i32(dst[torder]), w[torder].contiguous().to(device)
        self.n_src, self.n_dst = n_src, n_dst


class _CrossLayout:
    """The global -> regional half of the cross edges sorted by receiver (stable): `order` maps a sorted position to the
    reference edge id, `snd` / `rcv` are the sorted endpoints, `rowptr` the receiver CSR, `invdeg` 1 / in-degree."""

    def __init__(self, cross_edge_index, n_reg: int, device):
        half = cross_edge_index.shape[1] // 2
        snd, rcv = cross_edge_index[0, :half].to("cpu", torch.int64), cross_edge_index[1, :half].to("cpu", torch.int64)
        order = torch.sort(rcv, stable=True).indices
        cnt = torch.bincount(rcv, minlength=n_reg)
        rowptr = torch.zeros(n_reg + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(cnt, 0)
        i32 = lambda t: t.to(torch.int32).to(device)
        self.half, self.order_cpu = half, order
        self.order, self.snd, self.rcv, self.rowptr = i32(order), i32(snd[order]), i32(rcv[order]), i32(rowptr)
        self.snd_ref = i32(snd)  # reference edge order (precompute_global's cross_sender_feat)
        self.ident = i32(torch.arange(half))
        self.invdeg = (1.0 / cnt.clamp(min=1).to(torch.float32)).to(device)


# ------------------------------------------------------------------------------------------------------------------
# autograd Functions of the regional module
# ------------------------------------------------------------------------------------------------------------------
class RegEncoderFn(torch.autograd.Function):
    """RegionalEncoder (src/dual_mesh.py:415-426): h = mean_enc(SiLU(roi_in W1^T + b1)) W2^T + b2 on the regional rows.
    `roi_in` ([B, n_roi, Sp], zero-padded past S columns) carries no gradient."""

    @staticmethod
    def forward(ctx, roi3, S: int, lay: _WCSR, W1, b1, W2, b2):
        B, n_roi, Sp = roi3.shape
        H = W1.shape[0]
        k2 = roi3.view(B * n_roi, Sp)
        W1p = hip.pad_rows(W1.detach().unsqueeze(0), H, Sp)[0]  # zero weight columns meet the zero input columns
        za = hip.dense_fwd(k2, W1p, b1.detach())
        agg = hip.segment_wsum(za.view(B, n_roi, H), lay.idx, lay.w, lay.rowptr, act=hip.ACT_SILU)
        agg2 = agg.view(B * lay.n_dst, H)
        h = hip.dense_fwd(agg2, W2.detach(), b2.detach())
        ctx.S, ctx.lay, ctx.k2, ctx.za, ctx.agg2, ctx.B = S, lay, k2, za, agg2, B
        ctx.W1p, ctx.roi_shape = W1p, roi3.shape
        ctx.params = (W1, b1, W2, b2)
        return h.view(B, lay.n_dst, W2.shape[0])

    @staticmethod
    def backward(ctx, dh):
        W1, b1, W2, b2 = ctx.params
        lay, B = ctx.lay, ctx.B
        G = _Grads(list(ctx.params), list(ctx.needs_input_grad[3:]))
        for wi, W in ((0, W1), (2, W2)):
            if G.dst[wi] is None:
                G.dst[wi] = torch.zeros_like(W)
        dh2 = hip.rows2d(dh)
        _dw(dh2, ctx.agg2, W2, b2, G, 2)
        dagg = hip.dense_bwd_dx(dh2, W2.detach())
        H = dagg.shape[1]
        da = hip.segment_wsum(dagg.view(B, lay.n_dst, H), lay.tidx, lay.tw, lay.trowptr)  # transposed mean
        dza = hip.act_bwd(ctx.za, da.view(-1, H), hip.ACT_SILU)
        _dw(dza, ctx.k2[:, :ctx.S], W1, b1, G, 0)
        droi = None
        if ctx.needs_input_grad[0]:  # the raw-input columns carry a gradient in autoregressive training
            droi = hip.dense_bwd_dx(dza, ctx.W1p).view(ctx.roi_shape)
        return (droi, None, None) + G.out()


class RoiInputFn(torch.autograd.Function):
    """roi_input = [X[roi] | latent[roi]] on zero-padded [B, n_roi, Sp] rows (src/dual_mesh.py:683-686, one
    `gcl_roi_gather_rows`).  The latents come from the frozen global model; X carries a gradient in autoregressive
    training (the previous step's output is in the window), which goes back to the ROI rows of X through
    `gcl_roi_compose` over zeros: dX[b, g] = d_roi[b, pos[g], :F] on ROI rows, 0 elsewhere."""

    @staticmethod
    def forward(ctx, X3, lat3, rows, pos, Sp: int):
        ctx.pos, ctx.xshape = pos, X3.shape
        return hip.roi_gather_rows(rows, X3.shape[1], [X3.detach(), lat3], Sp, X3.shape[0])

    @staticmethod
    def backward(ctx, droi):
        dX = None
        if ctx.needs_input_grad[0]:
            d3 = droi if droi.stride(2) == 1 else droi.contiguous()
            zero = hip.zero_(torch.empty(ctx.xshape, dtype=torch.float32, device=droi.device))
            dX = hip.roi_compose(zero, d3, ctx.pos)
        return dX, None, None, None, None


def _cols(W, a: int, b: int):
    """Columns [a, b) of W as a 16-byte aligned [rows, roundup(b - a, 4)] operand (a view when it already is one)."""
    if a % 4 == 0 and (b - a) % 4 == 0 and W.stride(0) % 4 == 0:
        return W[:, a:b]
    return hip.pad_rows(W[:, a:b].unsqueeze(0), W.shape[0], _pad4(b - a))[0]


class CrossMsgFn(torch.autograd.Function):
    """The global -> regional cross message (src/dual_mesh.py:345-357, 774-787) over the receiver-sorted half of the
    cross edges:  ce = SiLU(raw W_ce^T + b_ce);  m = SiLU([S | h[r] | ce] W1^T + b1) W2^T + b2;
    y = LayerNorm_node(h + mean_r(m)).  S [B, hE, Dgp]: the gathered global mesh rows of the senders (zero-padded past
    Dg columns, no gradient).  params: W_ce, b_ce, W1, b1, W2, b2, gamma, beta."""

    @staticmethod
    def forward(ctx, h3, S3, Dg: int, lay: _CrossLayout, raw, eps: float, Wce, bce, W1, b1, W2, b2, gamma, beta):
        B, n, D = h3.shape
        hE, Dgp = lay.half, S3.shape[2]
        H = W1.shape[0]
        h3 = h3.detach() if h3.is_contiguous() else h3.detach().contiguous()
        W1d = W1.detach()
        Wg, Wr, We = _cols(W1d, 0, Dg), _cols(W1d, Dg, Dg + D), _cols(W1d, Dg + D, Dg + 2 * D)
        cep = hip.dense_fwd(raw, Wce.detach(), bce.detach())                   # [hE, D] batch-invariant
        ce = hip.dense_fwd(cep, We, b1.detach(), hip.ACT_SILU)                 # [hE, H] = SiLU(cep) W_e^T + b1
        S2, h2 = S3.view(B * hE, Dgp), h3.view(B * n, D)
        A = hip.dense_fwd(S2, Wg, None).view(B, hE, H)
        R = hip.dense_fwd(h2, Wr, None).view(B, n, H)
        hip.edge_combine(A, None, ce.unsqueeze(0).expand(B, hE, H), lay.ident, None, R, lay.rcv, out3=A)
        A2 = A.view(B * hE, H)
        msg = hip.dense_fwd(A2, W2.detach(), b2.detach(), hip.ACT_SILU).view(B, hE, D)
        pre, y, stats = hip.cross_update_fwd(h3, msg, lay.rowptr, gamma.detach(), beta.detach(), eps)
        ctx.lay, ctx.dims, ctx.raw = lay, (B, n, D, H, Dg), raw
        ctx.S2, ctx.h2, ctx.cep, ctx.A2, ctx.pre, ctx.stats, ctx.Wr, ctx.We = S2, h2, cep, A2, pre, stats, Wr, We
        ctx.params = (Wce, bce, W1, b1, W2, b2, gamma, beta)
        return y

    @staticmethod
    def backward(ctx, dy):
        Wce, bce, W1, b1, W2, b2, gamma, beta = ctx.params
        lay = ctx.lay
        B, n, D, H, Dg = ctx.dims
        hE = lay.half
        G = _Grads(list(ctx.params), list(ctx.needs_input_grad[6:]))
        for wi in (0, 2, 4, 6, 7):
            if G.dst[wi] is None:
                G.dst[wi] = torch.zeros_like(ctx.params[wi])
        dpre = hip.layernorm_bwd(hip.rows2d(dy), ctx.pre.view(B * n, D), gamma.detach(), ctx.stats, G.dst[6], G.dst[7],
                                 G.acc[6] and G.acc[7])
        dmsg = hip.edge_combine(None, None, dpre.view(B, n, D), lay.rcv, lay.invdeg, None, None)  # d pre[rcv] / deg
        dmsg2 = dmsg.view(B * hE, D)
        dA = hip.dense_bwd_dx(dmsg2, W2.detach(), ctx.A2, hip.ACT_SILU)                          # [B * hE, H]
        _dw(dmsg2, ctx.A2, W2, b2, G, 4, hip.ACT_SILU)
        dW1, acc1 = G.dst[2], G.acc[2]
        hip.dense_bwd_dw(dA, ctx.S2[:, :Dg], dW1[:, :Dg], None, acc1)
        dR = hip.segment_reduce(dA.view(B, hE, H), None, lay.rowptr, False)                       # [B, n, H]
        dR2 = dR.view(B * n, H)
        hip.dense_bwd_dw(dR2, ctx.h2, dW1[:, Dg:Dg + D], None, acc1)
        # the encoded cross-edge term is shared by the samples: its gradient is the sum over the batch
        dce = dA if B == 1 else hip.gather2_rows(dA.view(B, hE, H), None, None, None, hE, B, sum_batch=True)[0]
        if G.dst[3] is not None:
            hip.colsum(dce, G.dst[3], G.acc[3])
        hip.dense_bwd_dw(dce, ctx.cep, dW1[:, Dg + D:], None, acc1, hip.ACT_SILU)
        dcep = hip.dense_bwd_dx(dce, ctx.We, ctx.cep, hip.ACT_SILU)
        _dw(dcep, ctx.raw, Wce, bce, G, 0)
        dh = None
        if ctx.needs_input_grad[0]:
            dh = hip.dense_bwd_dx(dR2, ctx.Wr, addend=dpre).view(B, n, D)
        return (dh, None, None, None, None, None) + G.out()


class RegDecoderFn(torch.autograd.Function):
    """RegionalDecoder with IDW weights and the skip input (src/dual_mesh.py:455-474) without the concatenation:
    z = IDW_dec(hm W_mesh^T) + roi_in W_skip^T + b1 (the skip term is the weighted sum's addend);
    corr = SiLU(z) W2^T + b2, Cp = roundup(C, 4) wide (zero columns beyond C)."""

    @staticmethod
    def forward(ctx, hm3, roi3, S: int, lay: _WCSR, W1, b1, W2, b2):
        B, n_reg, D = hm3.shape
        n_roi, Sp = roi3.shape[1], roi3.shape[2]
        Hh, Cc = W1.shape[0], W2.shape[0]
        Cp = _pad4(Cc)
        hm2 = hip.rows2d(hm3.detach())
        k2 = roi3.view(B * n_roi, Sp)
        W1p = hip.pad_rows(W1.detach().unsqueeze(0), Hh, D + Sp)[0]   # [W_mesh | W_skip | 0]
        z = hip.dense_fwd(k2, W1p[:, D:], b1.detach()).view(B, n_roi, Hh)
        P = hip.dense_fwd(hm2, W1p[:, :D], None).view(B, n_reg, Hh)
        hip.segment_wsum(P, lay.idx, lay.w, lay.rowptr, out3=z, addend3=z)
        z2 = z.view(B * n_roi, Hh)
        W2p = hip.pad_rows(W2.detach().unsqueeze(0), Cp, Hh)[0]
        b2p = hip.pad_rows(b2.detach().view(1, 1, Cc), 1, Cp).view(Cp)
        corr = hip.dense_fwd(z2, W2p, b2p, hip.ACT_SILU)
        ctx.S, ctx.D, ctx.Cc, ctx.lay, ctx.B = S, D, Cc, lay, B
        ctx.hm2, ctx.k2, ctx.z2, ctx.W1p, ctx.W2p = hm2, k2, z2, W1p, W2p
        ctx.params = (W1, b1, W2, b2)
        return corr.view(B, n_roi, Cp)

    @staticmethod
    def backward(ctx, dcorr):
        W1, b1, W2, b2 = ctx.params
        D, Cc, lay, B = ctx.D, ctx.Cc, ctx.lay, ctx.B
        G = _Grads(list(ctx.params), list(ctx.needs_input_grad[4:]))
        for wi, W in ((0, W1), (2, W2)):
            if G.dst[wi] is None:
                G.dst[wi] = torch.zeros_like(W)
        dy = hip.rows2d(dcorr)  # [rows, Cp]; the columns beyond C only ever meet the zero weight row
        _dw(dy[:, :Cc], ctx.z2, W2, b2, G, 2, hip.ACT_SILU)
        dz = hip.dense_bwd_dx(dy, ctx.W2p, ctx.z2, hip.ACT_SILU)          # [B * n_roi, Hh]
        dW1 = G.dst[0]
        if G.dst[1] is not None and G.acc[1] != G.acc[0]:
            hip.colsum(dz, G.dst[1], G.acc[1])
            db = None
        else:
            db = G.dst[1]
        hip.dense_bwd_dw(dz, ctx.k2[:, :ctx.S], dW1[:, D:], db, G.acc[0])
        Hh = dz.shape[1]
        dP = hip.segment_wsum(dz.view(B, lay.n_dst, Hh), lay.tidx, lay.tw, lay.trowptr)   # [B, n_reg, Hh]
        dP2 = dP.view(B * lay.n_src, Hh)
        hip.dense_bwd_dw(dP2, ctx.hm2, dW1[:, :D], None, G.acc[0])
        dhm = None
        if ctx.needs_input_grad[0]:
            dhm = hip.dense_bwd_dx(dP2, ctx.W1p[:, :D]).view(B, lay.n_src, D)
        droi = None
        if ctx.needs_input_grad[1]:
            droi = hip.dense_bwd_dx(dz, ctx.W1p[:, D:]).view(B, lay.n_dst, -1)
        return (dhm, droi, None, None) + G.out()


# ------------------------------------------------------------------------------------------------------------------
# Modules (reference names, parameters and state-dict keys)
# ------------------------------------------------------------------------------------------------------------------
class CrossMessageLayer(nn.Module):
    """`src/dual_mesh.py:302-361`: `g2r_edge_mlp` (Linear, SiLU, Linear) and `norm_reg` (node-mode LayerNorm).  Only the
    global -> regional half of the cross edges is used.  Its compute is `CrossMsgFn`, run by `DualMeshModel`."""

    def __init__(self, node_dim: int, edge_dim: int, hidden_dim: int, global_latent_dim: int = None,
                 activation: str = "swish"):
        super().__init__()
        g_dim = global_latent_dim if global_latent_dim is not None else node_dim
        self.g2r_edge_mlp = nn.Sequential(nn.Linear(g_dim + node_dim + edge_dim, hidden_dim), _get_activation(activation),
                                          nn.Linear(hidden_dim, node_dim))
        self.norm_reg = LayerNorm(node_dim, mode="node")


class RegionalProcessor(nn.Module):
    """`src/dual_mesh.py:364-398`: edge encoder (raw 4-D -> node_dim, SiLU) and ONE `InteractionNetLayer` applied
    `num_steps` times (shared weights).  Runs as `InteractionNetFn` with the step's parameters repeated."""

    def __init__(self, node_dim: int, raw_edge_dim: int = 4, hidden_dim: int = 256, num_steps: int = 4,
                 activation: str = "swish"):
        super().__init__()
        if node_dim % 4 != 0:
            raise NotImplementedError("InteractionNet on the HIP path needs a latent width that is a multiple of 4")
        self.edge_encoder = nn.Sequential(nn.Linear(raw_edge_dim, node_dim), _get_activation(activation))
        self.step = InteractionNetLayer(node_dim=node_dim, edge_dim=node_dim, hidden_dim=hidden_dim,
                                        activation=activation, use_layer_norm=True)
        self.num_steps = num_steps
        _act_spec(self, self.edge_encoder[1])
        self._layout = None

    _edge_layout = InteractionNetProcessor._edge_layout

    def forward(self, x, edge_index, edge_attr_raw):
        lay, raw, pad = self._edge_layout(edge_index, edge_attr_raw, x.shape[-2], x.device)
        enc_W = self.edge_encoder[0].weight
        if pad:
            enc_W = torch.nn.functional.pad(enc_W, (0, pad))
        enc_act = self.edge_encoder[1]
        params = [enc_W, self.edge_encoder[0].bias, enc_act.weight if isinstance(enc_act, nn.PReLU) else None]
        # one tensor in num_steps slots: autograd sums the returned gradients, or every slot accumulates into a
        # preinstalled .grad (functional._grad_slot)
        params += self.step.step_params() * self.num_steps
        return InteractionNetFn.apply(x, self, lay, raw, self.num_steps, self.act_kind, True, self.step.node_norm.eps,
                                      *params)


class RegionalEncoder(nn.Module):
    """`src/dual_mesh.py:401-426`: `mlp` (Linear, SiLU, Linear), then the mean over the encoding edges."""

    def __init__(self, input_dim: int, hidden_dim: int = 256):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(input_dim, hidden_dim), nn.SiLU(), nn.Linear(hidden_dim, hidden_dim))


class RegionalDecoder(nn.Module):
    """`src/dual_mesh.py:429-476`: `mlp` (Linear, SiLU, Linear) over `[IDW mesh sum | skip]`; the last Linear starts at
    normal(std=0.01) weights and a zero bias."""

    def __init__(self, input_dim: int, output_dim: int, hidden_dim: int = 256, skip_dim: int = 0):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(input_dim + skip_dim, hidden_dim), nn.SiLU(),
                                 nn.Linear(hidden_dim, output_dim))
        nn.init.normal_(self.mlp[-1].weight, std=0.01)
        nn.init.zeros_(self.mlp[-1].bias)


class DualMeshModel(nn.Module):
    """`src/dual_mesh.py:479-805`."""

    def __init__(self, global_model, roi: Tuple[float, float, float, float], grid_lats: np.ndarray,
                 grid_lons: np.ndarray, device, reg_mesh_level: int = 7, reg_mesh_buffer: float = 2.0,
                 reg_processor_steps: int = 4, cross_k: int = 3, hidden_dim: int = 256):
        super().__init__()
        self.global_model = global_model
        global_model.requires_grad_(False)  # frozen (the reference's driver: --freeze-global, default True)
        self.device = device
        self.roi = roi
        self.n_features = global_model.num_features
        self.obs_window = global_model.obs_window
        self.output_channels = global_model.num_features

        self.reg_mesh, reg_lats, reg_lons = create_regional_mesh(roi=roi, level=reg_mesh_level,
                                                                 buffer_deg=reg_mesh_buffer)
        self.n_reg_mesh = len(reg_lats)
        reg_edge_index = torch.tensor(get_edges_from_faces(self.reg_mesh.faces), dtype=torch.int64)
        self.register_buffer("reg_processing_edges", reg_edge_index)
        self.register_buffer("reg_processing_edge_features",
                             torch.from_numpy(mesh_edge_features(reg_lats, reg_lons, reg_edge_index.numpy())))

        cross_edge_index, cross_edge_features = build_cross_edges(
            global_lats=global_model._mesh_nodes_lat, global_lons=global_model._mesh_nodes_lon,
            reg_lats=reg_lats, reg_lons=reg_lons, k=cross_k)
        self.register_buffer("cross_edge_index", cross_edge_index)
        self.register_buffer("cross_edge_features", cross_edge_features)
        self.n_global_mesh = global_model._num_mesh_nodes

        roi_mask, enc_edges, dec_edges, dec_dist = build_regional_grid_mesh_edges(
            grid_lats=grid_lats, grid_lons=grid_lons, reg_lats=reg_lats, reg_lons=reg_lons, roi=roi)
        self.register_buffer("roi_mask", torch.tensor(roi_mask, dtype=torch.bool))
        self.register_buffer("reg_encoding_edges", enc_edges)
        self.register_buffer("reg_decoding_edges", dec_edges)
        self.n_roi_grid = int(roi_mask.sum())
        # IDW weights: w = 1/(d + eps), normalised per ROI point (src/dual_mesh.py:560-567)
        eps = 1e-8
        inv_dist = 1.0 / (dec_dist + eps)
        wsum = torch.zeros(self.n_roi_grid, dtype=torch.float32).index_add_(0, dec_edges[1], inv_dist)
        self.register_buffer("dec_idw_weights", inv_dist / (wsum[dec_edges[1]] + eps))

        total_feature_size = self.n_features * self.obs_window
        global_latent_dim = global_model.encoder.output_dim
        reg_enc_input_dim = total_feature_size + global_latent_dim
        self.reg_enc_input_dim, self.global_latent_dim = reg_enc_input_dim, global_latent_dim
        self.reg_encoder = RegionalEncoder(input_dim=reg_enc_input_dim, hidden_dim=hidden_dim)
        self.reg_processor = RegionalProcessor(node_dim=hidden_dim, raw_edge_dim=4, hidden_dim=hidden_dim,
                                               num_steps=reg_processor_steps)
        self.cross_message = CrossMessageLayer(node_dim=hidden_dim, edge_dim=hidden_dim, hidden_dim=hidden_dim,
                                               global_latent_dim=global_latent_dim)
        self.cross_edge_encoder = nn.Sequential(nn.Linear(4, hidden_dim), _get_activation("swish"))
        self.reg_decoder = RegionalDecoder(input_dim=hidden_dim, output_dim=self.output_channels, hidden_dim=hidden_dim,
                                           skip_dim=reg_enc_input_dim)

        # index lists of the kernels (not in the state dict)
        G = int(roi_mask.shape[0])
        roi_indices = torch.from_numpy(np.where(roi_mask)[0])
        pos = torch.full((G,), -1, dtype=torch.int32)
        pos[roi_indices] = torch.arange(self.n_roi_grid, dtype=torch.int32)
        self.register_buffer("_roi_rows", roi_indices.to(torch.int32), persistent=False)
        self.register_buffer("_roi_pos", pos, persistent=False)
        self.register_buffer("_roi_ident", torch.arange(self.n_roi_grid, dtype=torch.int32), persistent=False)
        self.to(device)
        dev = self.roi_mask.device
        enc_deg = torch.bincount(enc_edges[1], minlength=self.n_reg_mesh)
        self._enc = _WCSR(enc_edges[0], enc_edges[1], 1.0 / enc_deg.clamp(min=1).to(torch.float32)[enc_edges[1]],
                          self.n_roi_grid, self.n_reg_mesh, dev)
        self._dec = _WCSR(dec_edges[0], dec_edges[1], self.dec_idw_weights, self.n_reg_mesh, self.n_roi_grid, dev)
        self._cross = _CrossLayout(cross_edge_index, self.n_reg_mesh, dev)
        self._cross_raw = cross_edge_features[:self._cross.half][self._cross.order_cpu].contiguous().to(dev)

        reg_params = sum(p.numel() for n, p in self.named_parameters() if not n.startswith("global_model."))
        dec_deg = torch.bincount(dec_edges[1], minlength=self.n_roi_grid)
        _log(f"[DualMesh] Regional module parameters: {reg_params:,}")
        _log(f"[DualMesh] Global model parameters: {sum(p.numel() for p in global_model.parameters()):,}")
        _log(f"[DualMesh] ROI grid points: {self.n_roi_grid}")
        _log(f"[DualMesh] Regional mesh nodes: {self.n_reg_mesh}")
        for name, deg, n in (("encoding", enc_deg, self.n_reg_mesh), ("decoding", dec_deg, self.n_roi_grid)):
            z = int((deg == 0).sum())
            if z:
                _log(f"  WARNING: {z}/{n} nodes have ZERO {name} edges")
            _log(f"  {name.capitalize()} edge degree: min={deg.min().item()} max={deg.max().item()} "
                 f"mean={deg.float().mean().item():.1f}")

    # --- pieces ------------------------------------------------------------------------------------------------------
    def _global(self, X, attention_threshold=0.0, **kwargs):
        """(prediction [B, G, C], grid latents [B, G, D], processed mesh latents [B, M, D]), one frozen forward."""
        with torch.no_grad():
            pred, lat, mesh = self.global_model.forward_with_latents(X, attention_threshold, **kwargs)
        if pred.dim() == 2:
            pred, lat, mesh = pred.unsqueeze(0), lat.unsqueeze(0), mesh.unsqueeze(0)
        if mesh.stride(-1) != 1:
            mesh = mesh.contiguous()
        return pred, lat, mesh

    def _regional(self, roi3, send3):
        """The trainable part: correction [B, n_roi, Cp] from roi_input [B, n_roi, Sp] and the cross senders' global
        mesh rows [B, half_E, Dgp] in receiver-sorted order (separated so that tests can inject them)."""
        S = self.reg_enc_input_dim
        e = self.reg_encoder.mlp
        h = RegEncoderFn.apply(roi3, S, self._enc, e[0].weight, e[0].bias, e[2].weight, e[2].bias)
        ce, g2r, nr = self.cross_edge_encoder[0], self.cross_message.g2r_edge_mlp, self.cross_message.norm_reg
        h = CrossMsgFn.apply(h, send3, self.global_latent_dim, self._cross, self._cross_raw, nr.eps, ce.weight, ce.bias,
                             g2r[0].weight, g2r[0].bias, g2r[2].weight, g2r[2].bias, nr.weight, nr.bias)
        h = self.reg_processor(x=h, edge_index=self.reg_processing_edges,
                               edge_attr_raw=self.reg_processing_edge_features)
        d = self.reg_decoder.mlp
        return RegDecoderFn.apply(h, roi3, S, self._dec, d[0].weight, d[0].bias, d[2].weight, d[2].bias)

    def forward(self, X: torch.Tensor, attention_threshold=0.0, **kwargs):
        X3 = X if X.dim() == 3 else X.unsqueeze(0)
        if X3.shape[-1] != self.n_features * self.obs_window:
            raise ValueError(f"expected {self.n_features * self.obs_window} input channels per grid point, "
                             f"got {X3.shape[-1]}")
        if X3.stride(2) != 1:
            X3 = X3.contiguous()
        pred3, lat3, mesh3 = self._global(X, attention_threshold, **kwargs)
        B, G = X3.shape[0], X3.shape[1]
        roi3 = RoiInputFn.apply(X3, lat3, self._roi_rows, self._roi_pos, _pad4(self.reg_enc_input_dim))
        send3 = hip.roi_gather_rows(self._cross.snd, mesh3.shape[1], [mesh3], _pad4(self.global_latent_dim), B)
        corr = self._regional(roi3, send3)
        out = ROIComposeFn.apply(pred3, corr, self._roi_rows, self._roi_pos)
        return out[0] if out.shape[0] == 1 else out

    # --- cached training support ------------------------------------------------------------------------------------
    @torch.no_grad()
    def precompute_global(self, X: torch.Tensor) -> dict:
        """`src/dual_mesh.py:731-752`: the global outputs the regional module needs, as CPU tensors: `global_pred_roi`
        (n_roi, C), `roi_grid_latent` (n_roi, D), `cross_sender_feat` (half_E, D) - with a leading [B] for B > 1."""
        pred3, lat3, mesh3 = self._global(X, 0.0)
        B, G, C = pred3.shape
        D, M, Dm = lat3.shape[2], mesh3.shape[1], mesh3.shape[2]
        p = hip.roi_gather_rows(self._roi_rows, G, [pred3], _pad4(C), B)[..., :C]
        lt = hip.roi_gather_rows(self._roi_rows, G, [lat3], _pad4(D), B)[..., :D]
        cs = hip.roi_gather_rows(self._cross.snd_ref, M, [mesh3], _pad4(Dm), B)[..., :Dm]
        out = {"global_pred_roi": p.cpu(), "roi_grid_latent": lt.cpu(), "cross_sender_feat": cs.cpu()}
        if B == 1:
            out = {k: v[0] for k, v in out.items()}
        return out

    def forward_cached(self, roi_raw: torch.Tensor, global_pred_roi: torch.Tensor, roi_grid_latent: torch.Tensor,
                       cross_sender_feat: torch.Tensor) -> torch.Tensor:
        """`src/dual_mesh.py:754-805`: global_pred_roi + correction on the ROI rows, (n_roi, C) (or [B, n_roi, C] for
        batched inputs), from `precompute_global`'s outputs moved to the device."""
        squeeze = roi_raw.dim() == 2
        t3 = [t.unsqueeze(0) if squeeze else t for t in (roi_raw, global_pred_roi, roi_grid_latent, cross_sender_feat)]
        raw3, pred3, lat3, cs3 = [t if t.stride(-1) == 1 else t.contiguous() for t in t3]
        B, n = raw3.shape[0], raw3.shape[1]
        roi3 = torch.empty(B, n, _pad4(self.reg_enc_input_dim), dtype=torch.float32, device=raw3.device)
        hip.roi_gather_rows(None, n, [raw3, lat3], roi3.shape[2], B, out=roi3)
        send3 = hip.roi_gather_rows(self._cross.order, cs3.shape[1], [cs3], _pad4(cs3.shape[2]), B)
        corr = self._regional(roi3, send3)
        out = ROIComposeFn.apply(pred3, corr, self._roi_ident, self._roi_ident)
        return out[0] if squeeze else out


class DualMeshCachedStep(Captured):
    """One optimiser step of the reference's cached mode (scripts/train_dual_mesh.py:176-193): `forward_cached`, then
    `weighted_mse_loss(out_roi, y_roi, None)`, with `x_last_roi = roi_raw[..., -C:]` added to the output first when
    `use_residual`; backward and Adam over the regional parameters.  The global model never runs.

    Inputs are copied into static device buffers and, as in `TrainStep`, the step is captured into a hipGraph after
    two eager steps: use_graph=True requires the capture (a failure raises), None replays when the capture works and
    stays eager otherwise (see `.launch_mode` / `.graph_active`), False is always eager."""

    def __init__(self, model: DualMeshModel, lr=1e-3, use_residual: bool = False, use_graph=None):
        from .train import FlatParams, FusedAdam

        self.model = model
        self.flat = FlatParams(model)
        self.opt = FusedAdam(self.flat, lr=lr)
        self.use_residual = use_residual
        super().__init__(graph_enabled(use_graph), required=use_graph is True)

    def _work(self, roi_raw, pred, lat, cs, y):
        from .train import weighted_mse_loss

        self.flat.zero_grad()
        out = self.model.forward_cached(roi_raw, pred, lat, cs)
        o3, y3 = (out.unsqueeze(0), y.unsqueeze(0)) if out.dim() == 2 else (out, y)
        r3 = roi_raw.unsqueeze(0) if roi_raw.dim() == 2 else roi_raw
        x_last = r3[..., r3.shape[-1] - o3.shape[-1]:] if self.use_residual else None
        loss = weighted_mse_loss(o3, y3, x_last=x_last)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def __call__(self, roi_raw, global_pred_roi, roi_grid_latent, cross_sender_feat, y_roi):
        dev = self.flat.flat.device
        args = [t.to(dev, torch.float32) for t in (roi_raw, global_pred_roi, roi_grid_latent, cross_sender_feat, y_roi)]
        return self._run(*args).detach()
