"""Dual-mesh regional model (`src/dual_mesh.py`): the three graph builders against the reference's own output, the two
new kernels against torch indexing and arithmetic, the regional module against the reference module's fixture, the
shared processor step against unrolled copies, and the whole model (frozen global + regional module) against a CPU
oracle composed here - forward, cached forward, gradients and training steps."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from parity import check_grads, oracle_fp64

DEV = "cuda:0"


def _gfx():
    return np.load(os.path.join(GOLDEN, "dual_mesh_graph_vectors.npz"))


def _mfx():
    return np.load(os.path.join(GOLDEN, "dual_mesh_model_vectors.npz"))


def _regular(nlat, nlon):
    lats = np.linspace(-90, 90, nlat, endpoint=True)
    lons = np.linspace(0, 360, nlon, endpoint=False)
    lon_grid, lat_grid = np.meshgrid(lons, lats)
    return lat_grid.flatten().astype(np.float32), lon_grid.flatten().astype(np.float32)


class StubGlobal(nn.Module):
    """A frozen 'global model' with fixed outputs: what DualMeshModel reads from WeatherPrediction."""

    def __init__(self, pred, lat, mesh, obs, mlat, mlon):
        super().__init__()
        self.num_features, self.obs_window = pred.shape[-1], obs
        self.register_buffer("pred", pred)
        self.register_buffer("lat", lat)
        self.register_buffer("mesh", mesh)
        self._mesh_nodes_lat, self._mesh_nodes_lon, self._num_mesh_nodes = mlat, mlon, len(mlat)
        self.dummy = nn.Parameter(torch.zeros(1))  # a global parameter, frozen by the dual-mesh model
        self.encoder = type("Enc", (), {"output_dim": lat.shape[-1]})()

    def forward_with_latents(self, X, attention_threshold=0.0, **kw):
        return self.pred, self.lat, self.mesh


def _fx_model(z, device):
    from graphcast_lite_amd.dual_mesh import DualMeshModel

    Fe, obs, D, hidden, steps, k, level = (int(v) for v in z["dims"])
    stub = StubGlobal(torch.from_numpy(z["pred"]), torch.from_numpy(z["lat"]), torch.from_numpy(z["mesh"]), obs,
                      z["global_lats"], z["global_lons"])
    return DualMeshModel(stub, tuple(z["roi"]), z["grid_lats"], z["grid_lons"], torch.device(device),
                         reg_mesh_level=level, reg_mesh_buffer=float(z["buffer"]), reg_processor_steps=steps,
                         cross_k=k, hidden_dim=hidden)


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_graph_builders_match_reference():
    from graphcast_lite_amd.dual_mesh import (build_cross_edges, build_regional_grid_mesh_edges,
                                              create_regional_mesh)

    z = _gfx()
    roi = tuple(z["roi"])
    mesh, rla, rlo = create_regional_mesh(roi, level=int(z["level"]), buffer_deg=float(z["buffer"]))
    assert len(rla) == 92
    assert np.array_equal(mesh.vertices, z["reg_vertices"]) and np.array_equal(mesh.faces, z["reg_faces"])
    assert mesh.faces.dtype == np.int32
    assert np.array_equal(rla, z["reg_lats"]) and np.array_equal(rlo, z["reg_lons"])
    cei, cef = build_cross_edges(z["global_lats"], z["global_lons"], rla, rlo, k=3)
    assert cei.dtype == torch.int64 and torch.equal(cei, torch.from_numpy(z["cross_edge_index"]))
    assert cef.dtype == torch.float32 and (cef - torch.from_numpy(z["cross_edge_features"])).abs().max() <= 1e-6
    mask, enc, dec, dist = build_regional_grid_mesh_edges(z["grid_lats"], z["grid_lons"], rla, rlo, roi)
    assert np.array_equal(np.asarray(mask), z["roi_mask"])
    assert enc.dtype == torch.int64 and torch.equal(enc, torch.from_numpy(z["enc_edges"]))
    assert dec.dtype == torch.int64 and torch.equal(dec, torch.from_numpy(z["dec_edges"]))
    assert dist.dtype == torch.float32 and (dist - torch.from_numpy(z["dec_dist"])).abs().max() <= 1e-7


def test_level_and_empty_roi_raise():
    from graphcast_lite_amd.dual_mesh import build_regional_grid_mesh_edges, create_regional_mesh

    for level in (5, 6):  # no vertex of a level <= 6 lies beyond the level-6 prefix
        with pytest.raises(ValueError):
            create_regional_mesh((50.0, 55.0, 83.0, 88.0), level=level, buffer_deg=1.0)
    lats, lons = _regular(8, 16)
    _, rla, rlo = create_regional_mesh((50.0, 55.0, 83.0, 88.0), level=7, buffer_deg=1.0)
    with pytest.raises(ValueError):
        build_regional_grid_mesh_edges(lats, lons, rla, rlo, (10.0, 11.0, 0.0, 360.0))


def test_state_dict_matches_reference():
    z = _mfx()
    m = _fx_model(z, "cpu")
    keys = sorted(k for k in m.state_dict() if not k.startswith("global_model."))
    assert keys == sorted(str(k) for k in z["sd_keys"])
    for k in keys:
        assert tuple(m.state_dict()[k].shape) == z["w:" + k].shape, k
    assert (m.dec_idw_weights - torch.from_numpy(z["dec_idw_weights"])).abs().max() <= 1e-6
    for k in ("reg_processing_edges", "cross_edge_index", "reg_encoding_edges", "reg_decoding_edges", "roi_mask"):
        assert torch.equal(m.state_dict()[k], torch.from_numpy(z["w:" + k])), k
    for k in ("reg_processing_edge_features", "cross_edge_features"):
        assert (m.state_dict()[k] - torch.from_numpy(z["w:" + k])).abs().max() <= 1e-6, k
    # the reference's best_regional.pth (every key outside global_model.) loads
    res = m.load_state_dict({k: torch.from_numpy(z["w:" + k]) for k in keys}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("global_model.") for k in res.missing_keys)
    m2 = _fx_model(z, "cpu")
    assert float(m2.reg_decoder.mlp[2].bias.abs().max()) == 0.0 and float(m2.reg_decoder.mlp[2].weight.std()) < 0.03
    assert not any(p.requires_grad for p in m2.global_model.parameters())
    assert m2.n_reg_mesh == 92 and m2.n_roi_grid == int(z["w:roi_mask"].sum())


# ------------------------------------------------------------------------------------------------------------------
# GPU: kernels
# ------------------------------------------------------------------------------------------------------------------
def _csr(dst, n):
    order = torch.sort(dst, stable=True).indices
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n), 0)
    return order, rowptr


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_segment_wsum_matches_torch(B):
    from graphcast_lite_amd import hip

    g = torch.Generator().manual_seed(30 + B)
    n_src, n, D, E = 57, 41, 36, 150
    src_i = torch.randint(0, n_src, (E,), generator=g)
    dst_i = torch.randint(0, n - 1, (E,), generator=g)          # the last destination row has an empty segment
    dst_i[dst_i == 7] = 8                                         # ... and so has row 7
    w = torch.rand(E, generator=g) + 0.1
    big = torch.randn(B, n_src + 5, D + 8, generator=g).to(DEV)
    src = big[:, 2:2 + n_src, 4:4 + D]                            # strided rows, column block
    add = torch.randn(B, n, D, generator=g).to(DEV)

    def ref(s, si, di, ww, nd, act=False):
        v = torch.nn.functional.silu(s) if act else s
        out = torch.zeros(B, nd, D, device=DEV, dtype=torch.float64)
        out.index_add_(1, di.to(DEV), (v[:, si.to(DEV)].double() * ww.to(DEV).double().view(1, -1, 1)))
        return out

    for direction in ("forward", "transposed"):
        if direction == "forward":
            si, di, nd, s_t = src_i, dst_i, n, src
        else:  # the same edges read the other way: the backward of the forward sum
            si, di, nd = dst_i, src_i, n_src
            s_t = torch.randn(B, n, D, generator=g).to(DEV)
        order, rowptr = _csr(di, nd)
        i32 = lambda t: t.to(torch.int32).to(DEV)
        idx, ww = i32(si[order]), w[order].to(DEV)
        for act in (False, True):
            out = hip.segment_wsum(s_t, idx, ww, i32(rowptr), act=hip.ACT_SILU if act else hip.ACT_NONE)
            torch.cuda.synchronize()
            r = ref(s_t, si, di, w, nd, act)
            assert (out.double() - r).abs().max().item() <= 1e-5 * (1 + r.abs().max().item()), (direction, act)
            if direction == "forward":
                assert torch.equal(out[:, 7], torch.zeros_like(out[:, 7])) and torch.equal(out[:, n - 1], out[:, 7])
    # column-block destination, addend, accumulate, and an empty segment giving the addend
    order, rowptr = _csr(dst_i, n)
    idx, ww, rp = src_i[order].to(torch.int32).to(DEV), w[order].to(DEV), rowptr.to(torch.int32).to(DEV)
    wide = torch.randn(B, n, D + 12, generator=g).to(DEV)
    keep = wide.clone()
    blk = wide[:, :, 8:8 + D]
    hip.segment_wsum(src, idx, ww, rp, out3=blk, addend3=add)
    torch.cuda.synchronize()
    r = ref(src, src_i, dst_i, w, n) + add.double()
    assert (blk.double() - r).abs().max().item() <= 1e-5 * (1 + r.abs().max().item())
    assert torch.equal(wide[:, :, :8], keep[:, :, :8]) and torch.equal(wide[:, :, 8 + D:], keep[:, :, 8 + D:])
    assert torch.equal(blk[:, 7], add[:, 7])
    before = blk.clone()
    hip.segment_wsum(src, idx, ww, rp, out3=blk, accumulate=True)
    torch.cuda.synchronize()
    r2 = before.double() + ref(src, src_i, dst_i, w, n)
    assert (blk.double() - r2).abs().max().item() <= 1e-5 * (1 + r2.abs().max().item())
    # a batch-1 source broadcasts over the destination batch
    out_b = hip.segment_wsum(src[:1], idx, ww, rp, out3=torch.empty(B, n, D, device=DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(out_b[b], out_b[0]) for b in range(B))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_cross_update_matches_torch(B):
    from graphcast_lite_amd import hip

    g = torch.Generator().manual_seed(50 + B)
    n, E = 29, 80
    for D in (32, 256):
        rcv = torch.randint(0, n - 1, (E,), generator=g)          # the last row has no message
        order, rowptr = _csr(rcv, n)
        rcv_s = rcv[order]
        big = torch.randn(B, n + 3, D + 4, generator=g).to(DEV)
        h = big[:, 1:1 + n, :D]                                    # strided regional rows
        msg = torch.randn(B, E, D, generator=g).to(DEV)
        gam = (torch.rand(D, generator=g) + 0.5).to(DEV)
        bet = torch.randn(D, generator=g).to(DEV)
        pre, y, stats = hip.cross_update_fwd(h, msg, rowptr.to(torch.int32).to(DEV), gam, bet, 1e-5)
        torch.cuda.synchronize()
        agg = torch.zeros(B, n, D, dtype=torch.float64, device=DEV).index_add_(1, rcv_s.to(DEV), msg.double())
        cnt = torch.bincount(rcv, minlength=n).clamp(min=1).to(DEV).double().view(1, n, 1)
        pre_r = h.double() + agg / cnt
        y_r = torch.nn.functional.layer_norm(pre_r, (D,), gam.double(), bet.double(), 1e-5)
        assert (pre.double() - pre_r).abs().max().item() <= 1e-5
        assert (y.double() - y_r).abs().max().item() <= 1e-4
        assert torch.equal(pre[:, n - 1], h[:, n - 1])
        assert (stats[:, 0].double() - pre_r.mean(-1).reshape(-1)).abs().max().item() <= 1e-5
        # the LayerNorm backward of the node LayerNorm takes this form unchanged
        dy = torch.randn(B, n, D, generator=g).to(DEV)
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        dpre = hip.layernorm_bwd(dy.view(-1, D), pre.view(-1, D), gam, stats, dg, db, False)
        p64 = pre_r.detach().clone().requires_grad_(True)
        g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
        torch.nn.functional.layer_norm(p64, (D,), g64, b64, 1e-5).backward(dy.double())
        assert (dpre.view(B, n, D).double() - p64.grad).abs().max().item() <= 1e-4
        assert (dg.double() - g64.grad).abs().max().item() <= 1e-3 and (db.double() - b64.grad).abs().max() <= 1e-3


# ------------------------------------------------------------------------------------------------------------------
# GPU: the regional module against the reference's fixture
# ------------------------------------------------------------------------------------------------------------------
def _fx_grads(z, kind):
    return {n: torch.from_numpy(z[f"{kind}:{n}"]) if f"{kind}:{n}" in z.files else None for n in z["param_names"]}


@pytest.mark.gpu
def test_regional_module_matches_reference_fixture():
    """Fixture weights loaded from a reference-layout state dict (strict=False), the fixture's global outputs injected
    through a stub: output, cached output and every regional gradient against the reference module, by the
    fp64-arbitrated rule."""
    z = _mfx()
    m = _fx_model(z, DEV)
    keys = [str(k) for k in z["sd_keys"]]
    res = m.load_state_dict({k: torch.from_numpy(z["w:" + k]) for k in keys}, strict=False)
    assert not res.unexpected_keys
    X, y = torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    out = m(X)
    assert out.shape == tuple(z["out32"].shape)
    mask = m.roi_mask
    ((out.unsqueeze(0)[:, mask] - y[:, mask]) ** 2).mean().backward()
    check_grads({"out": out.detach()}, {"out": torch.from_numpy(z["out32"])}, {"out": torch.from_numpy(z["out64"])},
                tag="dual-mesh output")
    hip_g = {n: (None if p.grad is None else p.grad.detach()) for n, p in m.named_parameters()
             if not n.startswith("global_model.")}
    check_grads(hip_g, _fx_grads(z, "g32"), _fx_grads(z, "g64"), tag="dual-mesh regional gradients")
    assert m.global_model.dummy.grad is None
    # rows outside the ROI are the global prediction, bit for bit
    assert torch.equal(out.detach()[~mask], m.global_model.pred[~mask])
    # precompute_global: the reference's keys and shapes, CPU tensors; forward_cached == forward's ROI rows
    c = m.precompute_global(X)
    assert sorted(c) == sorted(str(k) for k in z["cache_keys"])
    for k, v in c.items():
        assert v.device.type == "cpu" and tuple(v.shape) == tuple(z["cache_shape:" + k]), k
    with torch.no_grad():
        cached = m.forward_cached(X[0][mask], *(c[k].to(DEV) for k in ("global_pred_roi", "roi_grid_latent",
                                                                       "cross_sender_feat")))
    assert torch.equal(cached, out.detach()[mask])
    assert (cached.cpu() - torch.from_numpy(z["cached32"])).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------------------------------------------
# GPU: the shared processor step
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("preset", [False, True])
def test_shared_step_gradients_sum_over_steps(preset):
    """RegionalProcessor (one step applied num_steps times) against an oracle of num_steps independent copies of that
    step: every gradient of the shared step is the sum over the copies, with p.grad unset (autograd sums the slots)
    and with p.grad preinstalled (every slot accumulates into it)."""
    from oracle.model import OInteractionNetProcessor

    from graphcast_lite_amd.dual_mesh import RegionalProcessor, create_regional_mesh
    from graphcast_lite_amd.mesh import get_edges_from_faces
    from graphcast_lite_amd.utils import mesh_edge_features

    H, steps = 32, 3
    mesh, rla, rlo = create_regional_mesh((50.0, 55.0, 83.0, 88.0), level=7, buffer_deg=1.0)
    ei = torch.tensor(get_edges_from_faces(mesh.faces), dtype=torch.int64)
    ef = torch.from_numpy(mesh_edge_features(rla, rlo, ei.numpy()))
    torch.manual_seed(3)
    p = RegionalProcessor(H, 4, H, steps).to(DEV)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for ln in (p.step.edge_norm, p.step.node_norm):
            ln.weight.copy_(0.5 + torch.rand(H, generator=g))
            ln.bias.copy_(0.1 * torch.randn(H, generator=g))
    o = OInteractionNetProcessor(H, 4, H, H, steps)
    sd = {"edge_encoder.0." + k: v.cpu() for k, v in p.edge_encoder[0].state_dict().items()}
    for i in range(steps):
        sd.update({f"steps.{i}.{k}": v.cpu() for k, v in p.step.state_dict().items()})
    o.load_state_dict(sd)
    n = len(rla)
    x = torch.randn(n, H, generator=g)
    wout = torch.randn(n, H, generator=g)
    base = {}
    if preset:
        for name, q in p.named_parameters():
            base[name] = torch.randn(q.shape, generator=g).to(DEV)
            q.grad = base[name].clone()
    out = p(x.to(DEV), ei.to(DEV), ef.to(DEV))
    (out * wout.to(DEV)).sum().backward()

    def unrolled(oo, dt):
        for q in oo.parameters():
            q.grad = None
        r = oo(x.to(dt), ei, ef.to(dt))
        (r * wout.to(dt)).sum().backward()
        gr = {"edge_encoder.0.weight": oo.edge_encoder[0].weight.grad, "edge_encoder.0.bias": oo.edge_encoder[0].bias.grad}
        for name, _ in p.step.named_parameters():
            gs = [dict(st.named_parameters())[name].grad for st in oo.steps]
            gs = [t for t in gs if t is not None]
            gr["step." + name] = sum(gs) if gs else None
        return r.detach(), gr

    r32, g32 = unrolled(o, torch.float32)
    o64 = copy.deepcopy(o).double()
    r64, g64 = unrolled(o64, torch.float64)
    check_grads({"out": out.detach()}, {"out": r32}, {"out": r64}, tag="shared-step output")
    hip_g = {}
    for name, q in p.named_parameters():
        gq = q.grad.detach()
        hip_g[name] = gq - base[name] if preset else gq
    check_grads(hip_g, g32, g64, tag=f"shared-step gradients (preset={preset})")


# ------------------------------------------------------------------------------------------------------------------
# GPU: whole model against a composed CPU oracle
# ------------------------------------------------------------------------------------------------------------------
def _scatter_rows(src, index, n, mean):
    out = torch.zeros(src.shape[:-2] + (n, src.shape[-1]), dtype=src.dtype).index_add(-2, index, src)
    if not mean:
        return out
    cnt = torch.bincount(index, minlength=n).clamp(min=1).to(src.dtype)
    return out / cnt.view(-1, 1)


class _Holder(nn.Module):
    pass


class ODual(nn.Module):
    """src/dual_mesh.py:663-727 in plain torch over the oracle's WeatherPrediction and InteractionNet step, one sample
    at a time (the reference asserts B == 1)."""

    def __init__(self, og, m):
        from oracle.model import OInteractionNetLayer, OLayerNorm

        super().__init__()
        self.og = og
        H, S, C, Dg = m.reg_encoder.mlp[0].weight.shape[0], m.reg_enc_input_dim, m.output_channels, m.global_latent_dim
        self.reg_encoder = _Holder()
        self.reg_encoder.mlp = nn.Sequential(nn.Linear(S, H), nn.SiLU(), nn.Linear(H, H))
        self.reg_processor = _Holder()
        self.reg_processor.edge_encoder = nn.Sequential(nn.Linear(4, H), nn.SiLU())
        self.reg_processor.step = OInteractionNetLayer(H, H, H, "swish", True)
        self.cross_message = _Holder()
        self.cross_message.g2r_edge_mlp = nn.Sequential(nn.Linear(Dg + 2 * H, H), nn.SiLU(), nn.Linear(H, H))
        self.cross_message.norm_reg = OLayerNorm(H, mode="node")
        self.cross_edge_encoder = nn.Sequential(nn.Linear(4, H), nn.SiLU())
        self.reg_decoder = _Holder()
        self.reg_decoder.mlp = nn.Sequential(nn.Linear(H + S, H), nn.SiLU(), nn.Linear(H, C))
        own = {k: v.cpu() for k, v in m.state_dict().items() if not k.startswith("global_model.")}
        res = self.load_state_dict(own, strict=False)
        assert not [k for k in res.missing_keys if not k.startswith("og.")], res.missing_keys
        self.steps = m.reg_processor.num_steps
        self.mask, self.idx = m.roi_mask.cpu(), torch.where(m.roi_mask.cpu())[0]
        self.n_reg, self.n_roi = m.n_reg_mesh, m.n_roi_grid
        for k in ("reg_processing_edges", "reg_processing_edge_features", "cross_edge_index", "cross_edge_features",
                  "reg_encoding_edges", "reg_decoding_edges", "dec_idw_weights"):
            setattr(self, "_" + k, getattr(m, k).cpu())

    def regional(self, roi_input, mesh_lat_senders):
        dt = roi_input.dtype
        enc = self._reg_encoding_edges
        h = _scatter_rows(self.reg_encoder.mlp(roi_input)[enc[0]], enc[1], self.n_reg, True)
        half = self._cross_edge_index.shape[1] // 2
        rcv = self._cross_edge_index[1, :half]
        ce = self.cross_edge_encoder(self._cross_edge_features.to(dt))[:half]
        msg = self.cross_message.g2r_edge_mlp(torch.cat([mesh_lat_senders, h[rcv], ce], dim=-1))
        h = self.cross_message.norm_reg(h + _scatter_rows(msg, rcv, self.n_reg, True))
        e = self.reg_processor.edge_encoder(self._reg_processing_edge_features.to(dt))
        for _ in range(self.steps):
            h, e = self.reg_processor.step(h, self._reg_processing_edges, e)
        dec = self._reg_decoding_edges
        agg = _scatter_rows(h[dec[0]] * self._dec_idw_weights.to(dt).unsqueeze(-1), dec[1], self.n_roi, False)
        return self.reg_decoder.mlp(torch.cat([agg, roi_input], dim=-1))

    def global_parts(self, X1):
        with torch.no_grad():
            pred, lat, mesh = self.og.forward_with_latents(X1)
        half = self._cross_edge_index.shape[1] // 2
        return pred, lat, mesh[self._cross_edge_index[0, :half]]

    def forward(self, X):
        X3 = X if X.dim() == 3 else X.unsqueeze(0)
        outs = []
        for b in range(X3.shape[0]):
            pred, lat, send = self.global_parts(X3[b:b + 1])
            roi_input = torch.cat([X3[b][self.mask], lat[self.mask]], dim=-1)
            outs.append(pred.index_add(0, self.idx, self.regional(roi_input, send)))
        out = torch.stack(outs)
        return out[0] if out.shape[0] == 1 else out


def _oracle64(o):
    o64 = copy.deepcopy(o).double()
    o64.og = oracle_fp64(o.og)
    return o64


ROI = (20.0, 40.0, 30.0, 60.0)


def _pair(name, hidden=32, steps=2, seed=42):
    from graphcast_lite_amd.dual_mesh import DualMeshModel
    from test_hip_model import make_pair

    cfg, m, o = make_pair(name, [1, 2], seed=seed)
    lats, lons = _regular(32, 64)
    torch.manual_seed(seed + 7)
    r = DualMeshModel(m, ROI, lats, lons, torch.device(DEV), reg_mesh_level=7, reg_mesh_buffer=1.0,
                      reg_processor_steps=steps, cross_k=3, hidden_dim=hidden)
    g = torch.Generator().manual_seed(seed + 9)
    with torch.no_grad():  # off the decoder's near-zero start, so that the correction and every gradient matter
        r.reg_decoder.mlp[2].weight.copy_(0.2 * torch.randn(r.reg_decoder.mlp[2].weight.shape, generator=g))
        for ln in (r.reg_processor.step.node_norm, r.reg_processor.step.edge_norm, r.cross_message.norm_reg):
            ln.bias.copy_(0.1 * torch.randn(ln.bias.shape, generator=g))
    return cfg, r, ODual(o, r)


def _data(cfg, G, B, seed=1234):
    g = torch.Generator().manual_seed(seed)
    Fe, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    return torch.randn(B, G, obs * Fe, generator=g), torch.randn(B, G, Fe, generator=g)


def _roi_loss(out, y, idx):
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    return ((o3[:, idx] - y[:, idx]) ** 2).mean()


def _own(mod, skip):
    return {n: (None if p.grad is None else p.grad.detach()) for n, p in mod.named_parameters() if not n.startswith(skip)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["baseline", "region_krsk_cds_19f"])
def test_whole_model_matches_oracle(name):
    """GCN global (compact pipeline) and InteractionNet global: output, regional gradients, rows outside the ROI and
    frozen global parameters."""
    from graphcast_lite_amd.train import batch_loss

    cfg, r, o = _pair(name)
    gm = r.global_model
    G = gm._num_grid_nodes
    X, y = _data(cfg, G, 1)
    Xd, yd = X.to(DEV), y.to(DEV)
    out = r(Xd)
    out_o = o(X)
    assert out.shape == out_o.shape == (G, cfg.data.num_features_used)
    idx = o.idx
    mask3 = r.roi_mask.view(1, -1, 1).float()
    loss = batch_loss(r, Xd, yd, spatial_mask=mask3, use_residual=False)
    loss_o = _roi_loss(out_o, y, idx)
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) <= 1e-5 * abs(loss_o.item())
    loss.backward()
    o64 = _oracle64(o)
    out64 = o64(X.double())
    _roi_loss(out64, y.double(), idx).backward()
    check_grads({"out": out.detach()}, {"out": out_o.detach()}, {"out": out64.detach()}, tag=f"{name} dual output")
    check_grads(_own(r, "global_model."), _own(o, "og."), _own(o64, "og."), tag=f"{name} dual gradients")
    assert all(p.grad is None for p in gm.parameters())
    with torch.no_grad():
        glob = gm(Xd)
    assert torch.equal(out.detach()[~r.roi_mask], glob[~r.roi_mask])


@pytest.mark.gpu
def test_batch_is_per_sample_and_cached_matches_forward():
    from graphcast_lite_amd.train import batch_loss

    cfg, r, _ = _pair("baseline")
    G = r.global_model._num_grid_nodes
    X, y = _data(cfg, G, 3)
    Xd, yd = X.to(DEV), y.to(DEV)
    mask3 = r.roi_mask.view(1, -1, 1).float()
    out3 = r(Xd)
    assert out3.shape == (3, G, cfg.data.num_features_used)
    batch_loss(r, Xd, yd, spatial_mask=mask3, use_residual=False).backward()
    g3 = {n: p.grad.clone() for n, p in r.named_parameters() if p.grad is not None}
    r.zero_grad(set_to_none=True)
    for b in range(3):
        out1 = r(Xd[b:b + 1])
        assert torch.allclose(out1, out3[b], rtol=1e-5, atol=1e-6)
        with torch.no_grad():
            glob = r.global_model(Xd[b:b + 1])
        assert torch.equal(out3[b].detach()[~r.roi_mask], glob[~r.roi_mask])
        (batch_loss(r, Xd[b:b + 1], yd[b:b + 1], spatial_mask=mask3, use_residual=False) / 3).backward()
    for n, p in r.named_parameters():
        if n in g3:
            rel = ((p.grad - g3[n]).norm() / (g3[n].norm() + 1e-30)).item()
            assert rel < 1e-4, (n, rel)
    # precompute_global -> CPU tensors with the reference's keys and shapes; forward_cached == forward's ROI rows
    mask = r.roi_mask
    c1 = r.precompute_global(Xd[:1])
    half = r.cross_edge_index.shape[1] // 2
    D = r.global_latent_dim
    shapes = {"global_pred_roi": (r.n_roi_grid, cfg.data.num_features_used), "roi_grid_latent": (r.n_roi_grid, D),
              "cross_sender_feat": (half, D)}
    assert sorted(c1) == sorted(shapes)
    for k, v in c1.items():
        assert v.device.type == "cpu" and tuple(v.shape) == shapes[k], k
    with torch.no_grad():
        oc = r.forward_cached(Xd[0][mask], *(c1[k].to(DEV) for k in ("global_pred_roi", "roi_grid_latent",
                                                                     "cross_sender_feat")))
        assert torch.equal(oc, r(Xd[:1])[mask])
        cb = r.precompute_global(Xd)
        for k, v in cb.items():
            assert tuple(v.shape) == (3,) + shapes[k], k
        ocb = r.forward_cached(Xd[:, mask], *(cb[k].to(DEV) for k in ("global_pred_roi", "roi_grid_latent",
                                                                      "cross_sender_feat")))
        assert torch.equal(ocb, out3.detach()[:, mask])


@pytest.mark.gpu
def test_train_step_full_mode_captured_eager_and_oracle_adam():
    from graphcast_lite_amd.train import TrainStep

    cfg, r1, o = _pair("baseline", seed=5)
    _, r2, _ = _pair("baseline", seed=5)
    G = r1.global_model._num_grid_nodes
    X, y = _data(cfg, G, 1, seed=77)
    Xd, yd = X.to(DEV), y.to(DEV)
    mask3 = r1.roi_mask.view(1, -1, 1).float()
    gsnap = {n: p.detach().clone() for n, p in r1.global_model.named_parameters()}
    s1 = TrainStep(r1, lr=1e-3, spatial_mask=mask3, use_residual=False, use_graph=True)
    s2 = TrainStep(r2, lr=1e-3, spatial_mask=mask3, use_residual=False, use_graph=False)
    assert s1.flat.num_params == sum(p.numel() for n, p in r1.named_parameters() if not n.startswith("global_model."))
    opt = torch.optim.Adam([p for n, p in o.named_parameters() if not n.startswith("og.")], lr=1e-3)
    for i in range(4):
        l1, l2 = s1(Xd, yd), s2(Xd, yd)
        opt.zero_grad()
        lo = _roi_loss(o(X), y, o.idx)
        lo.backward()
        opt.step()
        assert abs(l1.item() - l2.item()) <= 1e-6 * abs(l2.item()), (i, l1.item(), l2.item())
        assert abs(l1.item() - lo.item()) <= 1e-4 * abs(lo.item()), (i, l1.item(), lo.item())
    assert s1.graph_active
    od = dict(o.named_parameters())
    for n, p in r1.named_parameters():
        if n.startswith("global_model."):
            continue
        p2 = dict(r2.named_parameters())[n]
        ref = od[n].detach().double()
        assert (p.detach().cpu().double() - ref).norm().item() <= 1e-4 * ref.norm().item(), n
        assert (p.detach() - p2.detach()).norm().item() <= 1e-5 * p2.detach().norm().item(), n
    for n, p in r1.global_model.named_parameters():
        assert torch.equal(p.detach(), gsnap[n]), n
        assert p.grad is None


@pytest.mark.gpu
def test_train_step_ar2_eager_against_oracle():
    """The reference's standard mode with ar_steps = 2 (scripts/train_dual_mesh.py:195-230): the prediction is fed
    back through the window, the loss is the mean of the per-step ROI losses."""
    from graphcast_lite_amd.train import TrainStep

    cfg, r, o = _pair("baseline", seed=8)
    G = r.global_model._num_grid_nodes
    Fe, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    g = torch.Generator().manual_seed(5)
    X = torch.randn(1, G, obs * Fe, generator=g)
    y = torch.randn(1, G, 2 * Fe, generator=g)
    mask3 = r.roi_mask.view(1, -1, 1).float()
    s = TrainStep(r, lr=1e-3, spatial_mask=mask3, use_residual=True, ar_steps=2, use_graph=False)
    opt = torch.optim.Adam([p for n, p in o.named_parameters() if not n.startswith("og.")], lr=1e-3)
    for i in range(2):
        ls = s(X.to(DEV), y.to(DEV))
        opt.zero_grad()
        state = X.view(1, G, obs, Fe)
        lo = 0.0
        for k in range(2):
            pred = o(state.view(1, G, -1)).unsqueeze(0) + state[:, :, -1, :]
            lo = lo + _roi_loss(pred, y[:, :, k * Fe:(k + 1) * Fe], o.idx)
            state = torch.cat([state[:, :, 1:, :], pred.unsqueeze(2)], dim=2)
        lo = lo / 2
        lo.backward()
        opt.step()
        assert abs(ls.item() - lo.item()) <= 1e-4 * abs(lo.item()), (i, ls.item(), lo.item())
    od = dict(o.named_parameters())
    for n, p in r.named_parameters():
        if not n.startswith("global_model."):
            ref = od[n].detach().double()
            assert (p.detach().cpu().double() - ref).norm().item() <= 1e-4 * ref.norm().item(), n


@pytest.mark.gpu
@pytest.mark.parametrize("use_residual", [False, True])
def test_cached_step_captured_eager_and_oracle(use_residual):
    from graphcast_lite_amd.dual_mesh import DualMeshCachedStep

    cfg, r1, o = _pair("baseline", seed=6)
    _, r2, _ = _pair("baseline", seed=6)
    G = r1.global_model._num_grid_nodes
    C = cfg.data.num_features_used
    mask = r1.roi_mask
    samples = []
    for sd in (11, 12):
        X, y = _data(cfg, G, 1, seed=sd)
        c = r1.precompute_global(X.to(DEV))
        samples.append((X[0][mask.cpu()], c, y[0][mask.cpu()]))
    s1 = DualMeshCachedStep(r1, lr=1e-3, use_residual=use_residual, use_graph=True)
    s2 = DualMeshCachedStep(r2, lr=1e-3, use_residual=use_residual, use_graph=False)
    opt = torch.optim.Adam([p for n, p in o.named_parameters() if not n.startswith("og.")], lr=1e-3)
    keys = ("global_pred_roi", "roi_grid_latent", "cross_sender_feat")
    for i in range(5):
        raw, c, y = samples[i % 2]
        l1 = s1(raw, *(c[k] for k in keys), y)
        l2 = s2(raw, *(c[k] for k in keys), y)
        opt.zero_grad()
        out = c["global_pred_roi"] + o.regional(torch.cat([raw, c["roi_grid_latent"]], -1), c["cross_sender_feat"])
        if use_residual:
            out = raw[:, -C:] + out
        lo = ((out - y) ** 2).mean()
        lo.backward()
        opt.step()
        assert abs(l1.item() - l2.item()) <= 1e-6 * abs(l2.item()), (i, l1.item(), l2.item())
        assert abs(l1.item() - lo.item()) <= 1e-4 * abs(lo.item()), (i, l1.item(), lo.item())
    assert s1.graph_active and not s2.graph_active
    od = dict(o.named_parameters())
    for n, p in r1.named_parameters():
        if n.startswith("global_model."):
            continue
        p2 = dict(r2.named_parameters())[n]
        ref = od[n].detach().double()
        assert (p.detach().cpu().double() - ref).norm().item() <= 1e-4 * ref.norm().item(), n
        assert (p.detach() - p2.detach()).norm().item() <= 1e-5 * p2.detach().norm().item(), n
    assert all(p.grad is None for p in r1.global_model.parameters())
