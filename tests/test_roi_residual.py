"""ROI residual head (`src/roi_residual.py`): the kNN graph builder against the reference's own output, the two glue
kernels against torch indexing, the head against the reference module's fixture, and the whole model (frozen global +
head) against a CPU oracle composed here - forward, gradients and training steps."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN
from parity import check_grads, oracle_fp64

DEV = "cuda:0"
KNN_CASES = ("box", "flat", "three", "one")


def _knn():
    return np.load(os.path.join(GOLDEN, "roi_knn_vectors.npz"))


def _head_fx():
    return np.load(os.path.join(GOLDEN, "roi_head_vectors.npz"))


def _regular(nlat, nlon):
    lats = np.linspace(-90, 90, nlat, endpoint=True)
    lons = np.linspace(0, 360, nlon, endpoint=False)
    lon_grid, lat_grid = np.meshgrid(lons, lats)
    return lat_grid.flatten().astype(np.float32), lon_grid.flatten().astype(np.float32)


class StubGlobal(nn.Module):
    """A frozen 'global model' with fixed outputs: what ROIResidualModel reads from WeatherPrediction."""

    def __init__(self, pred, lat, obs):
        super().__init__()
        self.num_features, self.obs_window = pred.shape[-1], obs
        self.register_buffer("pred", pred)
        self.register_buffer("lat", lat)
        self.dummy = nn.Parameter(torch.zeros(1))  # a global parameter, frozen by the ROI model
        self.encoder = type("Enc", (), {"output_dim": lat.shape[-1]})()

    def forward_with_latents(self, X, attention_threshold=0.0, **kw):
        return self.pred, self.lat, None


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KNN_CASES)
def test_knn_graph_matches_reference(case):
    from graphcast_lite_amd.roi_residual import build_roi_knn_graph

    z = _knn()
    mask, idx, ei, ef = build_roi_knn_graph(z[f"{case}_lats"], z[f"{case}_lons"], tuple(z[f"{case}_roi"]),
                                            k=int(z[f"{case}_k"]))
    assert torch.equal(torch.from_numpy(np.asarray(mask)), torch.from_numpy(z[f"{case}_mask"]))
    assert torch.equal(torch.from_numpy(np.asarray(idx, np.int64)), torch.from_numpy(z[f"{case}_indices"]))
    assert ei.dtype == torch.int64 and torch.equal(ei, torch.from_numpy(z[f"{case}_edge_index"]))
    ref = torch.from_numpy(z[f"{case}_edge_features"])
    assert ef.dtype == torch.float32 and ef.shape == ref.shape
    if ref.numel():
        assert (ef - ref).abs().max().item() <= 1e-6
    if case == "one":
        assert ei.shape == (2, 0)


def test_empty_roi_raises():
    from graphcast_lite_amd.roi_residual import build_roi_knn_graph

    lats, lons = _regular(8, 16)
    with pytest.raises(ValueError):
        build_roi_knn_graph(lats, lons, (10.0, 11.0, 0.0, 360.0))


def _cpu_model(z):
    from graphcast_lite_amd.roi_residual import ROIResidualModel

    Fe, obs, D, hidden, steps, k = (int(v) for v in z["dims"])
    stub = StubGlobal(torch.from_numpy(z["pred"]), torch.from_numpy(z["lat"]), obs)
    return ROIResidualModel(stub, tuple(z["roi"]), z["grid_lats"], z["grid_lons"], torch.device("cpu"),
                            hidden_dim=hidden, processor_steps=steps, roi_k=k)


def test_head_state_dict_keys_match_reference():
    z = _head_fx()
    m = _cpu_model(z)
    head = sorted(k for k in m.state_dict() if not k.startswith("global_model."))
    assert head == sorted(str(k) for k in z["head_keys"])
    for k in head:
        assert tuple(m.state_dict()[k].shape) == z["w:" + k].shape, k
    # the reference's best_head.pth (every key outside global_model.) loads
    res = m.load_state_dict({k: torch.from_numpy(z["w:" + k]) for k in head}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("global_model.") for k in res.missing_keys)
    # the last Linear starts at normal(std=0.01) weights and a zero bias; the global model is frozen
    m2 = _cpu_model(z)
    assert float(m2.decoder.mlp[4].bias.abs().max()) == 0.0 and float(m2.decoder.mlp[4].weight.std()) < 0.03
    assert not any(p.requires_grad for p in m2.global_model.parameters())
    assert m2.skip_dim == z["dims"][0] * z["dims"][1] + z["dims"][2] + z["dims"][0]


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
def test_glue_kernels_match_torch_indexing(B):
    from graphcast_lite_amd import hip

    G, Fx, D, Cc = 83, 7, 13, 5       # skip width 25: not a multiple of 4
    g = torch.Generator().manual_seed(3 + B)
    rows = torch.cat([torch.tensor([0, G - 1]), torch.randperm(G - 2, generator=g)[:35] + 1])  # n = 37
    n = rows.numel()
    X = torch.randn(B, G, Fx, generator=g).to(DEV)
    big = torch.randn(B, G + 9, D + 3, generator=g).to(DEV)
    lat = big[:, 3:3 + G, 2:2 + D]                                   # a column block inside a wider buffer
    predw = torch.randn(B, G, 8, generator=g).to(DEV)
    pred_strided = predw[..., :Cc]
    pred = predw[..., :Cc].contiguous()
    r32 = rows.to(torch.int32).to(DEV)
    Sp = 28
    skip = hip.roi_gather_rows(r32, G, [X, lat, pred_strided], Sp, B)
    torch.cuda.synchronize()
    ri = rows.to(DEV)
    ref = torch.cat([X[:, ri], lat[:, ri], pred_strided[:, ri], torch.zeros(B, n, Sp - Fx - D - Cc, device=DEV)], -1)
    assert torch.equal(skip, ref)

    pos = torch.full((G,), -1, dtype=torch.int32)
    pos[rows] = torch.arange(n, dtype=torch.int32)
    pos = pos.to(DEV)
    corr = torch.randn(B, n, 8, generator=g).to(DEV)
    inroi = torch.zeros(G, dtype=torch.bool, device=DEV)
    inroi[ri] = True
    for p in (pred, pred_strided):  # dense (16-byte quads, partial last quad) and strided source
        out = hip.roi_compose(p, corr, pos)
        exp = p.clone()
        exp[:, ri] = p[:, ri] + corr[..., :Cc]
        torch.cuda.synchronize()
        assert torch.equal(out, exp)
        assert torch.equal(out[:, ~inroi], p[:, ~inroi])

    dout = torch.randn(B, G, Cc, generator=g).to(DEV)
    d = hip.roi_gather_rows(r32, G, [dout], 8, B)
    torch.cuda.synchronize()
    assert torch.equal(d, torch.cat([dout[:, ri], torch.zeros(B, n, 3, device=DEV)], -1))


def _fx_grads(z, kind):
    return {n: torch.from_numpy(z[f"{kind}:{n}"]) if f"{kind}:{n}" in z.files else None for n in z["param_names"]}


@pytest.mark.gpu
def test_head_matches_reference_fixture():
    """Fixture weights and inputs, the fixture's global outputs injected through a stub: output and head gradients
    against the reference module (fp32 and fp64 runs of it), by the fp64-arbitrated rule."""
    from graphcast_lite_amd.roi_residual import ROIResidualModel

    z = _head_fx()
    Fe, obs, D, hidden, steps, k = (int(v) for v in z["dims"])
    stub = StubGlobal(torch.from_numpy(z["pred"]), torch.from_numpy(z["lat"]), obs)
    m = ROIResidualModel(stub, tuple(z["roi"]), z["grid_lats"], z["grid_lons"], torch.device(DEV), hidden_dim=hidden,
                         processor_steps=steps, roi_k=k)
    m.load_state_dict({k_: torch.from_numpy(z["w:" + k_]) for k_ in z["head_keys"]}, strict=False)
    X, y = torch.from_numpy(z["X"]).to(DEV), torch.from_numpy(z["y"]).to(DEV)
    out = m(X)
    assert out.shape == tuple(z["out32"].shape)
    mask = m.roi_mask
    loss = ((out.unsqueeze(0)[:, mask] - y[:, mask]) ** 2).mean()
    loss.backward()
    check_grads({"out": out.detach()}, {"out": torch.from_numpy(z["out32"])}, {"out": torch.from_numpy(z["out64"])},
                tag="roi head output")
    hip_g = {n: (None if p.grad is None else p.grad.detach()) for n, p in m.named_parameters()
             if not n.startswith("global_model.")}
    check_grads(hip_g, _fx_grads(z, "g32"), _fx_grads(z, "g64"), tag="roi head gradients")
    assert stub.dummy.grad is None


# --- whole model against a composed CPU oracle ----------------------------------------------------------------------
class OHead(nn.Module):
    def __init__(self, i, h, o):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(i, h), nn.SiLU(), nn.Linear(h, h), nn.SiLU(), nn.Linear(h, o))


class OROI(nn.Module):
    """src/roi_residual.py:158-185 in plain torch over the oracle's WeatherPrediction and InteractionNet processor."""

    def __init__(self, og, m):
        from oracle.model import OInteractionNetProcessor

        super().__init__()
        self.og = og
        H, S, C = m.input_proj[0].weight.shape[0], m.skip_dim, m.output_channels
        self.input_proj = nn.Sequential(nn.Linear(S, H), nn.SiLU(), nn.Linear(H, H))
        self.processor = OInteractionNetProcessor(H, 4, H, H, len(m.processor.steps))
        self.decoder = OHead(H + S, H, C)
        for name in ("input_proj", "processor", "decoder"):
            getattr(self, name).load_state_dict({k: v.cpu() for k, v in getattr(m, name).state_dict().items()})
        self.idx = m.roi_indices.cpu()
        self.ei, self.ef = m.roi_edge_index.cpu(), m.roi_edge_features.cpu()

    def forward(self, X):
        with torch.no_grad():
            pred, lat, _ = self.og.forward_with_latents(X)
        if pred.dim() == 2:
            pred, lat = pred.unsqueeze(0), lat.unsqueeze(0)
        X3 = X if X.dim() == 3 else X.unsqueeze(0)
        skip = torch.cat([X3[:, self.idx], lat[:, self.idx], pred[:, self.idx]], dim=-1)
        h = self.processor(self.input_proj(skip), self.ei, self.ef.to(X.dtype))
        corr = self.decoder.mlp(torch.cat([h, skip], dim=-1))
        out = pred.index_add(1, self.idx, corr)
        return out[0] if out.shape[0] == 1 else out


def _oracle64(o):
    o64 = copy.deepcopy(o).double()
    og64 = oracle_fp64(o.og)
    o64.og = og64
    return o64


def _pair(name, hidden=32, steps=2, seed=42):
    from graphcast_lite_amd.roi_residual import ROIResidualModel
    from test_hip_model import make_pair

    cfg, m, o = make_pair(name, [1, 2], seed=seed)
    lats, lons = _regular(32, 64)
    torch.manual_seed(seed + 7)
    r = ROIResidualModel(m, (20.0, 60.0, 30.0, 100.0), lats, lons, torch.device(DEV), hidden_dim=hidden,
                         processor_steps=steps, roi_k=8)
    g = torch.Generator().manual_seed(seed + 9)
    with torch.no_grad():  # off the head's near-zero start, so that the correction and every gradient matter
        r.decoder.mlp[4].weight.copy_(0.2 * torch.randn(r.decoder.mlp[4].weight.shape, generator=g))
        for st in r.processor.steps:
            st.node_norm.bias.copy_(0.1 * torch.randn(st.node_norm.bias.shape, generator=g))
    return cfg, r, OROI(o, r)


def _data(cfg, G, B, seed=1234):
    g = torch.Generator().manual_seed(seed)
    Fe, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    X = torch.randn(B, G, obs * Fe, generator=g)
    return X, torch.randn(B, G, Fe, generator=g)


def _roi_loss(out, y, idx):
    o3 = out if out.dim() == 3 else out.unsqueeze(0)
    return ((o3[:, idx] - y[:, idx]) ** 2).mean()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["baseline", "region_krsk_cds_19f"])
def test_whole_model_matches_oracle(name):
    """GCN global (compact pipeline) and InteractionNet global: output, head gradients, rows outside the ROI, frozen
    global parameters, and the latents forward_with_latents hands over vs the reference's second encoder pass."""
    from graphcast_lite_amd.train import batch_loss

    cfg, r, o = _pair(name)
    gm = r.global_model
    G = gm._num_grid_nodes
    X, y = _data(cfg, G, 1)
    Xd, yd = X.to(DEV), y.to(DEV)
    out = r(Xd)
    out_o = o(X)
    assert out.shape == out_o.shape == (G, cfg.data.num_features_used)
    idx = r.roi_indices.cpu()
    mask3 = r.roi_mask.view(1, -1, 1).float()
    loss = batch_loss(r, Xd, yd, spatial_mask=mask3, use_residual=False)
    loss_o = _roi_loss(out_o, y, idx)
    loss_o.backward()
    assert abs(loss.item() - loss_o.item()) <= 1e-5 * abs(loss_o.item())
    loss.backward()
    o64 = _oracle64(o)
    out64 = o64(X.double())
    _roi_loss(out64, y.double(), idx).backward()
    check_grads({"out": out.detach()}, {"out": out_o.detach()}, {"out": out64.detach()}, tag=f"{name} roi output")
    head = lambda mod, skip: {n: (None if p.grad is None else p.grad.detach()) for n, p in mod.named_parameters()
                              if not n.startswith(skip)}
    check_grads(head(r, "global_model."), head(o, "og."), head(o64, "og."), tag=f"{name} roi gradients")
    assert all(p.grad is None for p in gm.parameters())
    # rows outside the ROI are the global model's own forward, bit for bit
    with torch.no_grad():
        glob = gm(Xd)
    outside = ~r.roi_mask
    assert torch.equal(out.detach()[outside], glob[outside])
    # forward_with_latents' grid latents == the reference's second pass (_preprocess_input -> encoder.forward)
    with torch.no_grad():
        _, lat, _ = gm.forward_with_latents(Xd)
        enc = gm.encoder.forward(X=gm._preprocess_input(grid_node_features=Xd[0]), edge_index=gm.encoding_graph)
    ref_lat = enc[:G]
    err = ((lat - ref_lat).norm() / ref_lat.norm()).item()
    assert err < 1e-6, err


@pytest.mark.gpu
def test_batch_is_per_sample():
    from graphcast_lite_amd.train import batch_loss

    cfg, r, _ = _pair("baseline")
    G = r.global_model._num_grid_nodes
    X, y = _data(cfg, G, 2)
    Xd, yd = X.to(DEV), y.to(DEV)
    mask3 = r.roi_mask.view(1, -1, 1).float()
    out2 = r(Xd)
    assert out2.shape == (2, G, cfg.data.num_features_used)
    loss2 = batch_loss(r, Xd, yd, spatial_mask=mask3, use_residual=False)
    loss2.backward()
    g2 = {n: p.grad.clone() for n, p in r.named_parameters() if p.grad is not None}
    r.zero_grad(set_to_none=True)
    acc = {}
    for b in range(2):
        out1 = r(Xd[b:b + 1])
        assert torch.allclose(out1, out2[b], rtol=1e-5, atol=1e-6)
        (0.5 * batch_loss(r, Xd[b:b + 1], yd[b:b + 1], spatial_mask=mask3, use_residual=False)).backward()
    for n, p in r.named_parameters():
        if n in g2:
            rel = ((p.grad - g2[n]).norm() / (g2[n].norm() + 1e-30)).item()
            assert rel < 1e-4, (n, rel)


@pytest.mark.gpu
def test_train_step_captured_eager_and_oracle_adam(tmp_path):
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
    assert all(not n.startswith("global_model.") for n, p in r1.named_parameters() if any(p is q for q in s1.flat.params))
    assert s1.flat.num_params == sum(p.numel() for n, p in r1.named_parameters() if not n.startswith("global_model."))
    head_o = [p for n, p in o.named_parameters() if not n.startswith("og.")]
    opt = torch.optim.Adam(head_o, lr=1e-3)
    idx = r1.roi_indices.cpu()
    for i in range(3):
        l1, l2 = s1(Xd, yd), s2(Xd, yd)
        opt.zero_grad()
        lo = _roi_loss(o(X), y, idx)
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
        ref = od[n].detach().double()  # (the last step's edge LayerNorm never gets a gradient: it may stay all zero)
        assert (p.detach().cpu().double() - ref).norm().item() <= 1e-4 * ref.norm().item(), n
        assert (p.detach() - p2.detach()).norm().item() <= 1e-5 * p2.detach().norm().item(), n
    for n, p in r1.global_model.named_parameters():
        assert torch.equal(p.detach(), gsnap[n]), n
        assert p.grad is None

    # a head state dict saved by the module round-trips through load_state_dict(strict=False)
    path = tmp_path / "best_head.pth"
    torch.save({k: v for k, v in r1.state_dict().items() if not k.startswith("global_model.")}, path)
    from graphcast_lite_amd.roi_residual import ROIResidualModel

    lats, lons = _regular(32, 64)
    r3 = ROIResidualModel(r1.global_model, (20.0, 60.0, 30.0, 100.0), lats, lons, torch.device(DEV), hidden_dim=32,
                          processor_steps=2, roi_k=8)
    res = r3.load_state_dict(torch.load(path, map_location=DEV, weights_only=True), strict=False)
    assert not res.unexpected_keys and all(k.startswith("global_model.") for k in res.missing_keys)
    Xd2 = Xd * 1.01
    assert torch.equal(r3(Xd2), r1(Xd2))
