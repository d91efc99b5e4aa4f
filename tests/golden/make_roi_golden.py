"""Generate the ROI residual head fixtures by RUNNING the reference's own `src/roi_residual.py`.

Run from the repo root, only where `/root/reference` exists (never on the GPU box):

    python tests/golden/make_roi_golden.py

The absent third-party modules get `make_golden.py`'s placeholders (imported from there, not copied).  Two PyG pieces
on this path are then called for real, so they are supplied by plain torch instead of the placeholders:
  * `torch_geometric.utils.scatter(reduce="mean")` inside the InteractionNet step (src/models.py:220-221): a torch
    index-add sum divided by max(count, 1);
  * `torch_geometric.nn.LayerNorm` of the InteractionNet step (src/models.py:201-203): `F.layer_norm` in node mode and
    `(x - mean) / (std_biased + eps)` over all elements in graph mode, then the affine map.
The reference's `_compute_mesh_edge_features` cannot reduce an empty edge list (numpy max of an empty array), so for
the 1-point ROI the feature call is short-circuited to an empty [0, 4] tensor; mask, indices and edge_index of that
case are still the reference's own.  The head fixtures therefore pin the reference's module structure, weight
layout, arithmetic and gradients with these two stand-ins, not PyG itself.

Outputs (data only - arrays, no reference source text):
  tests/golden/roi_knn_vectors.npz   build_roi_knn_graph (src/roi_residual.py:15-59) for four cases: a box on the
                                     regular 64x32 grid, a flat per-node coordinate list, a 3-point ROI (k_eff
                                     truncates) and a 1-point ROI (no edges)
  tests/golden/roi_head_vectors.npz  ROIResidualModel (src/roi_residual.py:82-185) driven with a stub global model
                                     (fixed prediction and grid latents): head weights, inputs, output, and the
                                     autograd gradients of the head parameters for the ROI loss of the reference's
                                     driver (scripts/train_roi_residual.py:112-116), in float32 and float64
"""
import copy
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (placeholders for the absent modules)

REF = make_golden.REF


class _LayerNorm(torch.nn.Module):
    """Stand-in for `torch_geometric.nn.LayerNorm(C, mode)` (see the module docstring)."""

    def __init__(self, in_channels, eps=1e-5, affine=True, mode="graph"):
        super().__init__()
        self.mode, self.eps = mode, eps
        self.weight = torch.nn.Parameter(torch.ones(in_channels))
        self.bias = torch.nn.Parameter(torch.zeros(in_channels))

    def forward(self, x):
        if self.mode == "node":
            return F.layer_norm(x, (x.shape[-1],), self.weight, self.bias, self.eps)
        xc = x - x.mean()
        return xc / ((xc * xc).mean().sqrt() + self.eps) * self.weight + self.bias


def _scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    """Stand-in for `torch_geometric.utils.scatter(..., reduce="mean")` on rows (dim 0)."""
    assert dim == 0 and reduce == "mean"
    out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
    cnt = torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype))
    return out / cnt.clamp(min=1).unsqueeze(-1)


class StubGlobal(torch.nn.Module):
    """What ROIResidualModel reads from its global model: `num_features`, `obs_window`, `encoder.output_dim`, the
    forward (-> fixed prediction [G, C]) and `_preprocess_input` + `encoder.forward` (-> fixed grid latents in the first
    G rows).  Test scaffolding of THIS repo, not reference code."""

    def __init__(self, pred, lat, obs):
        super().__init__()
        self.num_features, self.obs_window = pred.shape[1], obs
        self._num_grid_nodes = pred.shape[0]
        self.register_buffer("pred", pred)
        self.register_buffer("lat", lat)
        self.encoding_graph = None
        outer = self

        class _Enc:
            output_dim = lat.shape[1]

            def forward(self, X, edge_index):
                return torch.cat([outer.lat, torch.zeros(3, outer.lat.shape[1], dtype=outer.lat.dtype)], dim=0)

        self.encoder = _Enc()

    def _preprocess_input(self, grid_node_features):
        return grid_node_features

    def forward(self, X, attention_threshold=0.0, **kw):
        return self.pred.clone()


def _regular(nlat, nlon):
    lats = np.linspace(-90, 90, nlat, endpoint=True)
    lons = np.linspace(0, 360, nlon, endpoint=False)
    lon_grid, lat_grid = np.meshgrid(lons, lats)  # as scripts/train_roi_residual.py builds them
    return lat_grid.flatten().astype(np.float32), lon_grid.flatten().astype(np.float32)


def _knn_vectors(build):
    rng = np.random.default_rng(7)
    flat_lats = rng.uniform(-60, 80, 600).astype(np.float32)
    flat_lons = rng.uniform(0, 360, 600).astype(np.float32)
    reg = _regular(32, 64)
    cases = {
        "box": (reg, (20.0, 60.0, 30.0, 100.0), 8),
        "flat": ((flat_lats, flat_lons), (10.0, 50.0, 40.0, 120.0), 8),
        "three": (reg, (0.0, 5.0, 0.0, 12.0), 8),
        "one": (reg, (0.0, 5.0, 0.0, 1.0), 8),
    }
    out = {}
    for name, ((la, lo), roi, k) in cases.items():
        mask, idx, ei, ef = build(la, lo, roi, k=k)
        out.update({f"{name}_lats": la, f"{name}_lons": lo, f"{name}_roi": np.asarray(roi, np.float64),
                    f"{name}_k": np.int64(k), f"{name}_mask": mask, f"{name}_indices": idx.astype(np.int64),
                    f"{name}_edge_index": ei.numpy(), f"{name}_edge_features": ef.numpy()})
    assert out["three_edge_index"].shape == (2, 6) and out["one_edge_index"].shape == (2, 0)
    np.savez_compressed(os.path.join(HERE, "roi_knn_vectors.npz"), **out)


def _head_vectors(ROIResidualModel):
    nlat, nlon, Fe, obs, D, hidden, steps, k = 12, 24, 5, 2, 11, 32, 2, 4
    lats, lons = _regular(nlat, nlon)
    G = lats.shape[0]
    roi = (-10.0, 40.0, 30.0, 120.0)
    g = torch.Generator().manual_seed(11)
    pred = torch.randn(G, Fe, generator=g)
    lat = torch.randn(G, D, generator=g)
    X = torch.randn(1, G, Fe * obs, generator=g)
    y = torch.randn(1, G, Fe, generator=g)
    torch.manual_seed(5)
    m = ROIResidualModel(StubGlobal(pred, lat, obs), roi, lats, lons, torch.device("cpu"), hidden_dim=hidden,
                         processor_steps=steps, roi_k=k)
    # move the head off its near-zero start so that every gradient is well conditioned
    with torch.no_grad():
        m.decoder.mlp[4].weight.normal_(0.0, 0.2, generator=g)
        m.decoder.mlp[4].bias.normal_(0.0, 0.1, generator=g)
        for st in m.processor.steps:
            for ln in (st.edge_norm, st.node_norm):
                ln.weight.uniform_(0.5, 1.5, generator=g)
                ln.bias.normal_(0.0, 0.1, generator=g)
    head = {kk: v.clone() for kk, v in m.state_dict().items() if not kk.startswith("global_model.")}
    names = [n for n, p in m.named_parameters() if not n.startswith("global_model.")]

    def run(model, dt):
        for p in model.parameters():
            p.grad = None
        out = model(X.to(dt))
        mask = model.roi_mask
        loss = ((out.unsqueeze(0)[:, mask, :] - y.to(dt)[:, mask, :]) ** 2).mean()
        loss.backward()
        gp = dict(model.named_parameters())
        # the last step's edge LayerNorm gets no gradient: the edge state after the last step is never read
        return out.detach(), loss.detach(), {n: gp[n].grad.detach().clone() for n in names if gp[n].grad is not None}

    out32, loss32, g32 = run(m, torch.float32)
    m64 = copy.deepcopy(m).double()
    out64, loss64, g64 = run(m64, torch.float64)
    arrays = {"X": X.numpy(), "y": y.numpy(), "pred": pred.numpy(), "lat": lat.numpy(), "grid_lats": lats,
              "grid_lons": lons, "roi": np.asarray(roi, np.float64),
              "dims": np.asarray([Fe, obs, D, hidden, steps, k], np.int64),
              "out32": out32.numpy(), "out64": out64.numpy(), "loss32": loss32.numpy(), "loss64": loss64.numpy(),
              "head_keys": np.asarray(sorted(head)), "param_names": np.asarray(names)}
    for kk, v in head.items():
        arrays["w:" + kk] = v.numpy()
    assert sorted(g32) == sorted(g64)
    for n in g32:
        arrays["g32:" + n] = g32[n].numpy()
        arrays["g64:" + n] = g64[n].numpy()
    np.savez_compressed(os.path.join(HERE, "roi_head_vectors.npz"), **arrays)


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    make_golden._placeholders()
    sys.modules["torch_geometric.nn"].LayerNorm = _LayerNorm
    sys.modules["torch_geometric.utils"].scatter = _scatter
    sys.path.insert(0, REF)
    import src.roi_residual as ref_roi
    from src.roi_residual import ROIResidualModel, build_roi_knn_graph

    feats = ref_roi._compute_mesh_edge_features
    ref_roi._compute_mesh_edge_features = lambda la, lo, ei: (
        torch.zeros(0, 4, dtype=torch.float32) if ei.shape[1] == 0 else feats(la, lo, ei))

    _knn_vectors(build_roi_knn_graph)
    _head_vectors(ROIResidualModel)
    print("wrote roi_knn_vectors.npz, roi_head_vectors.npz")


if __name__ == "__main__":
    main()
