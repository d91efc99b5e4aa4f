"""Generate the dual-mesh regional model fixtures by RUNNING the reference's own `src/dual_mesh.py`.

Run from the repo root, only where `/root/reference` exists (never on the GPU box):

    python tests/golden/make_dual_mesh_golden.py

The absent third-party modules get `make_golden.py`'s placeholders (imported from there, not copied).  The PyG pieces on
this path are then called for real, so they are supplied by plain torch instead of the placeholders:
  * `torch_geometric.utils.scatter(reduce="mean" | "sum")` (the InteractionNet step, src/models.py:220-221; the
    regional encoder mean, the cross-message mean, the IDW normalisation and the decoder sum of src/dual_mesh.py): a
    torch index-add sum, divided by max(count, 1) for "mean";
  * `torch_geometric.nn.LayerNorm` (`norm_reg` and the InteractionNet step): `F.layer_norm` in node mode and
    `(x - mean) / (std_biased + eps)` over all elements in graph mode, then the affine map.
The fixtures therefore pin the reference's graph builders, module structure, weight layout, arithmetic and gradients
with these two stand-ins, not PyG itself.

Outputs (data only - arrays, no reference source text):
  tests/golden/dual_mesh_graph_vectors.npz  create_regional_mesh, build_cross_edges and build_regional_grid_mesh_edges
                                            (src/dual_mesh.py:43-297) for a 5° box, level 7, buffer 1°, plus the
                                            model's dec_idw_weights
  tests/golden/dual_mesh_model_vectors.npz  DualMeshModel (src/dual_mesh.py:479-805) driven by a stub global model
                                            (fixed prediction, grid latents and processed mesh latents): regional
                                            weights, inputs, forward / forward_cached outputs, precompute_global
                                            shapes, and the autograd gradients of the regional parameters for the ROI
                                            loss of the reference's driver, in float32 and float64
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
from make_roi_golden import _LayerNorm  # noqa: E402  (the PyG LayerNorm stand-in)

REF = make_golden.REF
ROI = (50.0, 55.0, 83.0, 88.0)
LEVEL, BUFFER = 7, 1.0


def _scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    """Stand-in for `torch_geometric.utils.scatter(..., reduce="sum" | "mean")` on rows (dim 0)."""
    assert dim == 0 and reduce in ("sum", "mean")
    out = torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype).index_add_(0, index, src)
    if reduce == "sum":
        return out
    cnt = torch.zeros(dim_size, dtype=src.dtype).index_add_(0, index, torch.ones(index.numel(), dtype=src.dtype))
    return out / cnt.clamp(min=1).view((-1,) + (1,) * (src.dim() - 1))


def _grid():
    """A flat 0.5° patch around the box (the grid of the fixtures)."""
    lats = np.arange(45.0, 60.01, 0.5)
    lons = np.arange(78.0, 93.01, 0.5)
    lon_g, lat_g = np.meshgrid(lons, lats)
    return lat_g.reshape(-1).astype(np.float32), lon_g.reshape(-1).astype(np.float32)


def _global_mesh():
    """Vertices of a level-4 icosahedral mesh as lat/lon (the 'global mesh' of the fixtures), via the reference."""
    from src.mesh.create_mesh import get_hierarchy_of_triangular_meshes_for_sphere
    from src.utils import get_mesh_lat_long

    m = get_hierarchy_of_triangular_meshes_for_sphere(splits=4)[-1]
    la, lo = get_mesh_lat_long(m)
    return np.asarray(la, np.float32), np.asarray(lo, np.float32)


class StubGlobal(torch.nn.Module):
    """What DualMeshModel reads from its global model: `num_features`, `obs_window`, `encoder.output_dim`, the global
    mesh coordinates, and `forward_with_latents` (-> fixed prediction [G, C], grid latents [G, D], processed mesh
    latents [M, D]).  Test scaffolding of THIS repo, not reference code."""

    def __init__(self, pred, lat, mesh, obs, mlat, mlon):
        super().__init__()
        self.num_features, self.obs_window = pred.shape[1], obs
        self.register_buffer("pred", pred)
        self.register_buffer("lat", lat)
        self.register_buffer("mesh", mesh)
        self._mesh_nodes_lat, self._mesh_nodes_lon, self._num_mesh_nodes = mlat, mlon, len(mlat)
        self.encoder = type("Enc", (), {"output_dim": lat.shape[1]})()

    def forward_with_latents(self, X, attention_threshold=0.0, **kw):
        return self.pred.clone(), self.lat.clone(), self.mesh.clone()


def _graph_vectors(dm, glats, glons):
    lats, lons = _grid()
    mesh, rla, rlo = dm.create_regional_mesh(ROI, level=LEVEL, buffer_deg=BUFFER)
    cei, cef = dm.build_cross_edges(glats, glons, rla, rlo, k=3)
    mask, enc, dec, dist = dm.build_regional_grid_mesh_edges(lats, lons, rla, rlo, ROI)
    out = {"roi": np.asarray(ROI, np.float64), "level": np.int64(LEVEL), "buffer": np.float64(BUFFER),
           "grid_lats": lats, "grid_lons": lons, "global_lats": glats, "global_lons": glons,
           "reg_vertices": mesh.vertices, "reg_faces": mesh.faces, "reg_lats": rla, "reg_lons": rlo,
           "cross_edge_index": cei.numpy(), "cross_edge_features": cef.numpy(), "roi_mask": mask,
           "enc_edges": enc.numpy(), "dec_edges": dec.numpy(), "dec_dist": dist.numpy()}
    return out


def _model_vectors(dm, glats, glons):
    lats, lons = _grid()
    Fe, obs, D, hidden, steps, k = 5, 2, 11, 32, 2, 3
    G, M = lats.shape[0], glats.shape[0]
    g = torch.Generator().manual_seed(21)
    pred = torch.randn(G, Fe, generator=g)
    lat = torch.randn(G, D, generator=g)
    mesh = torch.randn(M, D, generator=g)
    X = torch.randn(1, G, Fe * obs, generator=g)
    y = torch.randn(1, G, Fe, generator=g)
    torch.manual_seed(9)
    m = dm.DualMeshModel(StubGlobal(pred, lat, mesh, obs, glats, glons), ROI, lats, lons, torch.device("cpu"),
                         reg_mesh_level=LEVEL, reg_mesh_buffer=BUFFER, reg_processor_steps=steps, cross_k=k,
                         hidden_dim=hidden)
    with torch.no_grad():  # off the decoder's near-zero start, so that every gradient is well conditioned
        m.reg_decoder.mlp[2].weight.normal_(0.0, 0.2, generator=g)
        m.reg_decoder.mlp[2].bias.normal_(0.0, 0.1, generator=g)
        for ln in (m.reg_processor.step.edge_norm, m.reg_processor.step.node_norm, m.cross_message.norm_reg):
            ln.weight.uniform_(0.5, 1.5, generator=g)
            ln.bias.normal_(0.0, 0.1, generator=g)
    sd = {kk: v.clone() for kk, v in m.state_dict().items() if not kk.startswith("global_model.")}
    names = [n for n, p in m.named_parameters() if not n.startswith("global_model.")]

    def run(model, dt):
        for p in model.parameters():
            p.grad = None
        out = model(X.to(dt))
        mask = model.roi_mask
        loss = ((out.unsqueeze(0)[:, mask, :] - y.to(dt)[:, mask, :]) ** 2).mean()
        loss.backward()
        gp = dict(model.named_parameters())
        return out.detach(), loss.detach(), {n: gp[n].grad.detach().clone() for n in names if gp[n].grad is not None}

    out32, loss32, g32 = run(m, torch.float32)
    with torch.no_grad():
        cache = m.precompute_global(X)
        cached = m.forward_cached(X[0][m.roi_mask], cache["global_pred_roi"], cache["roi_grid_latent"],
                                  cache["cross_sender_feat"])
    m64 = copy.deepcopy(m).double()
    m64.global_model.pred, m64.global_model.lat, m64.global_model.mesh = pred.double(), lat.double(), mesh.double()
    out64, loss64, g64 = run(m64, torch.float64)
    arrays = {"X": X.numpy(), "y": y.numpy(), "pred": pred.numpy(), "lat": lat.numpy(), "mesh": mesh.numpy(),
              "grid_lats": lats, "grid_lons": lons, "global_lats": glats, "global_lons": glons,
              "roi": np.asarray(ROI, np.float64), "dims": np.asarray([Fe, obs, D, hidden, steps, k, LEVEL], np.int64),
              "buffer": np.float64(BUFFER), "out32": out32.numpy(), "out64": out64.numpy(), "loss32": loss32.numpy(),
              "loss64": loss64.numpy(), "cached32": cached.numpy(), "sd_keys": np.asarray(sorted(sd)),
              "param_names": np.asarray(names), "cache_keys": np.asarray(sorted(cache)),
              "dec_idw_weights": m.dec_idw_weights.numpy()}
    for kk in sorted(cache):
        arrays["cache_shape:" + kk] = np.asarray(cache[kk].shape, np.int64)
    for kk, v in sd.items():
        arrays["w:" + kk] = v.numpy()
    assert sorted(g32) == sorted(g64)
    for n in g32:
        arrays["g32:" + n] = g32[n].numpy()
        arrays["g64:" + n] = g64[n].numpy()
    return arrays


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    make_golden._placeholders()
    sys.modules["torch_geometric.nn"].LayerNorm = _LayerNorm
    sys.modules["torch_geometric.utils"].scatter = _scatter
    sys.path.insert(0, REF)
    import src.dual_mesh as dm

    glats, glons = _global_mesh()
    graphs = _graph_vectors(dm, glats, glons)
    model = _model_vectors(dm, glats, glons)
    graphs["dec_idw_weights"] = model["dec_idw_weights"]
    np.savez_compressed(os.path.join(HERE, "dual_mesh_graph_vectors.npz"), **graphs)
    np.savez_compressed(os.path.join(HERE, "dual_mesh_model_vectors.npz"), **model)
    print("wrote dual_mesh_graph_vectors.npz, dual_mesh_model_vectors.npz")


if __name__ == "__main__":
    main()
