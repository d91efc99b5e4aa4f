"""The stub global model of the regional-training fixture (tests/golden/regional_train_vectors.npz): what
`DualMeshModel` reads from its global model, with the prediction, the grid latents and the processed mesh latents FIXED
LINEAR MAPS of the input window, so that an autoregressive rollout feeds back through them.  Plain torch, any device;
the maps come from a seed, so the generator (CPU, around the reference's model) and the tests (GPU, around the HIP
model) build the same one.  Test scaffolding of this repository."""
import torch
import torch.nn as nn


class LinearStubGlobal(nn.Module):
    def __init__(self, C: int, obs: int, D: int, mesh_lat, mesh_lon, seed: int = 77):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        F, M = C * obs, len(mesh_lat)
        self.num_features, self.obs_window = C, obs
        self.register_buffer("Wp", 0.3 * torch.randn(F, C, generator=g))
        self.register_buffer("Wl", 0.3 * torch.randn(F, D, generator=g))
        self.register_buffer("Wm", 0.3 * torch.randn(F, D, generator=g))
        self.register_buffer("mesh0", torch.randn(M, D, generator=g))
        self._mesh_nodes_lat, self._mesh_nodes_lon, self._num_mesh_nodes = mesh_lat, mesh_lon, M
        self.dummy = nn.Parameter(torch.zeros(1))  # a global parameter, frozen by the regional models
        # what the reference's ROIResidualModel reads besides (it encodes the window itself, src/roi_residual.py:155-160)
        self.encoding_graph, self._num_grid_nodes = None, None
        outer = self

        class _Enc:
            output_dim = D

            def forward(self, X, edge_index=None):
                return X @ outer.Wl

        self.encoder = _Enc()

    def _preprocess_input(self, grid_node_features):
        return grid_node_features

    def forward_with_latents(self, X, attention_threshold=0.0, **kw):
        X3 = X if X.dim() == 3 else X.unsqueeze(0)
        pred, lat = X3 @ self.Wp, X3 @ self.Wl
        mesh = self.mesh0.unsqueeze(0) + (X3.mean(dim=1) @ self.Wm).unsqueeze(1)
        if X3.shape[0] == 1:  # the reference's models take one sample and 2-D outputs
            return pred[0], lat[0], mesh[0]
        return pred, lat, mesh

    def forward(self, X, attention_threshold=0.0, **kw):
        return self.forward_with_latents(X, attention_threshold, **kw)[0]
