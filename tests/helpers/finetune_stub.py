"""The stub model the reference's `train()` (src/train.py:311-524) was driven with when
`tests/golden/finetune_vectors.npz` was generated (tests/golden/make_finetune_golden.py): `.obs_window`, an
`encoder`, a `processor` (what `freeze_processor_epochs` freezes and `finetune_processor_lr_factor` slows down) and a
`decoder`, declared in that order so that torch's group order (processor last) differs from the module order."""
import types

import numpy as np
import torch

N_LAT, N_LON, OBS, C, HIDDEN = 4, 6, 2, 3, 8
G = N_LAT * N_LON
PRED = 2          # targets per sample (pred window)
N_TRAIN, N_VAL, BATCH = 6, 2, 2


class FinetuneStub(torch.nn.Module):
    def __init__(self, seed=5):
        super().__init__()
        self.obs_window = OBS
        g = torch.Generator().manual_seed(seed)
        self.encoder = torch.nn.Linear(OBS * C, HIDDEN)
        self.processor = torch.nn.Linear(HIDDEN, HIDDEN)
        self.decoder = torch.nn.Linear(HIDDEN, C)
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(0.4 * torch.randn(p.shape, generator=g))

    def forward(self, X, attention_threshold=0.0, **kw):
        h = torch.tanh(self.encoder(X))
        h = h + torch.tanh(self.processor(h))
        return 0.5 * torch.tanh(self.decoder(h))


def data(seed=17):
    """(train, val) lists of (X [B, G, OBS*C], y [B, G, PRED*C]) batches."""
    g = torch.Generator().manual_seed(seed)

    def split(n):
        X = torch.randn(n, G, OBS * C, generator=g)
        y = X[..., (OBS - 1) * C:].repeat(1, 1, PRED) + 0.3 * torch.randn(n, G, PRED * C, generator=g)
        return [(X[i:i + BATCH], y[i:i + BATCH]) for i in range(0, n, BATCH)]

    return split(N_TRAIN), split(N_VAL)


def metadata():
    """What the reference's train() reads from `dataset_metadata`: a regular grid and an ROI mask."""
    roi = np.zeros(G, dtype=np.float32)
    roi[: 2 * G // 3] = 1.0
    return types.SimpleNamespace(num_latitudes=N_LAT, num_longitudes=N_LON, flat_grid=False, is_regional=roi)


def config(**over):
    """The reference config fields train() and the optimiser of src/main.py:190-211 read."""
    cfg = dict(use_latitude_weighting=True, max_ar_steps=2, static_channels=[], forcing_channels=[2],
               boundary_mask_width=0, roi_only_loss=True, use_residual=True, early_stopping_delta=0.0,
               early_stopping_patience=10, freeze_processor_epochs=2, finetune_processor_lr_factor=0.1,
               learning_rate=1e-2, data=types.SimpleNamespace(num_features_used=C))
    cfg.update(over)
    return types.SimpleNamespace(**cfg)


# the fixture's runs: (config overrides, epochs, epochs of the first part before a resume or None)
RUNS = {
    "a": (dict(), 5, None),
    "b": (dict(early_stopping_delta=0.02, early_stopping_patience=1), 6, None),
    "c": (dict(), 5, 3),
}
