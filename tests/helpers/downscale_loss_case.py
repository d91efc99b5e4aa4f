"""The cases of the downscaler's objective shared by tests/golden/make_downscale_loss_golden.py (which runs the
reference on them) and the tests: shapes, weights, the seeded inputs and the error measure."""
import hashlib
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "downscale_loss_vectors.npz")

SEED = 1234
SHAPES = [            # (B, C, H, W)
    (3, 2, 2, 2),     # the smallest legal shape
    (2, 5, 7, 9),     # the regional grid of downscale_case.py, both sizes odd
    (1, 3, 8, 6),     # both sizes even, with a Nyquist column
    (1, 4, 33, 70),   # more than one wave per row, several tiles, a partial last tile
    (1, 2, 5, 256),   # the size limits
    (1, 2, 256, 3),
]
WEIGHTS = [(0.0, 0.0), (0.1, 0.0), (0.0, 0.05), (0.1, 0.05)]  # (spectral, gradient)
MASKED_CHANNEL = 1
MIN_GAP, MIN_P = 1e-4, 5e-3   # the conditioning every case must have (asserted by the generator, never a tolerance)
TERMS = ("mse", "spec", "grad")

# the metrics case: three batches of unequal size
METRICS_SEED = 4321
METRICS_BATCHES = (4, 4, 1)
METRICS_C, METRICS_OBS, METRICS_NS, METRICS_H, METRICS_W = 5, 2, 2, 7, 9

# the training case on the archives of downscale_case.py
TRAIN_OBS, TRAIN_BATCH, TRAIN_LR, TRAIN_EPOCHS = 2, 3, 1e-2, 2
TRAIN_SW, TRAIN_GW, TRAIN_RESIDUAL = 0.1, 0.05, True


def inputs(shape):
    """(out, Y, x_last) float64 standard normals of a shape: a generator seeded SEED per shape gives out, then Y; x_last
    is a draw of its own from a generator seeded SEED + 1.  (As the third draw of the first generator x_last leaves
    shape (2, 5, 7, 9) with residual a bin whose | |P| - |T| | is 9.6e-6, below the conditioning every case must
    have; with this draw the smallest gap is 1.15e-4 and the smallest |P| 6.1e-3.)"""
    g = torch.Generator().manual_seed(SEED)
    out, Y = (torch.randn(*shape, generator=g, dtype=torch.float64) for _ in range(2))
    return out, Y, torch.randn(*shape, generator=torch.Generator().manual_seed(SEED + 1), dtype=torch.float64)


def digest(tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.numpy()).tobytes())
    return h.hexdigest()


def mask_for(C: int, masked: bool, dtype=torch.float64):
    if not masked:
        return None
    m = torch.ones(C, dtype=dtype)
    m[MASKED_CHANNEL] = 0.0
    return m


def metrics_inputs():
    """[(X, Y, out)] float32 of the metrics case: X [B, obs * C + Ns, H, W], Y and out [B, C, H, W]."""
    g = torch.Generator().manual_seed(METRICS_SEED)
    cx = METRICS_OBS * METRICS_C + METRICS_NS
    res = []
    for B in METRICS_BATCHES:
        X = torch.randn(B, cx, METRICS_H, METRICS_W, generator=g)
        Y = torch.randn(B, METRICS_C, METRICS_H, METRICS_W, generator=g)
        out = 0.5 * torch.randn(B, METRICS_C, METRICS_H, METRICS_W, generator=g)
        res.append((X, Y, out))
    return res


def E(x, x64) -> float:
    """max |x - x64| / max |x64|."""
    x, x64 = np.asarray(x, dtype=np.float64), np.asarray(x64, dtype=np.float64)
    return float(np.max(np.abs(x - x64)) / np.max(np.abs(x64)))


def case_key(si: int, residual: bool, masked: bool) -> str:
    return f"s{si}_r{int(residual)}_m{int(masked)}"


def golden():
    return np.load(GOLDEN)
