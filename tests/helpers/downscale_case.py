"""The downscaler case shared by tests/golden/make_downscale_golden.py (which runs the reference on it) and the tests:
the axes and the box of tests/helpers/multires_case.py (global 24 x 12, regional 9 x 7 reaching past the box
(15, 46, 60, 120)), 5 variables, 12 frames, scalers with `n`, and float64 restatements of what the reference computes."""
import json
import os

import numpy as np

import multires_case as MC

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "downscale_vectors.npz")

ROI, VARS, T = MC.ROI, MC.VARS, MC.T
C = len(VARS)
OBS = 2
STATIC = [3, 4]                                 # z_surf and tp stand in for the reference's z_surf / lsm (7, 8)
MAGS = np.array([280.0, 3.0, 3.0, 900.0, 0.002])
U_CHANNELS = (1,)                               # "10u"
SAMPLES = [0, 4, 10]                            # items of the "all" split stored in the fixture
SPLITS = ["train", "val", "test", "all"]
GLOBAL_SOURCE, REGION_SOURCE = "datasets/global_24x12", "datasets/region_9x7"  # the *_source strings of the info


def series(seed: int, n_lon: int, n_lat: int) -> np.ndarray:
    """fp16 (T, lon, lat, C): every channel its magnitude with 10 % noise."""
    rng = np.random.default_rng(seed)
    return (MAGS * (1.0 + 0.1 * rng.standard_normal((T, n_lon, n_lat, C)))).astype(np.float16)


def scalers(n_lon: int, n_lat: int):
    return MAGS.astype(np.float32), (0.1 * MAGS).astype(np.float32), np.int64(T * n_lon * n_lat)


def gnn_scalers():
    """The GNN data set's own scalers (the archive is denormalised with these, not with the pairs')."""
    return (MAGS * 0.98).astype(np.float32), (0.12 * MAGS).astype(np.float32)


def pair(seed: int):
    """(g_data, r_data) of a seed."""
    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    return series(seed, len(g_lons), len(g_lats)), series(seed + 1000, len(r_lons), len(r_lats))


def write_pair(root: str, g_data, r_data):
    """The two dataset directories in the reference's layout, scalers.npz with `n`."""
    g_lats, g_lons = MC.global_axes()
    r_lats, r_lons = MC.regional_axes()
    dirs = []
    for name, data, lats, lons in (("global", g_data, g_lats, g_lons), ("region", r_data, r_lats, r_lons)):
        mean, std, n = scalers(len(lons), len(lats))
        d = MC.write_dataset(os.path.join(root, name), data, lats, lons, mean, std, VARS)
        np.savez(os.path.join(d, "scalers.npz"), mean=mean, std=std, n=n)
        dirs.append(d)
    return dirs


def restate_coarse(g_data, pos, w):
    """(float64 sums [T, P, C]) of the point table over the full frames: each product rounded on its own, added in
    corner order onto 0.0."""
    v = g_data.reshape(g_data.shape[0], -1, g_data.shape[-1]).astype(np.float64)[:, pos, :]
    acc = np.zeros((v.shape[0], v.shape[1], v.shape[3]))
    for m in range(4):
        acc = acc + v[:, :, m, :] * w[:, m, None]
    return acc


def golden():
    return np.load(GOLDEN)


def info_of(g):
    return json.loads(str(g["info"]))
