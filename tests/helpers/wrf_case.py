"""The inputs of tests/golden/make_wrf_golden.py for test_wrf_host, test_wrf_kernels and test_wrf: the ERA5-like fp16
series on a regular 25 x 17 grid, its flat twin, the scalers, the prediction bundles, the sample-offset lists and the
dataset directories.  The generator imports this module, so both sides use the same seeded arrays."""
import json
import os
from pathlib import Path

import numpy as np

from conftest import GOLDEN

VAR_NAMES = ["t2m", "10u", "10v", "msl", "sp", "tcwv", "z_surf"]
C, P, T, N_SAMPLES, OBS = len(VAR_NAMES), 4, 20, 6, 2
TIME_START = "2023-01-18"
WRF_JSON = os.path.join(GOLDEN, "wrf_case.json")
OFFSETS = {"match": [3, 5, 7, 9, 11, 13],      # the target offset 7 is sample 2
           "plus2": [1, 2, 3, 4, 9, 12],       # only target + 2 is there: sample 4
           "none": [0, 1, 2, 3, 4, 10]}        # nothing within +-2
TIME_FORMATS = ["2023-01-18T00:00:00", "2023-01-18T00:00", "2023-01-18", "2023-01-18 00:00:00", "2023-01-17T18:00",
                "18.01.2023", ""]
CENTRE = np.array([262.0, 1.5, -0.8, 1015.0, 985.0, 6.0, 310.0], dtype=np.float64)
SPREAD = np.array([9.0, 4.0, 4.0, 8.0, 7.0, 2.5, 120.0], dtype=np.float64)
FLAT_SEED = 77


def golden():
    return dict(np.load(os.path.join(GOLDEN, "wrf_vectors.npz")))


def axes():
    """(lons, lats) float64 of the regular grid: 0.25 degrees over 90-96 E, 54-58 N."""
    return 90.0 + 0.25 * np.arange(25), 54.0 + 0.25 * np.arange(17)


def series():
    """fp16 [T, 25, 17, C] in physical (dataset) units: a smooth field plus noise per variable."""
    rng = np.random.default_rng(2023)
    lons, lats = axes()
    x = rng.standard_normal((T, 25, 17, C))
    wave = np.sin(lons / 1.7)[None, :, None, None] + np.cos(lats / 1.3)[None, None, :, None]
    trend = np.linspace(-1, 1, T)[:, None, None, None]
    return (CENTRE + SPREAD * (0.6 * wave + 0.3 * trend + 0.25 * x)).astype(np.float16)


def scalers():
    """(mean, std) float32, two entries longer than the variables (the scripts slice them)."""
    rng = np.random.default_rng(8)
    mean = np.concatenate([CENTRE + rng.normal(0, 0.5, C), [3.0, 4.0]]).astype(np.float32)
    std = np.concatenate([SPREAD * rng.uniform(0.8, 1.2, C), [1.0, 2.0]]).astype(np.float32)
    return mean, std


def predictions():
    """(pred, truth) normalised float32 [N_SAMPLES, 425, P * C], regular (longitude-major) node order."""
    rng = np.random.default_rng(31)
    truth = rng.standard_normal((N_SAMPLES, 425, P * C)).astype(np.float32)
    pred = (truth + 0.15 * rng.standard_normal(truth.shape)).astype(np.float32)
    return pred, truth


def flat_order():
    """perm[k] = the regular node that flat row k holds."""
    return np.random.default_rng(FLAT_SEED).permutation(425)


def node_coords(flat: bool):
    """(latitude, longitude) as coords.npz stores them: the axes, or per node in flat row order."""
    lons, lats = axes()
    if not flat:
        return lats, lons
    perm = flat_order()
    return np.tile(lats, 25)[perm], np.repeat(lons, 17)[perm]


def bundle(flat: bool, offsets, legacy: bool = False):
    """The predictions.pt content: the dictionary of scripts/predict.py, or the bare tensor."""
    import torch

    pred, truth = predictions()
    if flat:
        pred, truth = pred[:, flat_order()], truth[:, flat_order()]
    if legacy:
        return torch.from_numpy(pred.copy())
    return {"predictions": torch.from_numpy(pred.copy()), "ground_truth": torch.from_numpy(truth.copy()),
            "n_features": C, "ar_steps": P, "obs_window": OBS, "n_lon": 25, "n_lat": 17,
            "sample_offsets": list(offsets), "data_dir": "data"}


def dataset_dir(folder, flat: bool = False, time_start=TIME_START, with_series: bool = True, identity: bool = False):
    """A dataset directory as the scripts read it.  identity: scalers (0, 1), so a forecast comes back as it is."""
    folder = Path(folder)
    folder.mkdir(parents=True, exist_ok=True)
    mean, std = scalers()
    if identity:
        mean, std = np.zeros_like(mean), np.ones_like(std)
    np.savez(folder / "scalers.npz", mean=mean, std=std)
    (folder / "variables.json").write_text(json.dumps(VAR_NAMES))
    lat, lon = node_coords(flat)
    np.savez(folder / "coords.npz", latitude=lat, longitude=lon)
    info = {"n_time": T, "n_lon": 25, "n_lat": 17, "n_feat": C, "time_end": "2023-01-22"}
    if time_start is not None:
        info["time_start"] = time_start
    if flat:
        info["flat_grid"] = True
    (folder / "dataset_info.json").write_text(json.dumps(info))
    if with_series and not flat:
        series().tofile(folder / "data.npy")
    return folder


def shortened_wrf(path, n_steps: int):
    """The WRF JSON with only its first n_steps hourly values (the 7-step and 3-step rules of load_wrf)."""
    d = json.loads(Path(WRF_JSON).read_text())
    d["times"] = d["times"][:n_steps]
    d["domain_mean"] = {k: v[:n_steps] for k, v in d["domain_mean"].items()}
    d["domain_fields"] = {k: v[:n_steps] for k, v in d["domain_fields"].items()}
    Path(path).write_text(json.dumps(d))
    return path


def sum_bound(P_points: int, abs_sum):
    """4 * P * 2^-53 * sum|x|: the bound on two differently ordered float64 sums of P terms."""
    return 4.0 * P_points * 2.0 ** -53 * abs_sum


def apply_tables(values, pos, w, node_stride: int = 1, offset: int = 0) -> np.ndarray:
    """A point table applied as the kernels apply it, in numpy float64: the four products added in table order onto
    0.0, NaN where the table says outside."""
    flat = np.asarray(values).reshape(-1)
    safe = np.where(pos < 0, 0, pos).astype(np.int64)
    acc = np.zeros(pos.shape[0])
    for k in range(4):
        acc = acc + flat[offset + safe[:, k] * node_stride].astype(np.float32) * w[:, k]
    acc[pos[:, 0] < 0] = np.nan
    return acc
