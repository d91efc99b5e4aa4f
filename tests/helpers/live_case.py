"""The inputs of tests/golden/make_live_golden.py, restated for test_live, test_live_kernels and test_live_forecast:
source axes, seeded fields, nodes, scalers, statics and the tiny dataset directories."""
import json
import os
from datetime import datetime, timedelta, timezone
from pathlib import Path

import numpy as np

from conftest import GOLDEN

VAR_ORDER = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm",
             "t@850", "u@850", "v@850", "z@850", "q@850", "t@500", "u@500", "v@500", "z@500", "q@500",
             "sst", "cape"]
ABSENT = ("tp", "q@850", "q@500")
SURFACE_B = ("tcwv",)
CAPPED = ("sp",)
UNSUPPORTED = ("sst", "cape")
STATIC = ("z_surf", "lsm")
OBS = 2
T0 = datetime(2024, 2, 28, 18, tzinfo=timezone.utc)
SUMMARY_SEED = 90453


def golden():
    return dict(np.load(os.path.join(GOLDEN, "live_vectors.npz")))


def axes(kind):
    if kind == "a":
        return np.linspace(90.0, -90.0, 13), -180.0 + 15.0 * np.arange(24)
    if kind == "b":
        return np.linspace(-90.0, 90.0, 19), 10.0 * np.arange(36)
    return np.linspace(75.0, -75.0, 11), 20.0 * np.arange(18) - 100.0


def kind_of(name):
    return "b" if name in SURFACE_B else "c" if name in CAPPED else "a"


def field_values(name, cycle, var_order=VAR_ORDER):
    lats, lons = axes(kind_of(name))
    rng = np.random.default_rng(1000 * cycle + var_order.index(name))
    x = rng.standard_normal((lats.size, lons.size))
    if name in ("msl", "sp"):
        x = 100000.0 + 1500.0 * x
    elif name.startswith("t"):
        x = 270.0 + 12.0 * x
    elif name.startswith("z"):
        x = 30000.0 + 800.0 * x
    elif name.startswith("q"):
        x = 1e-3 * np.abs(x)
    else:
        x = 7.0 * x
    return x.astype(np.float32)


def nodes():
    rng = np.random.default_rng(42)
    lat = np.degrees(np.arcsin(rng.uniform(-1, 1, 690)))
    lon = rng.uniform(0, 360, 690)
    lat = np.concatenate([lat, [90.0, -90.0, 10.0, 20.0, 30.0, -40.0, 80.0, -85.0, 75.0, -75.0]])
    lon = np.concatenate([lon, [123.0, 321.0, 0.0, 359.99, 360.0 - 1e-4, -77.5, 200.0, 15.0, 240.0, 250.0]])
    return lat.astype(np.float32), lon.astype(np.float32)


def scalers():
    rng = np.random.default_rng(5)
    mean = rng.normal(0, 50, len(VAR_ORDER) + 2).astype(np.float32)
    std = rng.uniform(0.5, 40, len(VAR_ORDER) + 2).astype(np.float32)
    return mean, std


def statics(G):
    rng = np.random.default_rng(6)
    return {"z_surf": (500.0 * np.abs(rng.standard_normal(G))).astype(np.float32),
            "lsm": (rng.random(G) < 0.3).astype(np.float32)}


def summary_case(G, C):
    rng = np.random.default_rng(SUMMARY_SEED)
    pred = rng.standard_normal((G, 4, C))
    pred[..., 0] = 263.0 + 9.0 * pred[..., 0]
    pred[..., 1:3] *= 5.0
    pred[..., 3] = 1012.0 + 11.0 * pred[..., 3]
    lat = rng.uniform(54.0, 58.0, G).astype(np.float32)
    lon = rng.uniform(90.0, 96.0, G).astype(np.float32)
    return pred.astype(np.float32), lat, lon


def cycle_times():
    return [T0 + timedelta(hours=6 * k) for k in range(OBS)]


def analysis(cycle, var_order=VAR_ORDER, absent=ABSENT):
    """The AnalysisFields of a cycle: every supported, non-static name that the payload holds."""
    return {n: (field_values(n, cycle, var_order), *axes(kind_of(n))) for n in var_order
            if n not in absent and n not in STATIC and n not in UNSUPPORTED}


def tiny_dataset(folder: Path, flat: bool):
    rng = np.random.default_rng(11 + flat)
    names = ["t2m", "z_surf", "msl", "lsm", "10u"]
    folder.mkdir(parents=True)
    shape = (3, 12, 5) if flat else (3, 4, 3, 5)
    (rng.standard_normal(shape) * 100).astype(np.float16).tofile(folder / "data.npy")
    info = {"n_time": 3, "n_feat": 5, "variables": names}
    info.update({"flat": True, "n_nodes": 12} if flat else {"n_lon": 4, "n_lat": 3})
    (folder / "dataset_info.json").write_text(json.dumps(info))
    (folder / "variables.json").write_text(json.dumps(names))
    coords = {"latitude": rng.uniform(-90, 90, 12), "longitude": rng.uniform(0, 360, 12)}
    if flat:
        coords["is_regional"] = rng.random(12) < 0.5
        np.savez(folder / "scalers.npz", x_mean=rng.normal(size=5), x_scale=rng.uniform(1, 2, 5),
                 y_mean=rng.normal(size=5), y_scale=rng.uniform(1, 2, 5))
    else:
        np.savez(folder / "scalers.npz", mean=rng.normal(size=5), std=rng.uniform(1, 2, 5))
    np.savez(folder / "coords.npz", **coords)


def apply_tables(values, pos, w):
    """A point table applied as the kernel applies it, in numpy float64: the four products added in table order onto
    0.0, then float32."""
    flat = np.asarray(values, dtype=np.float32).reshape(-1)
    acc = np.zeros(pos.shape[0])
    for k in range(4):
        acc = acc + flat[pos[:, k]] * w[:, k]
    return acc.astype(np.float32)
