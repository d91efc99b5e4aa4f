"""The dataset-building case shared by tests/golden/make_dataset_golden.py (which runs the reference on it) and the
tests: seeded raw fields in physical units, the block sums fed to welford_update, and numpy restatements of what the
reference computes from them (the tests compare the HIP path with the recorded reference; the restatements are checked
against the same record without a GPU)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "dataset_vectors.npz")

VAR_ORDER = ["t2m", "10u", "10v", "msl", "tp", "sp", "tcwv", "z_surf", "lsm",
             "t@850", "u@850", "v@850", "z@850", "q@850", "t@500", "u@500", "v@500", "z@500", "q@500"]
SCALE = {"msl": 0.01, "sp": 0.01, "z_surf": 1 / 9.80665, "z@850": 1 / 9.80665, "z@500": 1 / 9.80665}
STATIC = ("z_surf", "lsm")
PLEV = {"temperature": "t", "u_component_of_wind": "u", "v_component_of_wind": "v", "geopotential": "z",
        "specific_humidity": "q"}
LEVELS = (850, 500)
OVERFLOWED = ("msl", "sp", "z_surf")  # raw values beyond 65504: inf in fp16 unless scaled first
N_LON, N_LAT, T, CHUNK = 7, 5, 23, 9  # 35 points; blocks of 9, 9 and 5 steps
TIME_START, TIME_END = "2011-12-29", "2012-01-03"  # 23 six-hourly steps across a year boundary
RESUME_FROM = 9
CONST_VARS, CONST_T, CONST_CHUNK = ["t2m", "lsm"], 5, 2  # the second build: lsm is 1.0 everywhere (std at the floor)
LON = np.linspace(80.0, 81.5, N_LON)
LAT = np.linspace(50.0, 51.0, N_LAT)


def raw_field(name, n_time=T):
    """Seeded float32 field of a variable in the source's units: [n_time, lon, lat], or [lon, lat] for a static one.
    Every channel has std >= 0.01 |mean| after scaling, so the cancellation in sumsq / n - mean^2 loses at most four of
    float64's sixteen digits and cannot move a float32 result by half an ulp."""
    rng = np.random.default_rng(7000 + VAR_ORDER.index(name))
    shape = (N_LON, N_LAT) if name in STATIC else (n_time, N_LON, N_LAT)
    x = rng.standard_normal(shape)
    if name in ("msl", "sp"):
        x = 100000.0 + 1500.0 * x
    elif name == "z_surf":
        x = 70000.0 + 6000.0 * np.abs(x)
    elif name == "lsm":
        x = (x > 0.3).astype(np.float64)
    elif name.startswith("z@"):
        x = (13500.0 if name.endswith("850") else 54000.0) + 800.0 * x
    elif name.startswith("t"):
        x = (2e-3 * np.abs(x)) if name == "tp" else (20.0 + 9.0 * np.abs(x)) if name == "tcwv" else 270.0 + 12.0 * x
    elif name.startswith("q"):
        x = 1e-4 * np.abs(x)  # reaches into the fp16 subnormals
    else:
        x = 7.0 * x
    return x.astype(np.float32)


def const_field(name):
    if name == "lsm":
        return np.ones((N_LON, N_LAT), dtype=np.float32)
    return raw_field(name, CONST_T)


def welford_blocks(C=5):
    """[(block_sum, block_sumsq, block_n)] of four unequal blocks; channel 0 is constant (its block variance rounds to
    either side of zero), channel 1 has a large mean."""
    rng = np.random.default_rng(99)
    out = []
    for n in (35, 3150, 1, 4096 * 17):
        x = rng.standard_normal((n, C)) * np.array([0.0, 1.0, 3.0, 1e-3, 50.0]) + np.array([0.1, 1e4, -2.0, 0.0, 7.0])
        out.append((x.sum(axis=0), (x * x).sum(axis=0), n))
    return out


def golden():
    return np.load(GOLDEN)


def block_sums(arr):
    """What the reference takes from a float32 block: (sum, sum of the float32 squares), both float64."""
    return arr.sum(dtype=np.float64), (arr * arr).sum(dtype=np.float64)


def welford_step(mean, m2, n, bs, bq, bn):
    bm = bs / bn
    bv = np.maximum(bq / bn - bm ** 2, 0.0)
    d = bm - mean
    nn = n + bn
    return mean + d * (bn / nn), m2 + (bv * bn + (d ** 2) * n * bn / nn), nn


def restate_build(fields, names, chunk, scale=SCALE, start=0, data=None):
    """(data fp16 [T, lon, lat, C], mean f32, std f32, n) of a build from {name: raw field}; with `start` > 0 the
    statistics of the rows before it come from `data` (the fp16 already written), as a resumed build takes them."""
    n_time = max(f.shape[0] for f in fields.values() if f.ndim == 3)
    C = len(names)
    out = np.zeros((n_time, N_LON, N_LAT, C), dtype=np.float16) if data is None else data.copy()
    mean, m2, n = np.zeros(C), np.zeros(C), 0
    for a in range(0, start, chunk):
        b = min(a + chunk, start)
        s, q = np.zeros(C), np.zeros(C)
        for j in range(C):
            s[j], q[j] = block_sums(np.nan_to_num(out[a:b, :, :, j].astype(np.float32), nan=0.0))
        mean, m2, n = welford_step(mean, m2, n, s, q, (b - a) * N_LON * N_LAT)
    for a in range(start, n_time, chunk):
        b = min(a + chunk, n_time)
        s, q = np.zeros(C), np.zeros(C)
        for j, name in enumerate(names):
            f = fields[name]
            arr = np.array(np.broadcast_to(f, (n_time, N_LON, N_LAT))[a:b] if f.ndim == 2 else f[a:b])
            if name in scale:
                arr = arr * np.float32(scale[name])
            out[a:b, :, :, j] = arr.astype(np.float16)
            s[j], q[j] = block_sums(arr)
        mean, m2, n = welford_step(mean, m2, n, s, q, (b - a) * N_LON * N_LAT)
    std = np.maximum(np.sqrt(m2 / max(n, 1)), 1e-6)
    return out, mean.astype(np.float32), std.astype(np.float32), n


def restate_widened_scalers(data):
    """Mean and population std per channel of an fp16 array [..., C] in float64, then float32 and the 1e-8 rule: the
    formula of the reference's add_time_features, which evaluates it in float32."""
    flat = data.reshape(-1, data.shape[-1]).astype(np.float64)
    mean, std = flat.mean(axis=0).astype(np.float32), flat.std(axis=0).astype(np.float32)
    std[std < 1e-8] = 1.0
    return mean, std


def build_info(names, n_time, size_gb):
    return {"time_start": TIME_START, "time_end": TIME_END, "n_time": n_time, "n_lon": N_LON, "n_lat": N_LAT,
            "n_feat": len(names), "variables": list(names), "dtype": "float16", "file": "data.npy", "size_gb": size_gb}


def build_info_text(names, n_time):
    """dataset_info.json as a build leaves it (the reference's keys and order)."""
    return json.dumps(build_info(names, n_time, round(n_time * N_LON * N_LAT * len(names) * 2 / 1024 ** 3, 1)), indent=2)


def ulp32(x):
    """Spacing of float32 at |x| (float64 array)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)
