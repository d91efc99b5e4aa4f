"""Geometry and settings shared by tests/golden/make_multires_golden.py and the tests that read its fixtures."""
from datetime import datetime, timedelta, timezone

import numpy as np

ROI = (15.0, 46.0, 60.0, 120.0)
VARS = ["t2m", "10u", "10v", "z_surf", "tp"]
T, OBS, PRED, AR = 12, 2, 2, 2
WINDOW_INDICES = [0, 5, 8]  # samples of the (obs 2, pred 2, split "all") loader stored in the fixture
FRAME_TIMES = [0, 7]        # frames of build_multires_frame stored in the fixture

# four stations inside the regional grid; the first two are nearest to the same grid point (25 N, 74 E)
STATIONS = [
    {"lat": 25.3, "lon": 74.5, "elev": 287, "name": "a"},
    {"lat": 24.6, "lon": 73.2, "elev": 257, "name": "b"},
    {"lat": 36.4, "lon": 98.9, "elev": 207, "name": "c"},
    {"lat": 41.0, "lon": 105.0, "elev": 93, "name": "d"},
]
# both nearest to a node of the first latitude row with a longitude index below the number of latitudes
FIRST_ROW_STATIONS = [{"lat": 14.4, "lon": 67.0, "elev": 10, "name": "e"}, {"lat": 15.9, "lon": 89.0, "elev": 20, "name": "f"}]
# The 9 x 7 regional grid is ~600 x 800 km per cell: the radius and the correlation length are widened from the
# script's 300 km / 100 km so that IDW and OI reach beyond the station points.
IDW_POWER, IDW_RADIUS_KM = 2.0, 1500.0
OI_SIGMA_B, OI_SIGMA_O, OI_L = 1.5, 0.5, 600_000.0
LAPSE_ELEV_FLOAT = 250.0
SAMPLE_STARTS = [3, 7]
BASE_TIME = datetime(2020, 6, 1, 0, 0, 0, tzinfo=timezone.utc)
VARIANTS = ["GNN", "GNN+lapse", "GNN+MOS", "GNN+lapse+MOS", "GNN+lapse+MOS+IDW", "GNN+lapse+MOS+IDW+OI", "Persistence"]


def mean_station_elev():
    """np.float64, as the script's MEAN_STATION_ELEV."""
    return np.mean([s["elev"] for s in STATIONS])


def valid_time(step: int):
    return BASE_TIME + timedelta(hours=6 * (step + 1))


def global_axes():
    return np.linspace(-82.5, 82.5, 12), np.arange(0.0, 360.0, 15.0)


def regional_axes():
    return np.linspace(14.0, 47.0, 7), np.linspace(58.0, 122.0, 9)


def fine_axes():
    """The 41 x 61 targets over the box whose float64 interpolation pins the corner order."""
    return np.linspace(ROI[0], ROI[1], 41), np.linspace(ROI[2], ROI[3], 61)


def write_dataset(path, data, lats, lons, mean, std, variables, time_start="2020-01-01T00", time_end="2020-01-03T18"):
    """A dataset directory in the reference's layout: raw fp16 data.npy (T, lon, lat, C) + dataset_info.json +
    coords.npz + scalers.npz + variables.json."""
    import json
    import os

    os.makedirs(path, exist_ok=True)
    data = np.ascontiguousarray(data, dtype=np.float16)
    data.tofile(os.path.join(path, "data.npy"))
    Tn, n_lon, n_lat, C = data.shape
    with open(os.path.join(path, "dataset_info.json"), "w") as fh:
        json.dump({"time_start": time_start, "time_end": time_end, "n_time": Tn, "n_lon": n_lon, "n_lat": n_lat,
                   "n_feat": C, "dtype": "float16", "file": "data.npy"}, fh)
    np.savez(os.path.join(path, "coords.npz"), latitude=lats, longitude=lons)
    np.savez(os.path.join(path, "scalers.npz"), mean=mean, std=std)
    with open(os.path.join(path, "variables.json"), "w") as fh:
        json.dump(list(variables), fh)
    return str(path)


def write_flat_dataset(path, data, mean, std, info):
    """The flat dataset a builder run left behind, recreated from its data.npy bytes and dataset_info."""
    import json
    import os

    os.makedirs(path, exist_ok=True)
    np.ascontiguousarray(data, dtype=np.float16).tofile(os.path.join(path, "data.npy"))
    with open(os.path.join(path, "dataset_info.json"), "w") as fh:
        json.dump(info, fh)
    np.savez(os.path.join(path, "scalers.npz"), mean=mean, std=std)
    return str(path)
