"""The small dataset directories behind `tests/golden/runner_vectors.npz`: the generator writes them for the reference's
loaders, the tests write the same files from the fixture's inputs for the product's.

Legacy tensors: N_train 6, N_test 5, LON 6, LAT 4, 3 stored steps (2 used), 5 features (3 used), 2 target steps (1 used),
as 4-D [N, LON, LAT, steps*F] or 5-D [N, LON, LAT, steps, F] files.  Chunked: a regular (T 14, 5 x 3, 4 channels) and a
flat (T 12, 7 nodes, 3 channels) fp16 series, obs 2, one target step, 3 features."""
import json
import os
import types

import numpy as np
import torch

NAME = "runner_case"
# (flattened, num_latitudes, num_longitudes, num_features, obs_window, pred_window): the grid is deliberately not the
# files' 6 x 4, so that the override from the file is exercised
TABLE_ROW = (True, 32, 64, 5, 3, 2)
N_TRAIN, N_TEST, LON, LAT, OBS, F, PRED = 6, 5, 6, 4, 3, 5, 2
OBS_USED, F_USED, PRED_USED = 2, 3, 1
CH_OBS, CH_PRED, CH_FEAT = 2, 1, 3


def data_config(flattened=True):
    return types.SimpleNamespace(dataset_name=NAME, num_features_used=F_USED, obs_window_used=OBS_USED,
                                 pred_window_used=PRED_USED, want_feats_flattened=flattened)


def make_inputs(seed=7):
    rng = np.random.default_rng(seed)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    z = dict(leg_X_train=f32(N_TRAIN, LON, LAT, OBS * F), leg_y_train=f32(N_TRAIN, LON, LAT, PRED * F),
             leg_X_test=f32(N_TEST, LON, LAT, OBS * F), leg_y_test=f32(N_TEST, LON, LAT, PRED * F),
             leg_lon=np.linspace(80.0, 100.0, LON), leg_lat=np.linspace(50.0, 62.0, LAT),
             reg_series=(3.0 * rng.standard_normal((14, 5, 3, 4)) + 1.0).astype(np.float16),
             reg_mean=f32(4), reg_std=(0.5 + rng.random(4)).astype(np.float32),
             reg_lon=np.linspace(0.0, 288.0, 5), reg_lat=np.linspace(-60.0, 60.0, 3),
             flat_series=(2.0 * rng.standard_normal((12, 7, 3))).astype(np.float16),
             flat_mean=f32(3), flat_std=(0.5 + rng.random(3)).astype(np.float32),
             flat_lon=(360.0 * rng.random(7)), flat_lat=(180.0 * rng.random(7) - 90.0),
             flat_is_regional=np.array([0, 1, 1, 0, 0, 1, 0], dtype=bool))
    return z


def write_legacy(path, z, five_d=False, coords=False):
    """X_train.pt .. y_test.pt (and coords.npz) as the reference's loader reads them."""
    os.makedirs(path, exist_ok=True)
    for split in ("train", "test"):
        X, y = torch.tensor(z[f"leg_X_{split}"]), torch.tensor(z[f"leg_y_{split}"])
        if five_d:
            X, y = X.view(-1, LON, LAT, OBS, F), y.view(-1, LON, LAT, PRED, F)
        torch.save(X, os.path.join(path, f"X_{split}.pt"))
        torch.save(y, os.path.join(path, f"y_{split}.pt"))
    if coords:
        np.savez(os.path.join(path, "coords.npz"), longitude=z["leg_lon"], latitude=z["leg_lat"])
    return path


def write_chunked(path, z, flat=False):
    """data.npy (raw fp16) + dataset_info.json + scalers.npz + coords.npz + variables.json."""
    os.makedirs(path, exist_ok=True)
    k = "flat" if flat else "reg"
    series = z[f"{k}_series"]
    series.tofile(os.path.join(path, "data.npy"))
    if flat:
        info = dict(flat=True, n_time=int(series.shape[0]), n_nodes=int(series.shape[1]), n_feat=int(series.shape[2]))
        np.savez(os.path.join(path, "coords.npz"), longitude=z["flat_lon"], latitude=z["flat_lat"],
                 is_regional=z["flat_is_regional"])
    else:
        info = dict(n_time=int(series.shape[0]), n_lon=int(series.shape[1]), n_lat=int(series.shape[2]),
                    n_feat=int(series.shape[3]))
        np.savez(os.path.join(path, "coords.npz"), longitude=z["reg_lon"], latitude=z["reg_lat"])
    with open(os.path.join(path, "dataset_info.json"), "w") as fh:
        json.dump(info, fh)
    np.savez(os.path.join(path, "scalers.npz"), mean=z[f"{k}_mean"], std=z[f"{k}_std"])
    with open(os.path.join(path, "variables.json"), "w") as fh:
        json.dump([f"v{i}" for i in range(series.shape[-1])], fh)
    return path
