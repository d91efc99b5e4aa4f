"""Generate the experiment-runner fixtures by RUNNING the reference's own dataset assembly on the CPU:
`load_train_and_test_datasets` (src/data/dataloader.py), `load_chunked_datasets` (src/data/dataloader_chunked.py) and
`get_dataset_metadata` (src/data/data_configs.py).

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_runner_golden.py

The inputs come from tests/helpers/runner_case.py, which also writes the directories.  The reference's dataset table has
no entry with the case's dimensions, so its lookup is pointed at `runner_case.TABLE_ROW` for the legacy loads (the
tests do the same to the product's table).  Output (data only): tests/golden/runner_vectors.npz
  leg_*, reg_*, flat_*            the inputs (runner_case.make_inputs)
  table_names, table_values       every dataset name of the reference's table and its six settings
  table_unknown                   a name of the reference's enum the table does not hold
  ref4_<X|y>_<train|val|test>     the tensors of the three datasets from the 4-D files (flattened, uniform axes)
  ref5_*                          the same from the 5-D files with coords.npz
  nf_*                            from the 4-D files with want_feats_flattened = False
  ref4_grid, ref5_grid            (num_longitudes, num_latitudes) after the override from the file
  ref4_lats, ref4_lons, ref5_*    metadata.cordinates
  chk_<reg|flat>_len              lengths of (train, val, test)
  chk_<reg|flat>_meta             (flattened, num_latitudes, num_longitudes, num_features, obs_window, pred_window,
                                  flat_grid, num_grid_nodes)
  chk_<reg|flat>_lats, _lons      metadata.cordinates; chk_flat_is_regional
  chk_<reg|flat>_<split>_X0, _Y0  item 0 of each split
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402  (where the reference checkout lives)
import runner_case as RC  # noqa: E402

sys.path.insert(0, make_golden.REF)


def main():
    from src.config import DatasetNames
    from src.data import dataloader as ref_loader
    from src.data.data_configs import DatasetMetadata, get_dataset_metadata
    from src.data.dataloader_chunked import load_chunked_datasets

    z = RC.make_inputs()
    out = dict(z)

    names, values, unknown = [], [], None
    for name in DatasetNames:
        try:
            m = get_dataset_metadata(name)
        except NotImplementedError:
            unknown = unknown or name.value
            continue
        names.append(name.value)
        values.append([int(m.flattened), m.num_latitudes, m.num_longitudes, m.num_features, m.obs_window, m.pred_window])
    out["table_names"], out["table_values"] = np.array(names), np.array(values, dtype=np.int64)
    out["table_unknown"] = np.array(unknown)

    ref_loader.get_dataset_metadata = lambda dataset_name: DatasetMetadata(*RC.TABLE_ROW)
    with tempfile.TemporaryDirectory() as tmp:
        cases = (("ref4", dict(five_d=False, coords=False), True), ("ref5", dict(five_d=True, coords=True), True),
                 ("nf", dict(five_d=False, coords=False), False))
        for tag, kw, flattened in cases:
            path = RC.write_legacy(os.path.join(tmp, tag), z, **kw)
            train, val, test, md = ref_loader.load_train_and_test_datasets(path, RC.data_config(flattened))
            for split, ds in (("train", train), ("val", val), ("test", test)):
                out[f"{tag}_X_{split}"], out[f"{tag}_y_{split}"] = ds.X.numpy().copy(), ds.y.numpy().copy()
                assert len(ds) == ds.X.shape[0]
            out[f"{tag}_grid"] = np.array([md.num_longitudes, md.num_latitudes], dtype=np.int64)
            out[f"{tag}_lats"], out[f"{tag}_lons"] = md.cordinates
        for k, flat in (("reg", False), ("flat", True)):
            path = RC.write_chunked(os.path.join(tmp, k), z, flat=flat)
            with contextlib.redirect_stdout(io.StringIO()):
                sets = load_chunked_datasets(path, obs_window=RC.CH_OBS, pred_steps=RC.CH_PRED, n_features=RC.CH_FEAT)
            md = sets[3]
            out[f"chk_{k}_len"] = np.array([len(s) for s in sets[:3]], dtype=np.int64)
            out[f"chk_{k}_meta"] = np.array([int(md.flattened), md.num_latitudes, md.num_longitudes, md.num_features,
                                             md.obs_window, md.pred_window, int(md.flat_grid), md.num_grid_nodes],
                                            dtype=np.int64)
            out[f"chk_{k}_lats"], out[f"chk_{k}_lons"] = md.cordinates
            if flat:
                out["chk_flat_is_regional"] = np.asarray(md.is_regional)
            for split, ds in zip(("train", "val", "test"), sets[:3]):
                X0, Y0 = ds[0]
                out[f"chk_{k}_{split}_X0"], out[f"chk_{k}_{split}_Y0"] = X0.numpy().copy(), Y0.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "runner_vectors.npz"), **out)
    print("wrote runner_vectors.npz:", len(out), "arrays")


if __name__ == "__main__":
    main()
