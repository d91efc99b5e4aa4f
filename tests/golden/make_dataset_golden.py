"""Generate the dataset-building fixtures by RUNNING the reference's own `welford_update` and `download_compute_save`
(scripts/build_dataset_512x256.py) and `main` of scripts/add_time_features.py (numpy, on the CPU).

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_dataset_golden.py

`xarray`, `dask` and `gcsfs` are absent from this image and get inert placeholders in `sys.modules` (`dask.compute`
hands back the `.values` of what it is given); the reference's functions receive the stand-in `Arr` below, which offers
only `.sizes`, `.isel`, `.values` and `.level`.

Output (data only - arrays and recorded text, no reference source text): tests/golden/dataset_vectors.npz
  data, mean, std, n              the 19-channel build of tests/helpers/dataset_case.py (23 steps, 7 x 5, chunks of 9)
  resume_mean / _std / _n         the same build resumed at step 9 (statistics of rows 0-8 from the fp16 on disk)
  const_data / _mean / _std / _n  the two-channel build whose lsm is 1.0 everywhere (std at the 1e-6 floor)
  welford_mean / _m2 / _n         the state after each block of dataset_case.welford_blocks()
  tf                              the (T, 4) float32 time features add_time_features forms (heard at its np.stack)
  wide_data / _mean / _std / _n   data.npy and scalers.npz of add_time_features on the build
  wide_variables, wide_info       its variables.json and dataset_info.json text
  ref_dev_mean / _std             per channel |reference's float32 scalers - float64 restatement of the formula|
The inputs come from the seeded generators of tests/helpers/dataset_case.py, which the tests restate by calling them.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import dataset_case as DC  # noqa: E402
import make_golden  # noqa: E402  (where the reference checkout lives)

REF = make_golden.REF


class Arr:
    """What the reference touches of a DataArray: dims (time, [level,] longitude, latitude)."""

    def __init__(self, values, level=None):
        self._v, self._level = values, level
        names = ("time", "level", "longitude", "latitude") if level is not None else ("time", "longitude", "latitude")
        self.sizes = dict(zip(names, values.shape))

    def isel(self, time):
        return Arr(self._v[time], self._level)

    @property
    def values(self):
        return np.array(self._v)  # a copy: the reference scales some blocks in place

    @property
    def level(self):
        return Arr(np.asarray(self._level))


def _load(name):
    for mod in ("xarray", "dask", "gcsfs"):
        sys.modules.setdefault(mod, types.ModuleType(mod))
    sys.modules["xarray"].Dataset = sys.modules["xarray"].DataArray = object
    sys.modules["dask"].compute = lambda *xs, **kw: tuple(x.values for x in xs)
    spec = importlib.util.spec_from_file_location("_ref_" + name, os.path.join(REF, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def parts(field, names, n_time):
    """(surf_parts, plev_groups) as build_channel_parts would hand them over."""
    surf, groups = {}, []
    for name in names:
        if "@" not in name:
            f = field(name)
            surf[name] = Arr(np.broadcast_to(f, (n_time,) + f.shape) if f.ndim == 2 else f)
    for src, short in DC.PLEV.items():
        if f"{short}@850" in names:
            groups.append((src, {lev: f"{short}@{lev}" for lev in DC.LEVELS},
                           Arr(np.stack([field(f"{short}@{lev}") for lev in DC.LEVELS], axis=1), DC.LEVELS)))
    return surf, groups


def run_build(build, field, names, n_time, chunk, folder, resume_from=None):
    surf, groups = parts(field, names, n_time)
    with contextlib.redirect_stdout(io.StringIO()):
        mean, std, n, nt, nlon, nlat = build.download_compute_save(surf, groups, list(names), Path(folder),
                                                                   time_chunk=chunk, resume_from=resume_from)
    assert (nt, nlon, nlat) == (n_time, DC.N_LON, DC.N_LAT)
    data = np.array(np.memmap(os.path.join(folder, "data.npy"), dtype=np.float16, mode="r",
                              shape=(n_time, nlon, nlat, len(names))))
    return data, mean, std, n


def main():
    build, atf = _load("build_dataset_512x256"), _load("add_time_features")
    assert build.VAR_ORDER == DC.VAR_ORDER and build.SCALE_FACTORS == DC.SCALE
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, cst = Path(tmp) / "src", Path(tmp) / "dst", Path(tmp) / "const"
        src.mkdir(), cst.mkdir()
        out["data"], out["mean"], out["std"], n = run_build(build, DC.raw_field, DC.VAR_ORDER, DC.T, DC.CHUNK, src)
        out["n"] = np.int64(n)
        assert np.isfinite(out["data"]).all()
        assert (out["std"] >= 0.01 * np.abs(out["mean"])).all(), "a channel is too narrow for the 1-ulp comparison"
        data2, out["resume_mean"], out["resume_std"], n2 = run_build(build, DC.raw_field, DC.VAR_ORDER, DC.T, DC.CHUNK,
                                                                     src, resume_from=DC.RESUME_FROM)
        out["resume_n"] = np.int64(n2)
        assert data2.tobytes() == out["data"].tobytes()
        out["const_data"], out["const_mean"], out["const_std"], n3 = run_build(build, DC.const_field, DC.CONST_VARS,
                                                                               DC.CONST_T, DC.CONST_CHUNK, cst)
        out["const_n"] = np.int64(n3)
        assert out["const_std"][1] == np.float32(1e-6) and out["const_mean"][1] == 1.0

        # the metadata the reference's main() writes next to data.npy, which add_time_features reads
        (src / "dataset_info.json").write_text(DC.build_info_text(DC.VAR_ORDER, DC.T))
        (src / "variables.json").write_text(json.dumps(DC.VAR_ORDER, indent=2, ensure_ascii=False))
        np.savez(src / "scalers.npz", mean=out["mean"], std=out["std"], n=n)
        np.savez(src / "coords.npz", longitude=DC.LON.astype(np.float32), latitude=DC.LAT.astype(np.float32))
        argv = sys.argv
        sys.argv = ["add_time_features.py", "--src", str(src), "--dst", str(dst)]
        stacked, np_stack = [], np.stack  # main() keeps its (T, 4) float32 features local: listen to np.stack

        def stack(*a, **k):
            stacked.append(np_stack(*a, **k))
            return stacked[-1]

        try:
            np.stack = stack
            with contextlib.redirect_stdout(io.StringIO()):
                atf.main()
        finally:
            sys.argv, np.stack = argv, np_stack
        wide = np.array(np.memmap(dst / "data.npy", dtype=np.float16, mode="r", shape=(DC.T, DC.N_LON, DC.N_LAT, 23)))
        out["wide_data"] = wide
        sc = np.load(dst / "scalers.npz")
        out["wide_mean"], out["wide_std"], out["wide_n"] = sc["mean"], sc["std"], sc["n"]
        out["wide_variables"] = np.array((dst / "variables.json").read_text())
        out["wide_info"] = np.array((dst / "dataset_info.json").read_text())
        assert (np.load(dst / "coords.npz")["longitude"] == DC.LON.astype(np.float32)).all()
    m64, s64 = DC.restate_widened_scalers(wide)
    out["ref_dev_mean"] = np.abs(out["wide_mean"].astype(np.float64) - m64.astype(np.float64))
    out["ref_dev_std"] = np.abs(out["wide_std"].astype(np.float64) - s64.astype(np.float64))

    tf, = [x for x in stacked if x.shape == (DC.T, 4)]  # the reference's own float32 time features
    assert tf.dtype == np.float32 and (tf.astype(np.float16)[:, None, None, :] == wide[..., 19:]).all()
    out["tf"] = tf

    mean, m2, n = np.zeros(5), np.zeros(5), 0
    states = []
    for bs, bq, bn in DC.welford_blocks():
        mean, m2, n = build.welford_update(mean, m2, n, bs, bq, bn)
        states.append((mean.copy(), m2.copy(), n))
    out["welford_mean"] = np.stack([s[0] for s in states])
    out["welford_m2"] = np.stack([s[1] for s in states])
    out["welford_n"] = np.array([s[2] for s in states], dtype=np.int64)

    np.savez_compressed(DC.GOLDEN, **out)
    print(f"wrote {DC.GOLDEN} ({os.path.getsize(DC.GOLDEN) / 1e3:.1f} kB, {len(out)} arrays)")
    print("ref_dev_mean / ulp:", np.round(out["ref_dev_mean"] / DC.ulp32(out["wide_mean"]), 2).max(),
          " ref_dev_std / ulp:", np.round(out["ref_dev_std"] / DC.ulp32(out["wide_std"]), 2).max())


if __name__ == "__main__":
    main()
