"""graphcast_lite_amd.dataset against the reference's recorded results (tests/golden/dataset_vectors.npz, made by
tests/golden/make_dataset_golden.py from the reference's download_compute_save, welford_update and add_time_features).

Without a GPU: the numpy restatements of tests/helpers/dataset_case.py reproduce the record exactly (same numpy, same
operations), and so do time_features, the JSON text and the host welford_update of the module.

On the GPU (marked): bytes are compared exactly; mean / std within 1 float32 ulp of the record.  Why 1 ulp: the device
sums differ from numpy's pairwise ones by a reordering of float64 additions (relative 35 * 23 * 2^-53 at most), the
fixture's channels have std >= 0.01 |mean|, so sumsq / n - mean^2 amplifies that by at most 1e4 - still seven orders
below half a float32 ulp (6e-8) - and the final cast rounds two nearby float64 values to the same or adjacent floats.
add_time_features is compared with the float64 restatement of the reference's formula (1 ulp, as above) and with the
reference's own float32 evaluation within ref_dev + 1 ulp, ref_dev being the recorded distance of the latter from the
restatement (triangle inequality).
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dataset_case as DC  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gv():
    return DC.golden()


@pytest.fixture(scope="module")
def fields():
    return {n: DC.raw_field(n) for n in DC.VAR_ORDER}


@pytest.fixture(scope="module")
def ds(lib_built):
    from graphcast_lite_amd import dataset

    return dataset


def close_1ulp(got, want, extra=0.0):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = DC.ulp32(want) + extra
    assert (err <= bound).all(), f"worst error / bound {np.max(err / bound):.3f} at channel {int(np.argmax(err / bound))}"


# ---- without a GPU ----------------------------------------------------------------------------------------------------
def test_restated_build_reproduces_the_reference(gv, fields):
    data, mean, std, n = DC.restate_build(fields, DC.VAR_ORDER, DC.CHUNK)
    assert data.tobytes() == gv["data"].tobytes()
    assert mean.tobytes() == gv["mean"].tobytes() and std.tobytes() == gv["std"].tobytes() and n == int(gv["n"])
    _, mean, std, n = DC.restate_build(fields, DC.VAR_ORDER, DC.CHUNK, start=DC.RESUME_FROM, data=gv["data"])
    assert mean.tobytes() == gv["resume_mean"].tobytes() and std.tobytes() == gv["resume_std"].tobytes()
    assert n == int(gv["resume_n"])
    cf = {n_: DC.const_field(n_) for n_ in DC.CONST_VARS}
    data, mean, std, n = DC.restate_build(cf, DC.CONST_VARS, DC.CONST_CHUNK)
    assert data.tobytes() == gv["const_data"].tobytes() and std[1] == np.float32(1e-6)
    assert mean.tobytes() == gv["const_mean"].tobytes() and std.tobytes() == gv["const_std"].tobytes()


def test_restated_widening_reproduces_the_reference(gv):
    wide = np.concatenate([gv["data"], np.broadcast_to(gv["tf"].astype(np.float16)[:, None, None, :],
                                                       (DC.T, DC.N_LON, DC.N_LAT, 4))], axis=-1)
    assert wide.tobytes() == gv["wide_data"].tobytes()
    m, s = DC.restate_widened_scalers(wide)
    assert (np.abs(m.astype(np.float64) - gv["wide_mean"]) == gv["ref_dev_mean"]).all()
    assert (np.abs(s.astype(np.float64) - gv["wide_std"]) == gv["ref_dev_std"]).all()
    assert int(gv["wide_n"]) == DC.T * DC.N_LON * DC.N_LAT


def test_time_features_and_constants(gv, ds):
    tf = ds.time_features(DC.TIME_START, DC.T)
    assert tf.dtype == np.float32 and tf.shape == (DC.T, 4) and tf.tobytes() == gv["tf"].tobytes()
    assert ds.VAR_ORDER == DC.VAR_ORDER and ds.SCALE_FACTORS == DC.SCALE
    assert json.loads(str(gv["wide_variables"]))[19:] == ds.TIME_FEATURES


def test_host_welford_update_equals_the_reference(gv, ds):
    mean, m2, n = np.zeros(5), np.zeros(5), 0
    for k, (bs, bq, bn) in enumerate(DC.welford_blocks()):
        mean, m2, n = ds.welford_update(mean, m2, n, bs, bq, bn)
        assert mean.tobytes() == gv["welford_mean"][k].tobytes() and m2.tobytes() == gv["welford_m2"][k].tobytes()
        assert n == int(gv["welford_n"][k])
        m_, q_, n_ = DC.welford_step(gv["welford_mean"][k - 1] if k else np.zeros(5),
                                     gv["welford_m2"][k - 1] if k else np.zeros(5),
                                     int(gv["welford_n"][k - 1]) if k else 0, bs, bq, bn)
        assert m_.tobytes() == mean.tobytes() and q_.tobytes() == m2.tobytes() and n_ == n


def test_dataset_info_text(ds):
    """The builder's dataset_info.json is the text the fixture generator handed to the reference's add_time_features."""
    b = ds.DatasetBuilder.__new__(ds.DatasetBuilder)
    b.var_names, b.n_time, b.n_lon, b.n_lat = list(DC.VAR_ORDER), DC.T, DC.N_LON, DC.N_LAT
    b.time_start, b.time_end = DC.TIME_START, DC.TIME_END
    assert json.dumps(b.dataset_info(), indent=2) == DC.build_info_text(DC.VAR_ORDER, DC.T)
    assert list(b.dataset_info()) == ["time_start", "time_end", "n_time", "n_lon", "n_lat", "n_feat", "variables",
                                      "dtype", "file", "size_gb"]


# ---- on the GPU -------------------------------------------------------------------------------------------------------
def read(folder, shape):
    return np.array(np.memmap(os.path.join(folder, "data.npy"), dtype=np.float16, mode="r", shape=shape))


def build(ds, fields, out_dir, stop_after=None, builder=None, names=DC.VAR_ORDER, chunk=DC.CHUNK, scale=None):
    n_time = max(f.shape[0] for f in fields.values() if f.ndim == 3)
    b = builder or ds.DatasetBuilder(names, n_time, DC.N_LON, DC.N_LAT, DC.TIME_START, DC.TIME_END, DEV, out_dir, chunk,
                                     **({} if scale is None else {"scale_factors": scale}))
    for a in range(b.t_done, n_time, chunk):
        if stop_after is not None and a >= stop_after:
            return b
        e = min(a + chunk, n_time)
        b.add_block(a, {n: (f if f.ndim == 2 else f[a:e]) for n, f in fields.items()})
    return b


@pytest.fixture(scope="module")
def built(ds, fields, tmp_path_factory):
    """The uninterrupted build of the fixture's fields, written to a directory: (builder, folder, mean, std, n)."""
    folder = str(tmp_path_factory.mktemp("built"))
    b = build(ds, fields, folder)
    assert os.path.exists(os.path.join(folder, "progress.json"))
    mean, std, n = b.finish(DC.LON, DC.LAT)
    return b, folder, mean, std, n


@gpu
def test_build_gives_the_reference_files(gv, built):
    b, folder, mean, std, n = built
    shape = (DC.T, DC.N_LON, DC.N_LAT, 19)
    assert read(folder, shape).tobytes() == gv["data"].tobytes()
    assert b.series.cpu().numpy().tobytes() == gv["data"].tobytes()
    assert n == int(gv["n"])
    close_1ulp(mean, gv["mean"])
    close_1ulp(std, gv["std"])
    sc = np.load(os.path.join(folder, "scalers.npz"))
    assert sorted(sc.files) == ["mean", "n", "std"] and sc["mean"].dtype == np.float32 and int(sc["n"]) == n
    assert sc["mean"].tobytes() == mean.tobytes() and sc["std"].tobytes() == std.tobytes()
    co = np.load(os.path.join(folder, "coords.npz"))
    assert co["longitude"].dtype == np.float32 and (co["latitude"] == DC.LAT.astype(np.float32)).all()
    assert open(os.path.join(folder, "dataset_info.json")).read() == DC.build_info_text(DC.VAR_ORDER, DC.T)
    assert open(os.path.join(folder, "variables.json")).read() == json.dumps(DC.VAR_ORDER, indent=2, ensure_ascii=False)
    assert not os.path.exists(os.path.join(folder, "progress.json"))


@gpu
def test_build_accepts_device_tensors_and_a_constant_channel(gv, ds):
    cf = {n: torch.from_numpy(DC.const_field(n)).to(DEV) for n in DC.CONST_VARS}
    b = build(ds, cf, None, names=DC.CONST_VARS, chunk=DC.CONST_CHUNK)
    mean, std, n = b.finish(DC.LON, DC.LAT)
    assert b.series.cpu().numpy().tobytes() == gv["const_data"].tobytes() and n == int(gv["const_n"])
    assert mean[1] == gv["const_mean"][1] == 1.0 and std[1] == gv["const_std"][1] == np.float32(1e-6)
    close_1ulp(mean, gv["const_mean"])
    close_1ulp(std, gv["const_std"])


@gpu
def test_resumed_build_follows_the_reference(gv, ds, fields, tmp_path):
    """Stop after two blocks, resume: one chunk back (step 9), the statistics of rows 0-8 from the fp16 on disk - the
    reference's resumed run recorded in the fixture - and the same data.npy and JSON as the uninterrupted build."""
    folder = str(tmp_path)
    build(ds, fields, folder, stop_after=2 * DC.CHUNK)
    assert json.load(open(os.path.join(folder, "progress.json"))) == {"last_completed_timestep": 18, "chunk_size": 9}
    b = ds.DatasetBuilder.resume(folder, DC.VAR_ORDER, DC.T, DC.N_LON, DC.N_LAT, DC.TIME_START, DC.TIME_END, DEV, DC.CHUNK)
    assert b.t_done == DC.RESUME_FROM
    mean, std, n = build(ds, fields, folder, builder=b).finish(DC.LON, DC.LAT)
    assert read(folder, (DC.T, DC.N_LON, DC.N_LAT, 19)).tobytes() == gv["data"].tobytes()
    assert n == int(gv["resume_n"])
    close_1ulp(mean, gv["resume_mean"])
    close_1ulp(std, gv["resume_std"])
    assert open(os.path.join(folder, "dataset_info.json")).read() == DC.build_info_text(DC.VAR_ORDER, DC.T)


@gpu
def test_build_stop_resume_gives_the_same_files(ds, tmp_path):
    """On fields of small whole numbers every value is an fp16 number and every sum is exact, so the statistics a
    resumed build takes from the fp16 on disk are those of the raw fields: all five files equal, byte for byte."""
    rng = np.random.default_rng(5)
    names = ["t2m", "10u", "lsm"]
    f = {"t2m": rng.integers(-40, 40, (DC.T, DC.N_LON, DC.N_LAT)).astype(np.float32),
         "10u": rng.integers(0, 2000, (DC.T, DC.N_LON, DC.N_LAT)).astype(np.float32),
         "lsm": rng.integers(0, 2, (DC.N_LON, DC.N_LAT)).astype(np.float32)}
    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    build(ds, f, one, names=names).finish(DC.LON, DC.LAT)
    build(ds, f, two, names=names, stop_after=2 * DC.CHUNK)
    b = ds.DatasetBuilder.resume(two, names, DC.T, DC.N_LON, DC.N_LAT, DC.TIME_START, DC.TIME_END, DEV, DC.CHUNK)
    assert b.t_done == DC.CHUNK
    build(ds, f, two, builder=b, names=names).finish(DC.LON, DC.LAT)
    assert sorted(os.listdir(one)) == sorted(os.listdir(two)) == ["coords.npz", "data.npy", "dataset_info.json",
                                                                  "scalers.npz", "variables.json"]
    for fn in ("data.npy", "dataset_info.json", "variables.json"):
        assert open(os.path.join(one, fn), "rb").read() == open(os.path.join(two, fn), "rb").read(), fn
    for fn in ("scalers.npz", "coords.npz"):
        a, c = np.load(os.path.join(one, fn)), np.load(os.path.join(two, fn))
        assert a.files == c.files and all(a[k].tobytes() == c[k].tobytes() and a[k].dtype == c[k].dtype for k in a.files)


@gpu
def test_repair_of_overflowed_channels(gv, ds, fields, built):
    """msl, sp and z_surf packed unscaled (Pa, m^2/s^2) are inf in fp16; repair_channels rewrites those columns from the
    raw fields and gives the bytes and (within 1 ulp) the scalers of a correct build.  Like the reference's repair, the
    other channels' statistics come from their fp16 values, so those are compared with the resumed build's rule: the
    numpy restatement of exactly that computation."""
    broken_scale = {k: v for k, v in DC.SCALE.items() if k not in DC.OVERFLOWED}
    b = build(ds, fields, None, scale=broken_scale)
    idx = [DC.VAR_ORDER.index(n) for n in DC.OVERFLOWED]
    before = ds.check_dataset(b.series, verbose=False)
    n_all = DC.T * DC.N_LON * DC.N_LAT
    assert [int(before["inf"][c]) for c in idx] == [n_all] * 3 and int(before["inf"].sum()) == 3 * n_all
    assert int(before["nan"].sum()) == 0

    def blocks():
        for a in range(0, DC.T, DC.CHUNK):
            e = min(a + DC.CHUNK, DC.T)
            yield a, {c: (fields[n] if fields[n].ndim == 2 else fields[n][a:e]) for c, n in zip(idx, DC.OVERFLOWED)}

    series, mean, std, n = ds.repair_channels(b.series, blocks(), {c: DC.SCALE[nm] for c, nm in zip(idx, DC.OVERFLOWED)},
                                              time_chunk=DC.CHUNK)
    assert series.cpu().numpy().tobytes() == gv["data"].tobytes() and n == int(gv["n"])
    after = ds.check_dataset(series, verbose=False)
    assert int(after["inf"].sum()) == 0 and int(after["nan"].sum()) == 0
    # expected scalers: repaired channels from the raw fields (the correct build's), the others from the fp16 data
    _, m16, s16, _ = DC.restate_build(fields, DC.VAR_ORDER, DC.CHUNK, start=DC.T, data=gv["data"])
    want_m, want_s = m16.copy(), s16.copy()
    want_m[idx], want_s[idx] = gv["mean"][idx], gv["std"][idx]
    close_1ulp(mean, want_m)
    close_1ulp(std, want_s)
    close_1ulp(mean[idx], built[2][idx])
    close_1ulp(std[idx], built[3][idx])


@gpu
def test_add_time_features(gv, ds, built, tmp_path):
    _, folder, _, _, _ = built
    dst = str(tmp_path / "wide")
    series = ds.add_time_features(folder, dst)
    shape = (DC.T, DC.N_LON, DC.N_LAT, 23)
    assert series.cpu().numpy().tobytes() == gv["wide_data"].tobytes()
    assert read(dst, shape).tobytes() == gv["wide_data"].tobytes()
    sc = np.load(os.path.join(dst, "scalers.npz"))
    assert int(sc["n"]) == int(gv["wide_n"]) and sc["mean"].dtype == np.float32 and sc["std"].dtype == np.float32
    m64, s64 = DC.restate_widened_scalers(gv["wide_data"])
    close_1ulp(sc["mean"], m64)
    close_1ulp(sc["std"], s64)
    close_1ulp(sc["mean"], gv["wide_mean"], extra=gv["ref_dev_mean"])
    close_1ulp(sc["std"], gv["wide_std"], extra=gv["ref_dev_std"])
    assert open(os.path.join(dst, "variables.json")).read() == str(gv["wide_variables"])
    assert open(os.path.join(dst, "dataset_info.json")).read() == str(gv["wide_info"])
    assert open(os.path.join(dst, "coords.npz"), "rb").read() == open(os.path.join(folder, "coords.npz"), "rb").read()
    out = ds.compare_scalers({"built": folder, "wide": dst}, verbose=False)
    assert list(out["wide"])[:19] == DC.VAR_ORDER and out["built"]["t2m"][0] == float(built[2][0])


@gpu
def test_recompute_scalers_and_check(gv, ds, built, tmp_path):
    """recompute_scalers of a directory = the reference's pass over the fp16 on disk in time_chunk blocks."""
    import shutil

    _, folder, _, _, _ = built
    work = str(tmp_path / "copy")
    shutil.copytree(folder, work)
    mean, std, n = ds.recompute_scalers(work, time_chunk=DC.CHUNK)
    _, m16, s16, n16 = DC.restate_build({k: DC.raw_field(k) for k in DC.VAR_ORDER}, DC.VAR_ORDER, DC.CHUNK, start=DC.T,
                                        data=gv["data"])
    assert n == n16
    close_1ulp(mean, m16)
    close_1ulp(std, s16)
    assert np.load(os.path.join(work, "scalers.npz"))["mean"].tobytes() == mean.tobytes()
    table = ds.check_dataset(work, verbose=False)
    x = gv["data"].astype(np.float32)
    assert (table["min"] == x.min(axis=(0, 1, 2))).all() and (table["max"] == x.max(axis=(0, 1, 2))).all()
    assert table["names"] == DC.VAR_ORDER and (table["stored_mean"] == mean).all()


@gpu
def test_from_series_equals_the_loader_on_the_written_files(ds, built):
    from graphcast_lite_amd.data import TimeseriesChunkDataset

    b, folder, mean, std, _ = built
    disk = TimeseriesChunkDataset(folder, obs_window=2, pred_steps=1, split="all", device=DEV)
    hbm = TimeseriesChunkDataset.from_series(b.series, mean, std, obs_window=2, pred_steps=1, split="all")
    assert len(hbm) == len(disk) == DC.T - 2 and hbm.grid_nodes == disk.grid_nodes
    idx = [0, 7, len(disk) - 1]
    (x0, y0), (x1, y1) = disk.batch(idx), hbm.batch(idx)
    assert torch.equal(x0, x1) and torch.equal(y0, y1) and x0.shape == (3, 35, 38)
    sub = TimeseriesChunkDataset.from_series(b.series, mean, std, split="train", n_features=5)
    ref = TimeseriesChunkDataset(folder, split="train", n_features=5, device=DEV)
    assert len(sub) == len(ref) and torch.equal(sub[3][0], ref[3][0]) and torch.equal(sub[3][1], ref[3][1])
