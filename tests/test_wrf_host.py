"""The host side of the WRF benchmark (graphcast_lite_amd/wrf.py, predict.save_predictions) against what the reference's
own scripts produced (tests/golden/wrf_vectors.npz, made by tests/golden/make_wrf_golden.py).  No GPU.

Rules:
  point tables     `wrf_point_tables` applied in numpy float64 (the four products added in table order onto 0.0) is
                   bit-equal to the recorded scipy result, NaN outside the axes included
  region rows, matching sample, the 25 / 7 / 3 step rules, match_steps: equal to the recorded values
  table text       built from the recorded domain means, equal to the recorded stdout
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wrf_case as WC  # noqa: E402


@pytest.fixture(scope="module")
def gv():
    return WC.golden()


@pytest.fixture(scope="module")
def W():
    from graphcast_lite_amd import wrf

    return wrf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_point_tables_reproduce_scipy(W, gv):
    fields, lat, lon, times, _ = W.load_wrf_json(WC.WRF_JSON)
    lons, lats = WC.axes()
    pos, w = W.wrf_point_tables(lons, lats, lon, lat)
    assert pos.dtype == np.int32 and pos.shape == (120, 4) and w.dtype == np.float64
    outside = pos[:, 0] < 0
    assert 18 <= outside.sum() <= 30 and (pos[outside] == -1).all() and pos[~outside].min() >= 0
    assert pos.max() < 425
    series = WC.series()
    for a, name in enumerate(("t2m", "10u", "10v", "sp")):
        vi = WC.VAR_NAMES.index(name)
        for h in range(5):
            got = WC.apply_tables(series, pos, w, node_stride=WC.C, offset=(8 + h) * 425 * WC.C + vi)
            want = gv["interp"][a, h].reshape(-1)
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.array_equal(bits(got)[~outside], bits(want)[~outside]), (name, h)
    f32 = series[8, :, :, 0].astype(np.float32) * np.float32(1.5)
    got = WC.apply_tables(f32, pos, w)
    assert np.array_equal(bits(got)[~outside], bits(gv["interp_f32"].reshape(-1))[~outside])
    assert np.isnan(gv["interp_f32"].reshape(-1)[outside]).all()


def test_points_on_the_last_nodes_are_inside(W):
    _, lat, lon, _, _ = W.load_wrf_json(WC.WRF_JSON)
    lons, lats = WC.axes()
    pos, w = W.wrf_point_tables(lons, lats, lon, lat)
    pos, w = pos.reshape(12, 10, 4), w.reshape(12, 10, 4)
    assert lon[5, 9] == 96.0 and pos[5, 9, 0] // 17 == 23  # cell n - 2 ..
    assert w[5, 9, 0] == 0.0 and w[5, 9, 1] == 0.0 and abs(w[5, 9, 2] + w[5, 9, 3] - 1.0) < 1e-15  # .. with all the weight on n - 1
    assert lat[11, 4] == 58.0 and pos[11, 4, 0] % 17 == 15
    assert w[11, 4, 0] == 0.0 and w[11, 4, 2] == 0.0 and abs(w[11, 4, 1] + w[11, 4, 3] - 1.0) < 1e-15
    # strictly outside on either axis: marked, whichever side
    p, _ = W.wrf_point_tables(lons, lats, np.float32([89.99, 96.01, 93.0, 93.0, 93.0]),
                              np.float32([56.0, 56.0, 53.99, 58.01, 56.0]))
    assert (p[:4] == -1).all() and (p[4] >= 0).all()


def test_point_tables_are_cached_and_read_only(W):
    lons, lats = WC.axes()
    q = np.float32([91.3, 95.2]), np.float32([55.1, 57.7])
    a = W.wrf_point_tables(lons, lats, *q)
    b = W.wrf_point_tables(lons, lats, *q)
    assert a[0] is b[0] and a[1] is b[1] and not a[0].flags.writeable
    node_of = WC.flat_order().argsort()
    c = W.wrf_point_tables(lons, lats, *q, node_of=node_of)
    assert np.array_equal(c[0], node_of[a[0]]) and np.array_equal(c[1], a[1])
    with pytest.raises(ValueError):
        W.wrf_point_tables(lons[::-1], lats, *q)
    with pytest.raises(ValueError):
        W.wrf_point_tables(lons, lats, np.float32([np.nan]), np.float32([55.0]))


def test_region_indices(W, gv):
    for flat in (False, True):
        lat, lon = WC.node_coords(flat)
        got = W.wrf_region_indices(lat, lon, flat)
        assert np.array_equal(got, gv["region_flat" if flat else "region_regular"])
    lat, lon = WC.node_coords(False)
    assert np.array_equal(W.wrf_region_indices(lat, lon)[:6], [8 * 17 + 6, 8 * 17 + 7, 8 * 17 + 8, 8 * 17 + 9, 8 * 17 + 10,
                                                              9 * 17 + 6])
    # per-node coordinates of more than 512 nodes are taken as flat without being told
    rng = np.random.default_rng(0)
    la, lo = rng.uniform(54, 58, 600), rng.uniform(90, 96, 600)
    assert np.array_equal(W.wrf_region_indices(la, lo), W.wrf_region_indices(la, lo, True))


def test_matching_sample(W, gv, tmp_path):
    d = WC.dataset_dir(tmp_path / "d", with_series=False)
    for name, offs in WC.OFFSETS.items():
        got = W.find_wrf_matching_sample(d, WC.WRF_JSON, offs, WC.OBS, WC.P)
        assert (-1 if got is None else got) == int(gv[f"match_{name}"]), name
    assert W.find_wrf_matching_sample(tmp_path / "missing", WC.WRF_JSON, [7], WC.OBS) is None
    got = []
    for ts in WC.TIME_FORMATS:
        d = WC.dataset_dir(tmp_path / "f", time_start=ts if ts else None, with_series=False)
        r = W.find_wrf_matching_sample(d, WC.WRF_JSON, WC.OFFSETS["match"], WC.OBS, WC.P)
        got.append(-1 if r is None else r)
    assert got == list(gv["match_formats"]), got
    assert W.wrf_target_offset("2023-01-18", ["2023-01-20_00:00:00"], 2)[0] == 7
    # exact first, then -1, +1, -2, +2
    assert W.match_offset([9, 8, 6, 5], 7)[:2] == (2, -1)
    assert W.match_offset([9, 8, 5], 7)[:2] == (1, 1)
    assert W.match_offset([9, 5], 7)[:2] == (1, -2)


def test_load_wrf_step_rules(W, gv, tmp_path):
    for n in (25, 7, 3):
        path = WC.WRF_JSON if n == 25 else WC.shortened_wrf(tmp_path / f"w{n}.json", n)
        wd = W.load_wrf(str(path), WC.P)
        assert list(wd) == ["t2m", "10u", "10v", "sp"]
        got = np.stack([wd[k] for k in wd])
        assert got.dtype == np.float32 and np.array_equal(got, gv[f"wrf_means_{n}"])
    assert gv["wrf_means_25"].shape == (4, 5) and gv["wrf_means_7"].shape == (4, 5) and gv["wrf_means_3"].shape == (4, 3)
    with pytest.raises(NotImplementedError, match="netCDF"):
        W.load_wrf("wrfout_d03_2023-01-20.nc", 4)


def test_load_wrf_json_and_match_steps(W, gv):
    fields, lat, lon, times, domain = W.load_wrf_json(WC.WRF_JSON)
    assert sorted(fields) == sorted(W.VAR_MAP) and fields["t2_K"].shape == (25, 12, 10)
    assert fields["t2_K"].dtype == np.float32 and lat.dtype == np.float32 and lat.shape == (12, 10) and len(times) == 25
    assert 0.02 < np.isnan(fields["u10_ms"]).mean() < 0.04 and set(domain) == {"lat_min", "lat_max", "lon_min", "lon_max"}
    steps = W.match_steps(WC.TIME_START, times, WC.T)
    assert [(e, w) for e, w, _ in steps] == [tuple(r) for r in gv["match_steps"]]
    assert [s[2] for s in steps] == ["+00h", "+06h", "+12h", "+18h", "+24h"]
    assert len(W.match_steps(WC.TIME_START, times, 11)) == 3 and len(W.match_steps(WC.TIME_START, times[:13], WC.T)) == 3


def test_load_era5(W, tmp_path):
    d = WC.dataset_dir(tmp_path / "e")
    data, lons, lats, names, info = W.load_era5(d)
    assert data.shape == (WC.T, 25, 17, WC.C) and data.dtype == np.float16 and np.array_equal(data, WC.series())
    assert lons.dtype == np.float64 and np.array_equal(lons, WC.axes()[0]) and names == WC.VAR_NAMES
    assert info["time_start"] == WC.TIME_START


@pytest.mark.parametrize("kind,lname", [("regular", "match"), ("regular", "plus2"), ("regular", "none"),
                                        ("flat", "match"), ("legacy", "match")])
def test_table_text_from_recorded_means(W, gv, kind, lname):
    """The tables are the reference's numpy float32 arithmetic on the [n, P, C] means: from the recorded means the text
    is the recorded stdout, character for character."""
    src = "regular" if lname != "match" else kind
    pm, tm = gv[f"{src}_pred_mean"], gv[f"{src}_truth_mean"]
    offs = list(range(pm.shape[0])) if kind == "legacy" else WC.OFFSETS[lname]
    wrf_means = W.load_wrf(WC.WRF_JSON, WC.P)
    _, _, _, times, _ = W.load_wrf_json(WC.WRF_JSON)
    target, lines = W.wrf_target_offset(WC.TIME_START, times, WC.OBS)
    si, _, more = W.match_offset(offs, target)
    text = W.benchmark_tables(pm, tm, WC.VAR_NAMES, wrf_means, si, offs, lines + more)
    assert text["metrics"] + text["wrf"] + text["summary"] == str(gv[f"text_{kind}_{lname}"])
    if lname == "match" and kind != "legacy":
        assert "<- us" in text["wrf"] or "<- WRF" in text["wrf"]
    else:
        assert ("Could not find WRF-matching sample" in text["wrf"]) == (si is None)


def test_table_text_without_wrf(W, gv):
    text = W.benchmark_tables(gv["regular_pred_mean"], gv["regular_truth_mean"], WC.VAR_NAMES, None, None,
                              WC.OFFSETS["match"])
    assert text["wrf"] == "" and "N/A" in text["summary"] and "NOTE:" not in text["summary"]


def test_predictions_round_trip(tmp_path):
    from graphcast_lite_amd import predict

    pred, truth = (torch.from_numpy(x) for x in WC.predictions())
    path = tmp_path / "predictions.pt"
    predict.save_predictions(path, pred, truth, WC.C, WC.P, WC.OBS, 25, 17, sample_offsets=WC.OFFSETS["match"],
                             data_dir="some/dir")
    b = predict.load_predictions(path)
    assert tuple(b) == predict.PREDICTION_KEYS == ("predictions", "ground_truth", "n_features", "ar_steps",
                                                    "obs_window", "n_lon", "n_lat", "sample_offsets", "data_dir")
    assert torch.equal(b["predictions"], pred) and torch.equal(b["ground_truth"], truth)
    assert (b["n_features"], b["ar_steps"], b["obs_window"], b["n_lon"], b["n_lat"]) == (WC.C, WC.P, WC.OBS, 25, 17)
    assert b["sample_offsets"] == WC.OFFSETS["match"] and b["data_dir"] == "some/dir"
    assert predict.save_predictions(path, pred, truth, WC.C, WC.P, WC.OBS, 25, 17)["sample_offsets"] == list(range(6))
    torch.save(pred, path)  # the legacy form comes back as the bare tensor
    assert torch.equal(predict.load_predictions(path), pred)
    with pytest.raises(ValueError):
        predict.save_predictions(path, pred, truth[:, :5], WC.C, WC.P, WC.OBS, 25, 17)
    with pytest.raises(ValueError):
        predict.save_predictions(path, pred, truth, WC.C, WC.P + 1, WC.OBS, 25, 17)
    with pytest.raises(ValueError):
        predict.save_predictions(path, pred, truth, WC.C, WC.P, WC.OBS, 25, 17, sample_offsets=[1, 2])


def test_argument_validation_without_gpu(lib_built, W):
    """Validation that returns before any HIP call: the entry points' own checks and the module's."""
    import ctypes as C

    L = lib_built
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert L.gcl_wrf_box_means(p, 1, 1, p, 0, p, p, 7, 28, 1, p, 28, None, 1, None) == -1
    assert b"empty row list" in L.gcl_last_error()
    assert L.gcl_wrf_box_means(p, 1, 1, p, 3, p, p, 7, 27, 1, p, 28, None, 1, None) == -1
    assert L.gcl_wrf_sample(p, 0, 1, p, p, None, 1, p, p, 4, p, None) == -1
    assert b"go together" in L.gcl_last_error()
    assert L.gcl_wrf_sample(p, 2, 1, p, None, None, 1, p, p, 4, p, None) == -1
    assert L.gcl_wrf_scores_ws_bytes(3, 257) == 3 * 2 * 6 * 8 and L.gcl_wrf_scores_ws_bytes(0, 5) == 0
    none = (None, 0, 0, None, None)
    assert L.gcl_wrf_scores(*none, *none, p, None, p, p, 4, 3, 10, None, 0, None, 0, p, p, 1 << 20, None) == -1
    assert b"multiple of S" in L.gcl_last_error()
    assert L.gcl_wrf_scores(*none, *none, p, None, p, p, 4, 4, 300, None, 0, None, 0, p, p, 8, None) == -1
    assert b"workspace" in L.gcl_last_error()
    assert L.gcl_wrf_scores(p, 0, 1, None, None, *none, p, None, p, p, 4, 4, 300, None, 0, None, 0, p, p, 1 << 20,
                            None) == -1
    mean, std = WC.scalers()
    lat, lon = WC.node_coords(False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.WrfBenchmark(mean, std, WC.VAR_NAMES, lat, lon, WC.P, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        W.interpolate_era5_to_wrf(torch.zeros(25, 17), *WC.axes(), np.zeros((2, 2), np.float32),
                                  np.zeros((2, 2), np.float32))
    with pytest.raises(TypeError):
        W.interpolate_era5_to_wrf(np.zeros((25, 17)), *WC.axes(), np.zeros((2, 2), np.float32),
                                  np.zeros((2, 2), np.float32))
