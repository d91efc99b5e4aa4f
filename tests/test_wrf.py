"""The WRF benchmark module (graphcast_lite_amd/wrf.py) on the GPU against what the reference's own scripts produced
(tests/golden/wrf_vectors.npz, made by tests/golden/make_wrf_golden.py).

Rules:
  interpolate_era5_to_wrf   bit-equal to the recorded scipy fields
  compare_wrf_era5          sums within 4 P 2^-53 sum|x| (two orders of a float64 sum of P terms), so rmse and mae
                            within (4 P + 4) 2^-53 of themselves (the square root and the division add a rounding each)
                            and bias within that of mae; the text equal to the recorded stdout (the generator asserts
                            that every printed number is 1e-6 away from a rounding boundary, the bound is below 1e-9)
  WrfBenchmark              the [n, P, C] means bit-equal to `load_predictions_and_truth(...).mean(axis=1)`, whatever the
                            batching; the table text and the matching sample equal
  on_wrf_grid               the six sums within the bound (P = points x samples added) of numpy on the reference's
                            `interpolate_era5_to_wrf` of the denormalised fields
  CapturedWrfBenchmark      replays from a hipGraph after the warm-up; state bit-equal to the eager one
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wrf_case as WC  # noqa: E402
from layouts import DEV, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
OURS = ("t2m", "10u", "10v", "sp")
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def W(lib_built):
    from graphcast_lite_amd import wrf

    return wrf


@pytest.fixture(scope="module")
def gv():
    return WC.golden()


@pytest.fixture(scope="module")
def wrf_json(W):
    return W.load_wrf_json(WC.WRF_JSON)


def test_interpolate_reproduces_the_fixture(W, gv, wrf_json):
    _, lat, lon, _, _ = wrf_json
    lons, lats = WC.axes()
    series = torch.from_numpy(WC.series()).to(DEV)
    for a, name in enumerate(OURS):
        for h in (0, 4):
            field = series[8 + h, :, :, WC.VAR_NAMES.index(name)]  # a view: read in place with node stride C
            got = W.interpolate_era5_to_wrf(field, lons, lats, lat, lon)
            assert got.is_cuda and got.dtype == torch.float64 and got.shape == (12, 10)
            assert same_bits(got.cpu(), torch.from_numpy(gv["interp"][a, h]))
    f32 = WC.series()[8, :, :, 0].astype(np.float32) * np.float32(1.5)
    got = W.interpolate_era5_to_wrf(f32, lons, lats, lat, lon)  # numpy in, numpy out
    assert isinstance(got, np.ndarray) and same_bits(torch.from_numpy(got), torch.from_numpy(gv["interp_f32"]))
    with pytest.raises(ValueError):
        W.interpolate_era5_to_wrf(series[8, :, :5, 0], lons, lats, lat, lon)


def test_compute_metrics(W, gv, wrf_json):
    fields = wrf_json[0]
    for a, key in enumerate(("u10_ms", "psfc_Pa")):
        ai = list(W.VAR_MAP).index(key)
        conv = fields[key][6] * W.VAR_MAP[key]["era5_to_wrf"]
        truth = gv["interp"][ai, 1]
        got = W.compute_metrics(conv, truth)  # float32 against float64, as the script calls it
        want = gv["era5_results"][ai, 1]
        tol = (4 * 120 + 4) * EPS
        assert abs(got[0] - want[0]) <= tol * want[0] and abs(got[1] - want[1]) <= tol * want[1]
        assert abs(got[2] - want[2]) <= tol * want[1]
        dev = W.compute_metrics(torch.from_numpy(conv).to(DEV), torch.from_numpy(truth).to(DEV))
        assert dev == got
    nan = np.full((3, 4), np.nan, dtype=np.float32)
    assert all(np.isnan(v) for v in W.compute_metrics(nan, np.ones((3, 4), dtype=np.float32)))
    same = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert W.compute_metrics(same, same + 2.0) == (2.0, 2.0, -2.0)
    with pytest.raises(ValueError):
        W.compute_metrics(same, same[:2])


def test_compare_wrf_era5(W, gv, wrf_json):
    series = torch.from_numpy(WC.series()).to(DEV)
    lons, lats = WC.axes()
    results, means, text = W.compare_wrf_era5(wrf_json, series, lons, lats, WC.VAR_NAMES, WC.TIME_START)
    tol = (4 * 120 + 4) * EPS
    for a, name in enumerate(OURS):
        for h, label in enumerate(("+00h", "+06h", "+12h", "+18h", "+24h")):
            got, want = results[name][label], gv["era5_results"][a, h]
            assert abs(got[0] - want[0]) <= tol * want[0], (name, label, got, want)
            assert abs(got[1] - want[1]) <= tol * want[1], (name, label, got, want)
            assert abs(got[2] - want[2]) <= tol * want[1], (name, label, got, want)
            wrf_mean, era5_mean = means[name][label]
            conv = wrf_json[0][list(W.VAR_MAP)[a]][6 * h] * W.VAR_MAP[list(W.VAR_MAP)[a]]["era5_to_wrf"]
            # each side's own nanmean: the reference's is a float32 pairwise sum of <= 120 terms
            assert abs(wrf_mean - np.nanmean(conv)) <= 120 * 2.0 ** -24 * np.nanmean(np.abs(conv))
            f = gv["interp"][a, h]
            assert abs(era5_mean - np.nanmean(f)) <= tol * np.nanmean(np.abs(f))
    assert text == str(gv["era5_text"])
    # a series without sp: the script's SKIP line, no row
    keep = [i for i, n in enumerate(WC.VAR_NAMES) if n != "sp"]
    res2, _, text2 = W.compare_wrf_era5(wrf_json, series[..., keep].contiguous(), lons, lats,
                                        [WC.VAR_NAMES[i] for i in keep], WC.TIME_START)
    assert "sp" not in res2 and "  SKIP sp: not in ERA5 dataset" in text2
    assert res2["t2m"] == results["t2m"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        W.compare_wrf_era5(wrf_json, series.cpu(), lons, lats, WC.VAR_NAMES)


def make_bench(W, flat, cls=None, **kw):
    mean, std = WC.scalers()
    lat, lon = WC.node_coords(flat)
    fields = W.load_wrf_json(WC.WRF_JSON)
    return (cls or W.WrfBenchmark)(mean, std, WC.VAR_NAMES, lat, lon, WC.P, DEV, flat_grid=flat,
                                   wrf_means=W.load_wrf(WC.WRF_JSON, WC.P), wrf_times=fields[3],
                                   time_start=WC.TIME_START, obs_window=WC.OBS, wrf_fields=fields, capacity=8, **kw)


def batches(flat):
    pred, truth = WC.predictions()
    if flat:
        pred, truth = pred[:, WC.flat_order()], truth[:, WC.flat_order()]
    return torch.from_numpy(pred.copy()).to(DEV), torch.from_numpy(truth.copy()).to(DEV)


def feed(bench, flat, split, offsets):
    pred, truth = batches(flat)
    s = 0
    for b in split:
        bench.update(pred[s:s + b], truth[s:s + b], offsets[s:s + b])
        s += b
    return bench


@pytest.mark.parametrize("split", [(6,), (1, 2, 3)])
@pytest.mark.parametrize("flat", [False, True])
def test_benchmark_means_and_text(W, gv, flat, split):
    kind = "flat" if flat else "regular"
    bench = feed(make_bench(W, flat), flat, split, WC.OFFSETS["match"])
    assert bench.launches == 2 * len(split)
    r = bench.results()
    assert r["pred_mean"].dtype == np.float32 and r["pred_mean"].shape == (6, WC.P, WC.C)
    assert same_bits(torch.from_numpy(r["pred_mean"]), torch.from_numpy(gv[f"{kind}_pred_mean"]))
    assert same_bits(torch.from_numpy(r["truth_mean"]), torch.from_numpy(gv[f"{kind}_truth_mean"]))
    assert r["wrf_sample"] == int(gv["match_match"]) and r["sample_offsets"] == WC.OFFSETS["match"]
    t = r["text"]
    assert t["metrics"] + t["wrf"] + t["summary"] == str(gv[f"text_{kind}_match"])
    with pytest.raises(ValueError, match="holds 8 samples"):
        feed(bench, flat, (3,), [20, 21, 22])


@pytest.mark.parametrize("lname", ["plus2", "none"])
def test_benchmark_approximate_and_missing_match(W, gv, lname):
    r = feed(make_bench(W, False), False, (4, 2), WC.OFFSETS[lname]).results()
    want = int(gv[f"match_{lname}"])
    assert (-1 if r["wrf_sample"] is None else r["wrf_sample"]) == want
    t = r["text"]
    assert t["metrics"] + t["wrf"] + t["summary"] == str(gv[f"text_regular_{lname}"])


def grid_check(W, gv, r, what):
    P = 120
    ref = gv["grid_sums"]
    for k, kind in enumerate(W.GRID_KINDS):
        terms = P * (WC.N_SAMPLES if k == 0 else 1)
        for v, name in enumerate(OURS):
            for h in range(WC.P):
                got, want = r["grid_stats"][kind][(name, h)], ref[k, h, v]
                assert got[0] == want[0], (what, kind, name, h)
                mags = gv["grid_mags"][k, h, v]
                for q in range(1, 6):
                    assert abs(got[q] - want[q]) <= WC.sum_bound(terms, mags[q]), (what, kind, name, h, q, got[q], want[q])
                if k > 0:  # one sample: the reference's own compute_metrics on its fields
                    rmse, mae, bias = W.metrics_from_stats(got)
                    m = gv["grid_metrics"][k, h, v]
                    tol = (4 * P + 4) * EPS
                    assert abs(rmse - m[0]) <= tol * m[0] and abs(mae - m[1]) <= tol * m[1]
                    assert abs(bias - m[2]) <= tol * m[1]


def test_on_wrf_grid_scores(W, gv):
    reg = feed(make_bench(W, False, on_wrf_grid=True), False, (1, 2, 3), WC.OFFSETS["match"])
    assert reg.launches == 3 * 3, "two box means and one scoring launch per update"
    r = reg.results()
    assert sorted(r["grid_stats"]) == sorted(W.GRID_KINDS) and all(len(r["grid_stats"][k]) == 16 for k in W.GRID_KINDS)
    grid_check(W, gv, r, "regular")
    assert "FIELD-LEVEL" in r["grid_text"] and r["grid_text"].count("+06h") == 4
    # the flat twin holds the same nodes in another order: the same values through the same tables, the same bits
    flat = feed(make_bench(W, True, on_wrf_grid=True), True, (1, 2, 3), WC.OFFSETS["match"]).results()
    for kind in W.GRID_KINDS:
        for key, st in r["grid_stats"][kind].items():
            assert same_bits(torch.from_numpy(st), torch.from_numpy(flat["grid_stats"][kind][key])), (kind, key)
    # one batch of six adds the samples in the same order
    one = feed(make_bench(W, False, on_wrf_grid=True), False, (6,), WC.OFFSETS["match"]).results()
    for kind in W.GRID_KINDS:
        for key, st in r["grid_stats"][kind].items():
            assert same_bits(torch.from_numpy(st), torch.from_numpy(one["grid_stats"][kind][key])), (kind, key)
    # an approximate match: the WRF sums are those of the sample at target + 2; no match: none
    p2 = feed(make_bench(W, False, on_wrf_grid=True), False, (6,), WC.OFFSETS["plus2"]).results()
    assert p2["wrf_sample"] == 4 and len(p2["grid_stats"]["ours_vs_wrf"]) == 16
    assert p2["grid_stats"]["ours_vs_wrf"][("t2m", 0)][0] == r["grid_stats"]["ours_vs_wrf"][("t2m", 0)][0]
    none = feed(make_bench(W, False, on_wrf_grid=True), False, (6,), WC.OFFSETS["none"]).results()
    assert none["wrf_sample"] is None and none["grid_stats"]["ours_vs_wrf"] == {}
    assert len(none["grid_stats"]["ours_vs_era5"]) == 16


def test_captured_benchmark_replays_and_matches_eager(W):
    pred, truth = batches(False)
    offs = WC.OFFSETS["match"]
    eager = make_bench(W, False, on_wrf_grid=True)
    cap = make_bench(W, False, cls=W.CapturedWrfBenchmark, on_wrf_grid=True)
    for i in range(5):
        for b in (eager, cap):
            b.update(pred[i:i + 1], truth[i:i + 1], offs[i:i + 1])
        if i >= 2:
            assert cap.graph_active, cap.launch_mode
    assert cap.n == eager.n == 5
    torch.cuda.synchronize()
    assert int(cap._count) == 5
    for name in ("_means", "_offs", "_stats", "_filled"):
        assert same_bits(getattr(cap, name), getattr(eager, name)), name
    a, b = cap.results(), eager.results()
    assert a["text"] == b["text"] and a["wrf_sample"] == b["wrf_sample"] == 2 and a["grid_text"] == b["grid_text"]


def test_from_bundle_new_and_legacy(W, gv, tmp_path):
    from graphcast_lite_amd import predict

    d = WC.dataset_dir(tmp_path / "data")
    pred, truth = (torch.from_numpy(x) for x in WC.predictions())
    path = tmp_path / "predictions.pt"
    predict.save_predictions(path, pred, truth, WC.C, WC.P, WC.OBS, 25, 17, sample_offsets=WC.OFFSETS["match"],
                             data_dir=str(d))
    r = W.WrfBenchmark.from_bundle(d, path, ar_steps=WC.P, wrf_path=WC.WRF_JSON, device=DEV, batch_size=4).results()
    assert same_bits(torch.from_numpy(r["pred_mean"]), torch.from_numpy(gv["regular_pred_mean"]))
    assert same_bits(torch.from_numpy(r["truth_mean"]), torch.from_numpy(gv["regular_truth_mean"]))
    t = r["text"]
    assert t["metrics"] + t["wrf"] + t["summary"] == str(gv["text_regular_match"]) and r["wrf_sample"] == 2
    torch.save(pred, path)  # legacy: the bare tensor, truth rebuilt from data.npy
    r = W.WrfBenchmark.from_bundle(d, path, ar_steps=WC.P, wrf_path=WC.WRF_JSON, device=DEV).results()
    assert r["n_samples"] == 2 and r["sample_offsets"] == [0, 1]
    assert same_bits(torch.from_numpy(r["pred_mean"]), torch.from_numpy(gv["legacy_pred_mean"]))
    assert same_bits(torch.from_numpy(r["truth_mean"]), torch.from_numpy(gv["legacy_truth_mean"]))
    t = r["text"]
    assert t["metrics"] + t["wrf"] + t["summary"] == str(gv["text_legacy_match"])
    flat = WC.dataset_dir(tmp_path / "flat", flat=True)
    with pytest.raises(RuntimeError, match="No ground truth"):
        W.WrfBenchmark.from_bundle(flat, path, ar_steps=WC.P, device=DEV)
