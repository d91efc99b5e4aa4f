"""`graphcast_lite_amd.unet_predict`: the regional U-Net forecaster's inference (src/unet/predict.py, predict_v2.py).

CPU: `forecast_tables` against the reference scripts' recorded stdout, the dataset wrapper's checks, the parser, the
architecture detection, and the fixture's own stability.  GPU: `predict_unet` on the fixture experiments against the
recorded accumulators and tables, batch-size and graph invariance, and the launch count.

The fixture (tests/golden/make_unet_forecast_golden.py, case in tests/helpers/unet_forecast_case.py) records, per case,
the accumulators of the reference script's own float32 CPU run ("ref32") and of the float64 restatement of the same loop,
network included ("f64"), and their distance per family (unet_forecast_case.distance): between 6.5e-8 and 1.4e-6 for the
squared-error sums, 4.6e-8 to 1.1e-7 per counted sample for the ACC sums.  The HIP path is allowed MARGIN = 4 times that
distance from f64: the margin of the suite's rule for the U-Nets themselves (unet_case.check), whose summation orders
differ from torch's CPU kernels in the same way.  Measured on an MI355X: 0.06 .. 1.72 times the reference's distance
(worst: sum_se of v1_carry, 5.3e-7 against 3.1e-7).  The generator has checked that no printed digit outside
unet_forecast_case.UNSTABLE moves when the float64 accumulators are moved by the whole tolerance, so the tables are
compared character for character."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_forecast_case as FC  # noqa: E402

DEV = "cuda:0"
CASE_IDS = list(FC.CASES)


@pytest.fixture(scope="module")
def rec():
    npz, js = FC.recorded()
    return {"npz": npz, "json": js}


def _names(case):
    return FC.load_dataset(FC.CASES[case][1])[3]


def _tables(case, acc, n):
    from graphcast_lite_amd.unet_predict import forecast_tables

    _, _, static, forcing, _ = FC.CASES[case]
    return forecast_tables(acc, _names(case), static, forcing, FC.N_LAT, FC.N_LON, n)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_IDS)
def test_tables_reproduce_the_reference_stdout(rec, case):
    """From the script's recorded accumulators, the script's recorded stdout, character for character."""
    got = _tables(case, FC.recorded_acc(rec["npz"], case, "ref32"), rec["json"][case]["n_samples"])
    assert got == rec["json"][case]["tables"]


def test_tables_cover_the_formats(rec):
    """The fixture exercises what the tables can print: the degree and metre formats, both tags, a horizon past
    pred_steps (count 0: the max(count, 1) rows)."""
    long = rec["json"]["v2_long"]["tables"]
    assert "°C" in long and "m²/s²" in long and "(static)" in long and "(forcing)" in long
    assert "+30h: avg_skill=0.0% | ACC=0.0000" in long and "AR=5" in long
    assert rec["npz"]["v2_long.ref32.count"].tolist() == [540, 540, 540, 0, 0]
    assert "(static)" in rec["json"]["v1_carry"]["tables"] and "lsm" in rec["json"]["v1_carry"]["tables"]


@pytest.mark.parametrize("case", CASE_IDS)
def test_fixture_tables_are_stable_under_the_tolerance(rec, case):
    """The float64 accumulators moved by MARGIN x the recorded distance either way print the reference's digits: the GPU
    test may compare the tables exactly.  The unstable cells are listed by name and are at most 5 % of the cells."""
    d, n = rec["json"][case]["distance"], rec["json"][case]["n_samples"]
    want = FC.mask_unstable(case, rec["json"][case]["tables"])
    f64 = FC.recorded_acc(rec["npz"], case, "f64")
    for sign in (0.0, -1.0, 1.0):
        assert FC.mask_unstable(case, _tables(case, FC.perturbed(f64, d, sign), n)) == want, sign
    ar, C = f64["sum_se"].shape
    cells = 2 * ar + ar * C + 3 * C + 2
    assert len(FC.UNSTABLE.get(case, [])) <= 0.05 * cells


def test_guess_unit_and_tags():
    from graphcast_lite_amd.unet_predict import _guess_unit

    assert [_guess_unit(n) for n in ("t2m", "T@850", "u10", "v@500", "msl", "sp", "z@500", "z_sfc", "tp", "tcwv", "q@700", "lsm",
                                     "toa")] == ["K", "K", "m/s", "m/s", "Pa", "Pa", "m²/s²", "m²/s²", "m", "m/s", "kg/m²", "-", "?"]


class _FakeChunks:
    def __init__(self, flat):
        self.flat_grid, self.n_lon, self.n_lat, self.n_feat = flat, None if flat else 12, None if flat else 9, 6
        self.obs_window, self.pred_steps = 2, 3
        self._sample_indices = [(0, t) for t in range(5)]

    def __len__(self):
        return len(self._sample_indices)


def test_grid2d_dataset_argument_checks():
    from graphcast_lite_amd.unet_predict import Grid2DDataset

    with pytest.raises(ValueError, match="regular grid"):
        Grid2DDataset(_FakeChunks(flat=True))
    ds = Grid2DDataset(_FakeChunks(flat=False))
    assert (ds.H, ds.W, len(ds), ds.channels) == (9, 12, 5, 6)
    assert ds.window_starts([0, 4, -1]) == [(0, 0), (0, 4), (0, 4)]
    with pytest.raises(IndexError, match="outside"):
        ds.window_starts([5])
    with pytest.raises(ValueError, match="no samples"):
        ds.batch([])


def test_channel_kinds():
    from graphcast_lite_amd.unet_predict import channel_kinds

    assert channel_kinds(6, [4, 3], [3]).tolist() == [0, 0, 0, 2, 1, 0]
    with pytest.raises(ValueError, match="forcing channel 6"):
        channel_kinds(6, [], [6])


def test_parser_defaults_are_the_scripts():
    from graphcast_lite_amd.unet_predict import build_parser

    a = build_parser().parse_args(["experiments/unet_region_krsk"])
    assert (a.experiment_dir, a.ckpt, a.ar_steps, a.max_samples, a.data_dir) == ("experiments/unet_region_krsk", None, None, 200, None)
    assert (a.arch, a.batch_size) == ("auto", 8)
    a = build_parser().parse_args(["e", "--ckpt", "m.pth", "--ar-steps", "4", "--max-samples", "7", "--data-dir", "d", "--arch", "v2",
                                   "--batch-size", "3"])
    assert (a.ckpt, a.ar_steps, a.max_samples, a.data_dir, a.arch, a.batch_size) == ("m.pth", 4, 7, "d", "v2", 3)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["e", "--arch", "v3"])


def test_arch_auto_on_both_checkpoints():
    from graphcast_lite_amd.unet import WeatherUNet
    from graphcast_lite_amd.unet_predict import detect_arch
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    sd1 = torch.load(FC.CKPT["v1"], map_location="cpu", weights_only=True)
    sd2 = torch.load(FC.CKPT["v2"], map_location="cpu", weights_only=True)
    assert detect_arch(sd1, FC.OBS * FC.C, FC.C, FC.BASE) == "v1" and detect_arch(sd2, FC.OBS * FC.C, FC.C, FC.BASE) == "v2"
    WeatherUNet(FC.OBS * FC.C, FC.C, FC.BASE).load_state_dict(sd1, strict=True)
    WeatherUNetV2(FC.OBS * FC.C, FC.C, FC.BASE, FC.HEADS, FC.MODES).load_state_dict(sd2, strict=True)


def test_config_defaults_are_the_scripts(tmp_path, monkeypatch):
    """obs_window 2, pred_steps 4, base_filters 64, max_ar_steps -> pred_steps, the split test_only, scalers cut to C."""
    import json

    from graphcast_lite_amd import unet_predict as UP

    seen = {}

    class Stop(Exception):
        pass

    def fake_dataset(data_dir, obs, pred, split, n_features, device):
        seen.update(data_dir=data_dir, obs=obs, pred=pred, split=split, n_features=n_features)
        raise Stop

    monkeypatch.setattr(UP, "TimeseriesChunkDataset", fake_dataset)
    (tmp_path / "config.json").write_text(json.dumps({"data_dir": "somewhere", "num_features": 19}))
    with pytest.raises(Stop):
        UP.predict_unet(str(tmp_path))
    assert seen == {"data_dir": "somewhere", "obs": 2, "pred": 4, "split": "test_only", "n_features": 19}
    with pytest.raises(ValueError, match="arch"):
        UP.predict_unet(str(tmp_path), arch="v3")


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _predict(case, **kw):
    from graphcast_lite_amd.unet_predict import predict_unet

    arch, data, _, _, ar = FC.CASES[case]
    return predict_unet(FC.exp_dir(case), ckpt=FC.CKPT[arch], data_dir=data, ar_steps=ar, device=DEV, **kw)


_RUNS = {}


def _run(case, **kw):
    """One `predict_unet` per (case, options), shared by the tests."""
    key = (case, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _RUNS[key] = _predict(case, **kw)
    return _RUNS[key]


def _same_results(a, b):
    keys = FC.FAMILIES + ("acc_count", "count")
    return all(np.array_equal(np.asarray(a[k]).view(np.int64), np.asarray(b[k]).view(np.int64)) for k in keys) \
        and a["tables"] == b["tables"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
def test_predict_unet_against_the_reference(rec, case):
    """The accumulators within MARGIN x the reference's own float32 / float64 distance of the float64 restatement, per
    family (recorded distances: see the module docstring); the counts equal; the tables equal to the reference's stdout
    outside the cells listed in unet_forecast_case.UNSTABLE."""
    res = _run(case)
    arch = FC.CASES[case][0]
    assert res["arch"] == arch and res["n_samples"] == rec["json"][case]["n_samples"] and (res["H"], res["W"]) == (FC.N_LAT, FC.N_LON)
    f64, ref32 = FC.recorded_acc(rec["npz"], case, "f64"), FC.recorded_acc(rec["npz"], case, "ref32")
    assert np.array_equal(res["count"], ref32["count"])
    unstable = [c for c, _ in FC.UNSTABLE.get(case, [])]
    keep = np.ones(f64["acc_count"].shape[1], dtype=bool)
    keep[unstable] = False
    assert np.array_equal(res["acc_count"][:, keep], f64["acc_count"][:, keep])
    assert np.array_equal(res["acc_count"][:, keep], ref32["acc_count"][:, keep])
    got = {k: np.where(keep[None, :], res[k], f64[k]) for k in FC.FAMILIES + ("acc_count",)}
    d_hip, d_ref = FC.distance(got, f64), rec["json"][case]["distance"]
    for k in FC.FAMILIES:
        print(f"[unet_forecast] {case} {k}: d(hip, f64) = {d_hip[k]:.3e}, d(ref32, f64) = {d_ref[k]:.3e}, "
              f"ratio {d_hip[k] / max(d_ref[k], 1e-300):.2f}")
    for k in FC.FAMILIES:
        assert d_hip[k] <= FC.MARGIN * d_ref[k], f"{case} {k}: {d_hip[k]:.3e} above {FC.MARGIN} x {d_ref[k]:.3e}"
    assert FC.mask_unstable(case, res["tables"]) == FC.mask_unstable(case, rec["json"][case]["tables"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["v1_carry", "v2_long"])
def test_squared_error_sums_against_numpy_float32(case):
    """With the network's output taken as given (the `pred` of the step kernel), the squared-error sums of a sample
    against numpy's float32 pairwise `.sum()` of the same float32 squares (predict_v2.py:159-163).  numpy adds blocks of
    128 terms with eight accumulators (16 + 3 roundings) and the blocks in a tree of depth ceil(log2(HW / 128)); the
    float64 sums here round at 2^-53.  For non-negative terms the gap is at most (16 + 3 + depth) 2^-24 relative."""
    from graphcast_lite_amd import hip

    arch, data, static, forcing, _ = FC.CASES[case]
    series, mean, std, _ = FC.load_dataset(data)
    kind = FC.kinds_of(FC.C, static, forcing)
    starts = FC.split_starts()
    B, H, W, HW = len(starts), FC.N_LAT, FC.N_LON, FC.N_LAT * FC.N_LON
    bound = (16 + 3 + max(0, math.ceil(math.log2(HW / 128)))) * 2.0 ** -24
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in {"series": series, "mean": mean, "std": std, "kind": kind}.items()}
    rng = np.random.default_rng(3)
    X = np.stack([FC.window_np(series, t, mean, std, FC.C, 0, FC.OBS) for t in starts])
    out = (X[:, FC.C:] + 0.1 * rng.standard_normal((B, FC.C, H, W))).astype(np.float32)
    worst = 0.0
    for b in range(B):  # one sample per call: the state is that sample's sums
        state = torch.zeros(1, FC.C, 5, dtype=torch.float64, device=DEV)
        pred = torch.empty(1, FC.C, H, W, device=DEV)
        hip.grid_forecast_step(torch.from_numpy(out[b:b + 1]).to(DEV), torch.from_numpy(X[b:b + 1]).to(DEV), dev["series"],
                               torch.tensor([starts[b]], device=DEV), dev["kind"], dev["mean"], dev["std"], 0,
                               torch.empty(1, FC.OBS * FC.C, H, W, device=DEV), state,
                               torch.zeros(1, FC.C, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV),
                               pred=pred)
        p, got = pred[0].cpu().numpy(), state[0].cpu().numpy()
        g = FC.window_np(series, starts[b], mean, std, FC.C, FC.OBS, 1)
        bl = X[b, FC.C:]
        for c in range(FC.C):
            pp, gp, bp = p[c] * std[c] + mean[c], g[c] * std[c] + mean[c], bl[c] * std[c] + mean[c]
            want = [((pp - gp) ** 2).sum(), ((bp - gp) ** 2).sum(), ((p[c] - g[c]) ** 2).sum(), ((bl[c] - g[c]) ** 2).sum()]
            for k in range(4):
                assert want[k].dtype == np.float32
                gap = abs(got[c, k] - float(want[k])) / float(want[k]) if want[k] > 0 else abs(got[c, k])
                worst = max(worst, gap)
                assert gap <= bound, f"sample {b} channel {c} sum {k}: {got[c, k]!r} against {float(want[k])!r}, gap {gap:.3e} > {bound:.3e}"
    print(f"[unet_forecast] {case}: worst gap to numpy's float32 sums {worst:.3e} (bound {bound:.3e})")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["v1_carry", "v2_long"])
def test_batch_size_does_not_reach_the_bits(case):
    """Five samples in batches of 1, 3 (a tail of two) and 8 (one padded batch): equal bits, equal tables."""
    base = _run(case)
    for bs in (1, 3):
        assert _same_results(_run(case, batch_size=bs), base), f"batch_size {bs}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["v1_carry", "v2_long"])
def test_captured_equals_eager(case):
    """Batches of one so that the graph is captured (after two eager warm-up calls) and replayed within five samples."""
    from graphcast_lite_amd.data import TimeseriesChunkDataset
    from graphcast_lite_amd.unet_predict import GridForecaster, Grid2DDataset

    eager = _run(case, batch_size=1, use_graph=False)
    graph = _run(case, batch_size=1, use_graph=True)
    assert _same_results(eager, graph)
    arch, data, static, forcing, ar = FC.CASES[case]
    ds = Grid2DDataset(TimeseriesChunkDataset(data, FC.OBS, FC.PRED, split="test_only", n_features=FC.C, device=DEV))
    f = GridForecaster(_model(arch), ds, static, forcing, ar, batch_size=1, use_graph=True).run(len(ds))
    assert f.graph_active, "the graph path stayed eager"
    assert np.array_equal(f.results()["sum_se"].view(np.int64), eager["sum_se"].view(np.int64))


def _model(arch):
    from graphcast_lite_amd.unet import WeatherUNet
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    m = WeatherUNet(FC.OBS * FC.C, FC.C, FC.BASE) if arch == "v1" else WeatherUNetV2(FC.OBS * FC.C, FC.C, FC.BASE, FC.HEADS, FC.MODES)
    m.load_state_dict(torch.load(FC.CKPT[arch], map_location="cpu", weights_only=True), strict=True)
    return m.to(DEV).eval()


@pytest.mark.gpu
@pytest.mark.parametrize("arch", ["v1", "v2"])
def test_launch_count_per_batch(arch):
    """1 (the pack) + AR x (the network's launches + the step's 3), from the sections' launch counters."""
    from graphcast_lite_amd import hip
    from graphcast_lite_amd.data import TimeseriesChunkDataset
    from graphcast_lite_amd.unet_predict import GridForecaster, Grid2DDataset

    ds = Grid2DDataset(TimeseriesChunkDataset(FC.DATA, FC.OBS, FC.PRED, split="test_only", n_features=FC.C, device=DEV))
    model = _model(arch)
    f = GridForecaster(model, ds, [5], [3], ar_steps=2, batch_size=3, use_graph=False)
    f.update([0, 1, 2])  # packs the weights
    torch.cuda.synchronize()

    def counters():
        return hip.unet_forecast_launches(), hip.unet_launches() + hip.unet_v2_launches()

    glue0, net0 = counters()
    model(f._windows[0], residual_from=(FC.C, 2 * FC.C))
    net_launches = counters()[1] - net0
    assert net_launches == (15 if arch == "v1" else 72)
    glue0, net0 = counters()
    f.update([3, 4])
    glue, net = counters()
    assert glue - glue0 == 1 + 2 * 3 and net - net0 == 2 * net_launches
    assert f.results()["count"].tolist() == [5 * FC.N_LAT * FC.N_LON] * 2


@pytest.mark.gpu
def test_grid2d_dataset_is_the_reference_wrapper():
    """`ds[i]` and `ds.batch` against the numpy restatement of the loader + Grid2DDataset, bit for bit."""
    from graphcast_lite_amd.data import TimeseriesChunkDataset
    from graphcast_lite_amd.unet_predict import Grid2DDataset

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
    from layouts import same_bits

    series, mean, std, _ = FC.load_dataset(FC.DATA)
    ds = Grid2DDataset(TimeseriesChunkDataset(FC.DATA, FC.OBS, FC.PRED, split="test_only", n_features=FC.C, device=DEV))
    starts = FC.split_starts()
    assert len(ds) == len(starts) and ds.window_starts(range(len(ds))) == [(0, t) for t in starts]
    X, Y = ds[1]
    assert same_bits(X.cpu(), torch.from_numpy(FC.window_np(series, starts[1], mean, std, FC.C, 0, FC.OBS)))
    assert same_bits(Y.cpu(), torch.from_numpy(FC.window_np(series, starts[1], mean, std, FC.C, FC.OBS, FC.PRED)))
    out = torch.empty(3, FC.OBS * FC.C, FC.N_LAT, FC.N_LON, device=DEV)
    assert ds.batch([4, 0, 2], out=out) is out
    for b, i in enumerate([4, 0, 2]):
        assert same_bits(out[b].cpu(), torch.from_numpy(FC.window_np(series, starts[i], mean, std, FC.C, 0, FC.OBS)))
