"""Per-grid-point error maps (verify.MetricMaps, csrc/maps.hip) against the reference's `scripts/metrics_maps.py`:
fixtures of tests/golden/make_maps_golden.py.  The float64 restatement stored there (x64_*) is the arbiter: the sums
here are float64 and the result is rounded to float32 once, so a map may differ from it by one float32 ulp of the value
plus 2^-40 of the node's error scale (a bias that cancels to nearly zero), and is never further from it than the
reference's own float32 arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, experiment

DEV = "cuda:0"
STATS = ("rmse", "mae", "bias", "acc")
CONST_CH = 7  # constant in the truth


@pytest.fixture(scope="module")
def Z():
    return np.load(os.path.join(GOLDEN, "maps_vectors.npz"))


def _V():
    from graphcast_lite_amd import verify

    return verify


def _names(Z):
    return [str(n) for n in Z["unit_names"]]


def _case(Z, **kw):
    V = _V()
    names = _names(Z)
    args = dict(leads=2, var_order=names, y_mean=Z["y_mean"], y_scale=Z["y_scale"])
    args.update(kw)
    return V.MetricMaps(len(names), Z["all_t"].shape[1], **args)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------------------
# Without a GPU
# ----------------------------------------------------------------------------------------------------------------------
def test_unit_label_matches_reference(Z):
    V = _V()
    assert len(Z["unit_names"]) == 8
    for i, name in enumerate(_names(Z)):
        want = (str(Z["unit_label"][i]), float(Z["unit_factor"][i]), float(Z["unit_offset"][i]),
                str(Z["unit_special"][i]) or None)
        assert V.unit_label(name) == want, name
    mm = V.MetricMaps(8, 16, var_order=_names(Z))
    assert mm.units == [str(u) for u in Z["unit_label"]]
    assert V.MetricMaps(3, 16).units == ["", "", ""]


def test_to_grid_matches_plot_field(Z):
    V = _V()
    n_lon, n_lat = (int(v) for v in Z["grid_shape"])
    got = V.MetricMaps.to_grid(torch.from_numpy(Z["grid_field"]), n_lon, n_lat)
    assert got.shape == (n_lat, n_lon) and np.array_equal(got, Z["grid_out"])
    assert np.array_equal(V.MetricMaps(1, n_lon * n_lat).to_grid(Z["grid_field"], n_lon, n_lat), Z["grid_out"])


def test_maps_before_any_update_are_zero():
    V = _V()
    mm = V.MetricMaps(3, 10, leads=2, rows=[1, 4, 7])
    assert mm.n == 0
    for s in STATS:
        m = mm.maps(s)
        assert m.shape == (2, 3, 3) and m.dtype == torch.float32 and not m.any()
    assert mm.map("rmse", 1, lead=1).shape == (3,)
    mm.reset()
    assert mm.n == 0


def test_argument_errors(tmp_path):
    V = _V()
    with pytest.raises(ValueError, match="var_order"):
        V.MetricMaps(3, 10, var_order=["t2m", "msl"])
    with pytest.raises(ValueError, match="unknown statistic"):
        V.MetricMaps(3, 10, stats=("rmse", "crps"))
    with pytest.raises(ValueError, match="y_mean"):
        V.MetricMaps(3, 10, y_mean=np.zeros(3))
    with pytest.raises(ValueError, match="y_mean"):
        V.MetricMaps(3, 10, leads=2, y_mean=np.zeros(4), y_scale=np.ones(4))
    with pytest.raises(ValueError, match="rows"):
        V.MetricMaps(3, 10, rows=[3, 10])
    mm = V.MetricMaps(3, 10, leads=2, stats=("rmse", "bias"))
    with pytest.raises(ValueError, match="unknown statistic"):
        mm.maps("crps")
    with pytest.raises(ValueError, match="not accumulated"):
        mm.maps("acc")
    with pytest.raises(ValueError, match="not accumulated"):
        V.MetricMaps(3, 10, stats=("mae",)).skill(mm)
    with pytest.raises(ValueError, match="GPU"):
        mm.update(torch.zeros(10, 6), torch.zeros(10, 6))
    with pytest.raises(ValueError, match="GPU"):
        mm.update(torch.zeros(2, 10, 6), V.Persistence(torch.zeros(2, 10, 9), 3))
    with pytest.raises(ValueError, match="GPU"):
        V.MetricMaps(3, 10, device="cpu")
    for shape in ((10, 3), (10, 7), (9, 6), (2, 10, 5)):
        with pytest.raises(ValueError, match="2 leads x 3 channels"):
            mm.update(torch.zeros(*shape), torch.zeros(*shape))
    with pytest.raises(ValueError, match="2 leads x 3 channels"):
        mm.update(torch.zeros(10, 6), torch.zeros(10, 3))
    with pytest.raises(ValueError):
        V.compute_stat(torch.zeros(2, 4), torch.zeros(2, 4), "crps")
    with pytest.warns(RuntimeWarning, match="standardised units"):
        assert V.load_scaler_stats(tmp_path) is None
    np.savez(tmp_path / "scalers.npz", y_mean=np.arange(3.0), y_scale=np.ones(3))
    st = V.load_scaler_stats(tmp_path)
    assert sorted(st) == ["y_mean", "y_scale"] and np.array_equal(st["y_mean"], np.arange(3.0))


def test_helpers_reject_host_tensors(Z):
    """The conversion helpers run on the GPU only, like every other entry of the package."""
    V = _V()
    t = torch.from_numpy(Z["all_t"][..., :8])
    with pytest.raises(ValueError, match="GPU"):
        V.inverse_standardize(t, Z["y_mean"], Z["y_scale"])
    with pytest.raises(ValueError, match="GPU"):
        V.apply_units(t[..., 4], "z@500")
    with pytest.raises(ValueError, match="GPU"):
        V.compute_stat(t[0].T, t[1].T, "rmse")


def test_maps_abi_validates_before_any_hip_call(lib_built):
    L = lib_built
    buf = (C.c_double * 64)()
    cnt = (C.c_int64 * 1)()
    f = (C.c_float * 64)()
    p, pf, pc = C.addressof(buf), C.addressof(f), C.addressof(cnt)
    assert L.gcl_maps_colstats_ws_bytes(0, 4, 1) == 0 and L.gcl_maps_colstats_ws_bytes(1000, 19, 2) > 0
    assert L.gcl_maps_colstats(None, 4, 0, pf, 4, 0, None, 4, None, None, None, 4, 1, p, p, 64, None) == -1
    assert b"maps_colstats" in L.gcl_last_error()
    assert L.gcl_maps_colstats(pf, 4, 0, pf, 4, 0, None, 4, None, None, None, 4, 1, p, p, 8, None) == -1
    assert b"workspace" in L.gcl_last_error()
    assert L.gcl_maps_accumulate(pf, 4, 0, pf, 4, 0, None, 1, 4, None, None, None, 4, 1, None, 0, p, pc, None) == -1
    assert b"sums" in L.gcl_last_error()
    assert L.gcl_maps_accumulate(pf, 4, 0, pf, 4, 0, None, 1, 4, None, None, None, 4, 1, None, 8, p, pc, None) == -1
    assert b"column statistics" in L.gcl_last_error()
    assert L.gcl_maps_accumulate(pf, 4, 0, pf, 4, 0, None, 1, 4, None, None, None, 0, 1, None, 2, p, pc, None) == -1
    assert L.gcl_maps_accumulate(pf, 4, 0, pf, 4, 0, None, 1, 4, None, None, None, 4, 1, None, 2, p, None, None) == -1
    assert L.gcl_maps_finalize(p, pc, 2, 2, 1, 16, 0, None, None, 0, 0, pf, None) == -1
    assert b"plane" in L.gcl_last_error()
    assert L.gcl_maps_finalize(p, pc, 0, 1, 1, 16, 4, None, None, 0, 0, pf, None) == -1
    assert b"skill" in L.gcl_last_error()
    assert L.gcl_maps_finalize(p, pc, 0, 1, 1, 16, 7, None, None, 0, 0, pf, None) == -1
    assert L.gcl_maps_convert(pf, pf, 16, 4, None, None, None) == -1
    assert L.gcl_maps_convert(pf, pf, 16, 0, pf, pf, None) == -1
    assert cnt[0] == 0 and not any(buf)


# ----------------------------------------------------------------------------------------------------------------------
# On the GPU
# ----------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _check_against_arbiter(Z, tag, mm):
    for stat in STATS:
        got = mm.maps(stat)
        assert got.dtype == torch.float32 and got.is_cuda
        got = got.cpu().numpy().astype(np.float64)
        x64, ref = Z[f"{tag}_x64_{stat}"], Z[f"{tag}_ref_{stat}"].astype(np.float64)
        assert got.shape == x64.shape
        scale = np.ones_like(x64) if stat == "acc" else Z[f"{tag}_x64_mae"]
        err = np.abs(got - x64)
        bound = _ulp32(x64) + 2.0 ** -40 * scale
        worst = float((err / bound).max())
        print(f"{tag} {stat}: max|got - x64| = {err.max():.3e}, max|ref - x64| = {np.abs(ref - x64).max():.3e}, "
              f"worst err / bound = {worst:.3f}")
        assert np.all(err <= bound), f"{tag} {stat}: {worst:.3f} of the bound"
        keep = [c for c in range(x64.shape[-1]) if not (stat == "acc" and c == CONST_CH)]
        assert err[..., keep].max() <= np.abs(ref - x64)[..., keep].max(), f"{tag} {stat}: further off than the reference"
    # the truth of this channel is constant: its anomaly is exactly zero here (the reference's float32 value there,
    # |ref| up to ~1e4, is rounding noise divided by 1e-8)
    acc = mm.maps("acc")[..., CONST_CH]
    assert not acc.any()


@pytest.mark.gpu
def test_conversion_is_bit_equal(Z, lib_built):
    V = _V()
    names, Cn = _names(Z), len(Z["unit_names"])
    for src, conv in (("all_t", "all_conv_t"), ("all_p", "all_conv_p")):
        for lead in range(2):
            x = _dev(Z[src][..., lead * Cn:(lead + 1) * Cn])
            phys = V.inverse_standardize(x, Z["y_mean"], Z["y_scale"])
            assert phys.is_cuda and phys.dtype == torch.float32
            for c, name in enumerate(names):
                got, label = V.apply_units(phys[..., c], name)
                assert label == str(Z["unit_label"][c]) and got.is_cuda
                assert torch.equal(got.cpu(), torch.from_numpy(Z[conv][..., lead * Cn + c])), (src, lead, name)


@pytest.mark.gpu
def test_maps_against_float64_arbiter(Z, lib_built):
    V = _V()
    mm = _case(Z, device=DEV)
    mm.update(_dev(Z["all_t"]), _dev(Z["all_p"]))
    assert mm.n == 6
    _check_against_arbiter(Z, "all", mm)
    rg = _case(Z, rows=Z["reg_rows"])
    rg.update(_dev(Z["all_t"]), _dev(Z["all_p"]))
    assert rg.maps("rmse").shape == (2, len(Z["reg_rows"]), 8)
    _check_against_arbiter(Z, "reg", rg)
    # the one-shot form on already converted values
    Cn = 8
    for stat in STATS:
        for k in (2, Cn + 4):  # msl of lead 0, z@500 of lead 1
            got = V.compute_stat(_dev(Z["all_conv_p"][..., k]), _dev(Z["all_conv_t"][..., k]), stat)
            assert _bits(got, mm.maps(stat)[k // Cn, :, k % Cn].contiguous()), (stat, k)
    # identity units, standardised values
    plain = V.MetricMaps(8, 512, leads=2, stats=("mae",))
    plain.update(_dev(Z["all_t"]), _dev(Z["all_p"]))
    want = np.abs(Z["all_p"].astype(np.float64) - Z["all_t"]).mean(axis=0).reshape(512, 2, 8).transpose(1, 0, 2)
    assert np.array_equal(plain.maps("mae").cpu().numpy(), want.astype(np.float32))


@pytest.mark.gpu
def test_streaming_invariance(Z, lib_built):
    t, p = _dev(Z["all_t"]), _dev(Z["all_p"])
    one = _case(Z)
    one.update(t, p)

    def same(a, b):
        assert a.n == b.n and _bits(a._state, b._state)
        for s in STATS:
            assert _bits(a.maps(s), b.maps(s)), s

    six = _case(Z)
    for b in range(6):
        six.update(t[b:b + 1], p[b:b + 1])
    same(one, six)
    two_d = _case(Z)
    for b in range(6):
        two_d.update(t[b], p[b])
    same(one, two_d)
    again = _case(Z)
    again.update(t, p)
    same(one, again)
    # each lead alone: a strided slice (element kernel) and a contiguous copy (16-byte kernel)
    for lead in range(2):
        for copy in (False, True):
            tl, pl = t[..., lead * 8:(lead + 1) * 8], p[..., lead * 8:(lead + 1) * 8]
            if copy:
                tl, pl = tl.contiguous(), pl.contiguous()
            alone = _case(Z, leads=1)
            alone.update(tl, pl)
            assert _bits(alone._state[0], one._state[lead]), (lead, copy)
            for s in STATS:
                assert _bits(alone.maps(s)[0], one.maps(s)[lead]), (lead, copy, s)
    # a region through the row list, and its rows gathered into tensors of their own
    rows = torch.from_numpy(Z["reg_rows"]).to(DEV)
    rg = _case(Z, rows=Z["reg_rows"])
    rg.update(t, p)
    V = _V()
    gathered = V.MetricMaps(8, len(Z["reg_rows"]), leads=2, var_order=_names(Z), y_mean=Z["y_mean"], y_scale=Z["y_scale"])
    gathered.update(t[:, rows].contiguous(), p[:, rows].contiguous())
    same(rg, gathered)
    one.reset()
    assert one.n == 0 and not one._state.any()


@pytest.mark.gpu
@pytest.mark.parametrize("leads,B", [(1, 8), (3, 4), (1, 24), (3, 8)])
def test_statistics_table_in_lds_and_in_global_memory(leads, B, lib_built):
    """The 16-byte kernel copies a column-statistics table of at most 8 KB (B * K * 32 bytes) into LDS and reads a
    larger one from global memory: 2816 and 4224 bytes on one side, 8448 bytes on the other, with one lead (state as
    16-byte pairs) and three.  Each equals, bit for bit, the same samples fed one by one (a 352- or 1056-byte table)
    and the element kernel on padded rows."""
    V = _V()
    G, Cn = 96, 11
    K = leads * Cn
    g = torch.Generator(device=DEV).manual_seed(leads * 100 + B)
    wide_t = torch.randn(B, G, K + 3, generator=g, device=DEV) * 3.0 + 50.0
    wide_p = wide_t + 0.5 * torch.randn(B, G, K + 3, generator=g, device=DEV)
    t, p = wide_t[..., :K].contiguous(), wide_p[..., :K].contiguous()
    batch = V.MetricMaps(Cn, G, leads=leads)
    batch.update(t, p)
    singly = V.MetricMaps(Cn, G, leads=leads)
    for b in range(B):
        singly.update(t[b:b + 1], p[b:b + 1])
    padded = V.MetricMaps(Cn, G, leads=leads)
    padded.update(wide_t[..., :K], wide_p[..., :K])
    for other in (singly, padded):
        assert other.n == batch.n == B and _bits(other._state, batch._state)
        assert _bits(other.maps("acc"), batch.maps("acc"))
    # and ACC is the float64 value: both sides sum in float64 (errors near 1e-13), the map is rounded to float32 once
    # (2^-24 relative), so 2^-23 of max(1, |value|) has room
    ph, th = ((x - x.mean(1, keepdim=True)) / (x.std(1, keepdim=True) + 1e-8) for x in (p.double(), t.double()))
    want = (ph * th).mean(0).view(G, leads, Cn).permute(1, 0, 2)
    err = (batch.maps("acc").double() - want).abs()
    assert bool((err <= 2.0 ** -23 * want.abs().clamp(min=1.0)).all()), float(err.max())


@pytest.mark.gpu
def test_selected_sums(Z, lib_built):
    t, p = _dev(Z["all_t"]), _dev(Z["all_p"])
    full = _case(Z)
    full.update(t, p)
    only = _case(Z, stats=("rmse",))
    only.update(t, p)
    assert only._state.shape == (2, 1, 512 * 8) and full._state.shape == (2, 4, 512 * 8)
    assert _bits(only.maps("rmse"), full.maps("rmse"))
    with pytest.raises(ValueError, match="not accumulated"):
        only.maps("acc")
    pair = _case(Z, stats=("acc", "mae"))
    pair.update(t, p)
    assert pair._state.shape[1] == 2
    assert _bits(pair.maps("acc"), full.maps("acc")) and _bits(pair.maps("mae"), full.maps("mae"))


@pytest.mark.gpu
def test_persistence_and_skill(Z, lib_built):
    V = _V()
    t, p = _dev(Z["all_t"]), _dev(Z["all_p"])
    g = torch.Generator().manual_seed(5)
    X = torch.randn(6, 512, 3 * 8, generator=g).to(DEV)  # observation window of 3 steps
    X[..., -8:] += 0.5 * t[..., :8]
    view = _case(Z)
    view.update(t, V.Persistence(X, 8))
    mat = _case(Z)
    mat.update(t, X[..., -8:].repeat(1, 1, 2))
    assert _bits(view._state, mat._state)
    for s in STATS:
        assert _bits(view.maps(s), mat.maps(s)), s
    model = _case(Z)
    model.update(t, p)
    got = model.skill(view).cpu().numpy().astype(np.float64)
    r, rp = model.maps("rmse").cpu().numpy().astype(np.float64), view.maps("rmse").cpu().numpy().astype(np.float64)
    want = 1.0 - r / np.maximum(rp, 1e-9)
    assert np.all(np.abs(got - want) <= _ulp32(want))
    assert got.mean() > 0.3  # the prediction is closer to the truth than the last frame


@pytest.mark.gpu
def test_captured_update_counts_on_the_device(Z, lib_built):
    V = _V()
    t, p = _dev(Z["all_t"]), _dev(Z["all_p"])
    kw = dict(leads=2, var_order=_names(Z), y_mean=Z["y_mean"], y_scale=Z["y_scale"])
    cap, eager = V.CapturedMetricMaps(8, 512, **kw), V.MetricMaps(8, 512, **kw)
    k, B = 6, 2
    for i in range(k):
        b0 = (2 * i) % 6
        cap.update(t[b0:b0 + B], p[b0:b0 + B])
        eager.update(t[b0:b0 + B], p[b0:b0 + B])
    assert cap.graph_active and cap.launch_mode == "hipGraph replay"
    assert cap.n == k * B == eager.n
    assert _bits(cap._state, eager._state)
    for s in STATS:
        assert _bits(cap.maps(s), eager.maps(s)), s
    off = V.CapturedMetricMaps(8, 512, use_graph=False, **kw)
    off.update(t, p)
    assert off.launch_mode == "eager" and off.n == 6


def _series(tmp_path, T, n_lon, n_lat, Cn, seed=3):
    rng = np.random.RandomState(seed)
    mean = rng.randn(Cn).astype(np.float32)
    std = (0.5 + rng.rand(Cn)).astype(np.float32)
    base = rng.randn(1, n_lon, n_lat, Cn)
    data = (mean + std * (base + 0.3 * rng.randn(T, n_lon, n_lat, Cn))).astype(np.float16)
    np.save(tmp_path / "chunk_0.npy", data)
    np.savez(tmp_path / "scalers.npz", mean=mean, std=std, n=T)


@pytest.mark.gpu
@pytest.mark.parametrize("captured", [False, True])
def test_metric_maps_driver(tmp_path, monkeypatch, captured, lib_built):
    from graphcast_lite_amd import predict
    from graphcast_lite_amd.data import TimeseriesChunkDataset
    from graphcast_lite_amd.models import WeatherPrediction

    V = _V()
    cfg = experiment("baseline", [1, 2])
    Cn, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    torch.manual_seed(11)
    lats, lons = np.linspace(-90, 90, 32, endpoint=True), np.linspace(0, 360, 64, endpoint=False)
    model = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, torch.device(DEV))
    _series(tmp_path, 14, 64, 32, Cn)
    ds = TimeseriesChunkDataset(str(tmp_path), obs_window=obs, pred_steps=2, split="all", device=DEV)
    assert len(ds) == 11
    kw = dict(stats=("rmse", "bias", "acc"), y_mean=ds.mean_np, y_scale=ds.std_np)
    static = [Cn - 1]

    # the loop written out
    want, want_p = V.MetricMaps(Cn, 64 * 32, leads=2, **kw), V.MetricMaps(Cn, 64 * 32, leads=2, **kw)
    idx = list(range(len(ds)))
    for s in range(0, len(idx), 2):  # 6 batches: the captured run replays its graphs from the third on
        X, Y = ds.batch(idx[s:s + 2])
        out = predict.rollout(model, X, 2, static_channels=static, use_residual=True)
        want.update(Y, out)
        want_p.update(Y, V.Persistence(X, Cn))

    def refuse(self, *a, **k):
        raise AssertionError("device-to-host copy inside metric_maps")
    with monkeypatch.context() as mp:
        for name in ("cpu", "item", "tolist", "numpy"):
            mp.setattr(torch.Tensor, name, refuse)
        got, got_p = V.metric_maps(model, ds, ar_steps=2, batch_size=2, static_channels=static, persistence=True,
                                   captured=captured, **kw)
    assert isinstance(got, V.CapturedMetricMaps) == captured
    assert got.n == 11 == got_p.n
    assert _bits(got._state, want._state) and _bits(got_p._state, want_p._state)
    for s in kw["stats"]:
        m = got.maps(s)
        assert m.is_cuda and m.shape == (2, 64 * 32, Cn) and _bits(m, want.maps(s))
    assert _bits(got.skill(got_p), want.skill(want_p))
    sub = V.metric_maps(model, ds, indices=[1, 5, 6], ar_steps=1, batch_size=2, captured=False, stats=("mae",))
    assert sub.n == 3 and sub.leads == 1 and torch.isfinite(sub.maps("mae")).all()
