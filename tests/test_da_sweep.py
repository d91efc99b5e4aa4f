"""The DA grid search: per-row nudging and OI kernels, the sweep assimilator, its rollout (eager and captured), the
`DaSweep` driver and its tables - every setting of one batched rollout against that setting run on its own at batch 1
with the single-setting path (`NudgingAssimilator`, `OINetwork`, `assimilated_rollout`, `ForecastVerifier`)."""
import numpy as np
import pytest
import torch


def _A():
    from graphcast_lite_amd import assimilation

    return assimilation


def _grid(nlat=32, nlon=64):
    return np.linspace(-90, 90, nlat, endpoint=True), np.linspace(0, 360, nlon, endpoint=False)


def _roi():
    """The 144-node box of test_network_apply_equals_apply."""
    lats, lons = _grid()
    li, lj = np.where((lats >= 20) & (lats <= 70))[0], np.where((lons >= 30) & (lons <= 120))[0]
    return (lj[:, None] * 32 + li[None, :]).ravel()


def _predict_obs(y, stations, C, channels=None):
    """scripts/predict.py:474-483: NaN except the station rows (and the observed channels)."""
    obs = torch.full_like(y, float("nan"))
    obs[stations] = y[stations]
    if channels is not None:
        of = obs.view(obs.shape[0], -1, C)
        mask = torch.ones(C, dtype=torch.bool)
        mask[channels] = False
        of[:, :, mask] = float("nan")
        obs = of.view(obs.shape)
    return obs


# ======================================================================================================================
# CPU
# ======================================================================================================================
@pytest.mark.parametrize("npool", [294, 2048])
@pytest.mark.parametrize("sparsity", [0.01, 0.1, 0.001])
def test_station_network_is_the_reference_draw(npool, sparsity):
    A = _A()
    pool = np.arange(npool) if npool == 2048 else 5 + 3 * np.arange(npool)
    # scripts/predict.py:397-406 restated
    rng = np.random.RandomState(42)
    n_stations = max(1, int(len(pool) * sparsity))
    want = rng.choice(pool, n_stations, replace=False)
    want.sort()
    got = A.station_network(pool, sparsity, seed=42)
    assert np.array_equal(got, want) and len(got) == n_stations
    assert np.all(np.diff(got) > 0) and np.isin(got, pool).all()
    assert np.array_equal(A.station_network(pool, sparsity), got)  # a fresh generator per call, default seed 42
    if sparsity == 0.001:
        assert len(got) == (1 if npool == 294 else 2)  # int(0.294) = 0: the floor of one station
    if n_stations > 1:
        assert not np.array_equal(A.station_network(pool, sparsity, seed=43), got)


def test_da_grid_reproduces_the_grid_search_driver():
    A = _A()
    grid = A.da_grid()
    # da_grid_search.sh restated: the nudging loops, then the OI loops
    want = []
    for sp, tag in ((0.01, "1"), (0.1, "10")):
        for alpha in ("0.01", "0.05", "0.1", "0.3"):
            want.append(("nudging", sp, f"nudg{tag}_a{alpha}"))
    for sp, tag in ((0.01, "1"), (0.1, "10")):
        for corr in (5000, 10000, 50000):
            for so in ("0.3", "0.5"):
                want.append(("oi", sp, f"oi{tag}_c{corr // 1000}_s{so}"))
    assert [(s.method, s.sparsity, s.label) for s in grid] == want
    assert sum(s.method == "nudging" for s in grid) == 8 and sum(s.method == "oi" for s in grid) == 12
    oi = [s for s in grid if s.method == "oi"]
    assert {s.sigma_b for s in oi} == {0.8} and {s.corr_len for s in oi} == {5000.0, 10000.0, 50000.0}
    assert [s.alpha for s in grid[:4]] == [0.01, 0.05, 0.1, 0.3]
    # parse_da_results.py reads corr_len and sigma back from the label
    for s in oi:
        parts = s.label.split("_")
        assert int(parts[1][1:]) * 1000 == s.corr_len and float(parts[2][1:]) == s.sigma_o
    with_base = A.da_grid(baseline=True)
    assert with_base[0].method == "none" and with_base[0].label == "baseline" and with_base[1:] == grid
    some = A.da_grid(nudging_alphas=(), oi=[(0.1, 100000, 1.0), (0.01, 200000, 0.5)])
    assert [s.label for s in some] == ["oi10_c100_s1", "oi1_c200_s0.5"]
    with pytest.raises(ValueError):
        A.DASetting("oi", label="x")  # no station density
    with pytest.raises(ValueError):
        A.DASetting("kalman", sparsity=0.1)


def test_sweep_row_order():
    A = _A()
    settings = A.da_grid(baseline=True) + [A.DASetting(label="baseline2")]
    settings = [settings[i] for i in np.random.RandomState(0).permutation(len(settings))]
    sw = A.DASweepAssimilator(_grid(), settings, np.arange(2048), 42)  # no GPU work before prepare()
    rows = sw.settings_by_row
    S = len(settings)
    assert sorted(sw.row_of.values()) == list(range(S)) and set(sw.row_of) == {s.label for s in settings}
    assert all(rows[sw.row_of[s.label]] is s for s in settings)
    kinds = [s.method for s in rows]
    assert kinds == ["none"] * 2 + ["nudging"] * 8 + ["oi"] * 12
    oi = rows[10:]
    dens = [s.sparsity for s in oi]
    assert dens[:6] == [dens[0]] * 6 and dens[6:] == [dens[6]] * 6 and dens[0] != dens[6]  # contiguous groups
    for grp in (oi[:6], oi[6:]):
        assert all(a.corr_len <= b.corr_len for a, b in zip(grp, grp[1:]))
    # ties keep the order of `settings`
    pos = {s.label: i for i, s in enumerate(settings)}
    for a, b in zip(oi, oi[1:]):
        if a.sparsity == b.sparsity and a.corr_len == b.corr_len:
            assert pos[a.label] < pos[b.label]
    assert set(sw.networks) == {0.01, 0.1}
    assert np.array_equal(sw.networks[0.1], A.station_network(np.arange(2048), 0.1, 42))
    with pytest.raises(ValueError):
        A.DASweepAssimilator(_grid(), [settings[0], settings[0]], np.arange(2048), 42)


def _hand_verifier(C, ar, rmse6, base6=2.0, rmse12=1.0, n_elem=8.0):
    """A ForecastVerifier whose region +6h / +12h objects hold the given RMSE (state written by hand)."""
    from graphcast_lite_amd.verify import ForecastVerifier

    v = ForecastVerifier(C, ar, region_idxs=[0, 1], device="cpu")

    def fill(o, rmse, acc):
        st = torch.zeros(4 + 4 * C, dtype=torch.float64)
        st[0], st[1], st[2], st[3] = rmse ** 2 * n_elem, rmse * n_elem, 1, n_elem
        st[4:4 + C] = rmse ** 2 * n_elem / C
        st[4 + C:4 + 2 * C] = acc
        st[4 + 2 * C:4 + 3 * C] = n_elem / C
        st[4 + 3 * C:4 + 4 * C] = 1
        o._state.copy_(st)

    for m, r6, r12, acc in (("pred", rmse6, rmse12, 0.5), ("base", base6, 2.0, 0.25)):
        fill(v.overall[m], 3.0 if m == "pred" else 4.0, acc)
        fill(v.region[m], 0.5 * (r6 + r12), acc)
        for objs in (v.horizon[m], v.region_horizon[m]):
            fill(objs[0], r6, acc)
            fill(objs[1], r12, acc)
    return v


def test_da_sweep_tables_on_hand_made_states():
    A = _A()
    from graphcast_lite_amd.pipeline import da_sweep_tables

    S = A.DASetting
    settings = [S(label="baseline"),
                S("nudging", alpha=0.1, sparsity=0.1, label="nudg10_a0.1"),
                S("nudging", alpha=0.3, sparsity=0.1, label="nudg10_a0.3"),
                S("oi", sigma_o=0.5, corr_len=50000.0, sparsity=0.1, label="oi10_c50_s0.5"),
                S("oi", sigma_o=0.3, corr_len=10000.0, sparsity=0.1, label="oi10_c10_s0.3"),
                S("oi", sigma_o=0.5, corr_len=10000.0, sparsity=0.1, label="oi10_c10_s0.5"),
                S("oi", sigma_o=0.5, corr_len=200000.0, sparsity=0.01, label="oi1_c200_s0.5")]
    rmse6 = [1.8, 1.5, 1.0, 0.5, 0.5, 1.0, 1.2]  # the two best OI 10% settings tie; nudging: the second wins
    vs = [_hand_verifier(2, 2, r) for r in rmse6]
    res = da_sweep_tables(vs, settings)
    assert res["settings"] == [s.label for s in settings]
    for s, r in zip(settings, rmse6):
        row = res["per_setting"][s.label]
        want = (1.0 - r / (2.0 + 1e-12)) * 100
        assert row["skill_6h"] == want and row["region_horizon"][0]["skill"] == want
        assert row["region_horizon"][0]["rmse"] == r and row["region_horizon"][0]["base_rmse"] == 2.0
        assert row["region_horizon"][1]["rmse"] == 1.0 and row["region"]["rmse"] == 0.5 * (r + 1.0)
        assert row["global"]["rmse"] == 3.0 and row["global"]["skill"] == (1.0 - 3.0 / (4.0 + 1e-12)) * 100
        assert row["region"]["acc"] == 0.5 and row["region"]["base_acc"] == 0.25
        assert row["region"]["rmse_per_channel"] == [0.5 * (r + 1.0)] * 2
        assert (row["method"], row["sparsity"], row["corr_len"]) == (s.method, s.sparsity, s.corr_len)
    assert res["best"] == {("nudging", "10"): "nudg10_a0.3", ("oi", "10"): "oi10_c50_s0.5",  # the first of the tie
                           ("oi", "1"): "oi1_c200_s0.5"}
    sk = lambda r: (1.0 - r / (2.0 + 1e-12)) * 100  # noqa: E731
    assert res["oi_tables"]["10"] == {"corr_lens_km": [10.0, 50.0], "sigma_os": [0.3, 0.5],
                                      "skill": [[sk(0.5), sk(1.0)], [None, sk(0.5)]]}
    assert res["oi_tables"]["1"] == {"corr_lens_km": [200.0], "sigma_os": [0.5], "skill": [[sk(1.2)]]}
    # without a region the figure is the whole grid's first horizon; with one horizon the overall one
    from graphcast_lite_amd.verify import ForecastVerifier

    v = ForecastVerifier(2, 1, device="cpu")
    v.overall["pred"]._state[0], v.overall["pred"]._state[3] = 4.0, 4.0
    v.overall["base"]._state[0], v.overall["base"]._state[3] = 16.0, 4.0
    one = da_sweep_tables([v], settings[:1])
    assert one["per_setting"]["baseline"]["skill_6h"] == (1.0 - 1.0 / (2.0 + 1e-12)) * 100
    assert "region" not in one["per_setting"]["baseline"] and one["best"] == {} and one["oi_tables"] == {}
    with pytest.raises(ValueError):
        da_sweep_tables(vs[:2], settings)


def test_new_entry_points_are_declared_and_bound():
    import os

    from conftest import ROOT
    from graphcast_lite_amd import hip

    header = open(os.path.join(ROOT, "include", "gcl.h")).read()
    for name in ("gcl_nudge_rows", "gcl_oi_analysis_rows"):
        assert f"int {name}(" in header and name in hip._SIGNATURES
    assert len(hip._SIGNATURES["gcl_nudge_rows"][1]) == 18
    assert len(hip._SIGNATURES["gcl_oi_analysis_rows"][1]) == len(hip._SIGNATURES["gcl_oi_analysis"][1])


# ======================================================================================================================
# GPU
# ======================================================================================================================
G, C = 2048, 33
OI_SETTINGS = [(0.8, 0.5, 800e3), (0.8, 0.3, 800e3), (1.2, 0.5, 800e3), (0.8, 0.5, 2000e3), (0.8, 0.5, 50e3)]


@pytest.fixture(scope="module")
def small_model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import __graft_entry__ as ge
    from graphcast_lite_amd.models import WeatherPrediction

    cfg = ge._small_config()
    torch.manual_seed(42)
    return WeatherPrediction(_grid(), cfg.graph, cfg.pipeline, cfg.data, torch.device("cuda:0"))


@pytest.mark.gpu
def test_nudge_rows_bit_equal(lib_built):
    A = _A()
    from graphcast_lite_amd import hip

    dev = torch.device("cuda:0")
    nets = [A.station_network(np.arange(G), 0.1, 42), A.station_network(np.arange(G), 0.01, 42)]
    alphas, net_of = [0.0, 0.01, 0.3, 0.3, 0.05], [-1, 0, 0, 1, 1]
    chan = torch.arange(C) % 3 != 0
    g = torch.Generator().manual_seed(3)
    f = torch.randn(5, G, C, generator=g)
    truth = torch.randn(1, G, C, generator=g)
    truth[0, nets[0][:3], 1] = float("nan")  # missing observations at stations
    truth[0, nets[1][-2:], :] = float("nan")
    truth[0, nets[0][7], 4:9] = float("nan")
    want = f.clone()
    for b in range(1, 5):
        nud = A.NudgingAssimilator(alphas[b], device=dev, feature_mask_flat=chan)
        obs = _predict_obs(truth[0], nets[net_of[b]], C)
        want[b] = nud.apply_(f[b:b + 1].to(dev), obs.unsqueeze(0).to(dev))[0].cpu()
    assert not torch.equal(want[1:], f[1:]) and not torch.equal(want[2], want[3])
    mask = np.zeros((2, G), dtype=np.uint8)
    mask[0, nets[0]], mask[1, nets[1]] = 1, 1
    args = (torch.from_numpy(mask).to(dev), torch.tensor(net_of, dtype=torch.int32, device=dev),
            torch.tensor(np.array(alphas, dtype=np.float32), device=dev), chan.to(dev, torch.uint8))
    fd, td = f.to(dev), truth.to(dev)
    out = torch.full_like(fd, 7.0)
    hip.nudge_rows(fd, td, out, *args)  # out of place: every value written, the row without a network copied
    assert torch.equal(out.cpu(), want) and torch.equal(fd.cpu(), f)
    hip.nudge_rows(fd, td, fd, *args)  # in place
    assert torch.equal(fd.cpu(), want)
    # the truth given per row, and no channel mask
    fd = f.to(dev)
    hip.nudge_rows(fd, td.expand(5, G, C).contiguous(), fd, *args[:3], None)
    for b in range(1, 5):
        obs = _predict_obs(truth[0], nets[net_of[b]], C)
        ref = A.NudgingAssimilator(alphas[b], device=dev).apply_(f[b:b + 1].to(dev), obs.unsqueeze(0).to(dev))
        assert torch.equal(fd[b], ref[0])
    assert torch.equal(fd[0].cpu(), f[0])


def _oi_sweep(mode, channels, dev, per_setting=False):
    A = _A()
    pool = np.arange(G) if mode == "full" else _roi()
    settings = [A.DASetting("oi", sigma_b=sb, sigma_o=so, corr_len=L, sparsity=0.1, label=f"oi{j}")
                for j, (sb, so, L) in enumerate(OI_SETTINGS)]
    sw = A.DASweepAssimilator(_grid(), settings, pool, 42, channels=channels, roi_idx=None if mode == "full" else pool,
                              device=dev, per_setting=per_setting)
    return sw, settings, pool


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["full", "roi"])
@pytest.mark.parametrize("channels", [None, [0, 3, 10]])
def test_oi_analysis_rows_bit_equal(mode, channels, lib_built):
    """Every row of the per-row analysis against the single-setting OINetwork.apply of that row's setting."""
    A = _A()
    from graphcast_lite_amd import hip

    dev = torch.device("cuda:0")
    sw, settings, pool = _oi_sweep(mode, channels, dev)
    st = sw.networks[0.1]
    assert len(st) == (204 if mode == "full" else 14)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(len(settings), G, C, generator=g)
    truth = x[:1] + torch.randn(1, G, C, generator=g)
    got = sw.apply_(x.to(dev), truth.to(dev)).cpu()
    obs = _predict_obs(truth[0], st, C, channels).to(dev)
    lats, lons = _grid()
    changed = []
    for s in settings:
        r = sw.row_of[s.label]
        oi = A.OptimalInterpolation(lats, lons, s.sigma_b, s.sigma_o, s.corr_len, dev,
                                    roi_idx=None if mode == "full" else pool)
        want = oi.prepare_network(st, channels).apply(x[r].to(dev), obs).cpu()
        assert torch.equal(got[r], want), s
        changed.append((want - x[r]).abs().amax(dim=1))
    outside = np.setdiff1d(np.arange(G), pool)
    assert torch.equal(got[:, outside], x[:, outside])  # rows outside the OI region are untouched
    # rows are ordered by corr_len; the analysis moved every station's own node, for the shortest length too
    assert sw.row_of["oi4"] == 0 and sw.row_of["oi3"] == len(settings) - 1
    assert all(ch[st].min() > 1e-3 for ch in changed)
    if channels is not None:
        rest = [c for c in range(C) if c not in channels]
        assert torch.equal(got[:, :, rest], x[:, :, rest])

    # every row one setting: the per-row kernel against gcl_oi_analysis at that batch size
    net = sw.oi_nets[sw.row_of["oi0"]]
    B, nch = 5, len(channels or range(C))
    ch = torch.tensor(channels or list(range(C)), dtype=torch.int32, device=dev)
    W = torch.randn(B * nch, net.fac.m, generator=g).to(dev)
    xb = torch.randn(B, G, C, generator=g).to(dev)
    o = net.oi
    for n in (B, 3, 1):  # other batch sizes take other block widths
        xn, Wn = xb[:n], W[:n * nch]
        one = hip.oi_analysis(xn, xn.clone(), ch, o._node_row, o._nodes, net.fac.stations, Wn, o._sb2, o._rl2,
                              o._th_cut, o._a_cut)
        tab = lambda v: torch.full((n,), v, dtype=torch.float64).to(dev, torch.float32)  # noqa: E731
        rows = hip.oi_analysis_rows(xn, xn.clone(), ch, o._node_row, o._nodes, net.fac.stations, Wn, tab(o._sb2),
                                    tab(o._rl2), o._th_cut, o._a_cut)
        assert torch.equal(rows, one) and not torch.equal(one, xn)


def _sweep_settings():
    A = _A()
    S = A.DASetting
    (b0, o0, l0), (b1, o1, l1), (b2, o2, l2), (b3, o3, l3), (b4, o4, l4) = OI_SETTINGS
    return [S("oi", sigma_b=b3, sigma_o=o3, corr_len=l3, sparsity=0.1, label="oi10_c2000"),
            S("nudging", alpha=0.3, sparsity=0.1, label="nudg10_a0.3"),
            S("oi", sigma_b=b0, sigma_o=o0, corr_len=l0, sparsity=0.1, label="oi10_c800"),
            S(label="baseline"),
            S("oi", sigma_b=b2, sigma_o=o2, corr_len=l2, sparsity=0.01, label="oi1_c800_b1.2"),
            S("oi", sigma_b=b4, sigma_o=o4, corr_len=l4, sparsity=0.1, label="oi10_c50"),
            S("nudging", alpha=0.05, sparsity=0.01, label="nudg1_a0.05"),
            S("oi", sigma_b=b1, sigma_o=o1, corr_len=l1, sparsity=0.01, label="oi1_c800_s0.3")]


def _own_assimilator(s, dev, channels, pool, roi):
    """The single-setting assimilator of the parent path and the station network of setting s."""
    A = _A()
    st = A.station_network(pool, s.sparsity, 42)
    if s.method == "nudging":
        return A.NudgingAssimilator(alpha=s.alpha, device=dev), st
    lats, lons = _grid()
    oi = A.OptimalInterpolation(lats, lons, s.sigma_b, s.sigma_o, s.corr_len, dev, roi_idx=roi)
    return oi.prepare_network(st, channels), st


def _rollout_inputs(p, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, G, 2 * C, generator=g), torch.randn(1, G, p * C, generator=g)


@pytest.mark.gpu
@pytest.mark.parametrize("residual", [False, True])
def test_sweep_rollout_rows_equal_single_setting_rollouts(small_model, residual, lib_built):
    A = _A()
    from graphcast_lite_amd.predict import rollout

    dev = torch.device("cuda:0")
    settings, p = _sweep_settings(), 3
    S = len(settings)
    channels = [0, 3, 10] if residual else None
    kw = dict(use_residual=True, static_channels=[2]) if residual else dict(use_residual=False)
    X, truth = _rollout_inputs(p, 4)
    Xd, td = X.to(dev), truth.to(dev)
    pool = np.arange(G)
    sw = A.DASweepAssimilator(_grid(), settings, pool, 42, channels=channels, device=dev)
    got = A.assimilated_rollout(small_model, Xd.expand(S, -1, -1), p, td, sw, **kw)
    assert got.shape == (S, G, p * C)
    for s in settings:
        row = got[sw.row_of[s.label]]
        if s.method == "none":
            assert torch.equal(row, rollout(small_model, Xd, p, **kw)[0])
            continue
        asm, st = _own_assimilator(s, dev, channels, pool, None)
        obs = _predict_obs(truth[0], st, C, channels).unsqueeze(0).to(dev)
        want = A.assimilated_rollout(small_model, Xd, p, obs, asm, **kw)[0]
        assert torch.equal(row, want), s.label
    assert len({got[r].cpu().numpy().tobytes() for r in range(S)}) == S  # the settings do differ
    # the truth given per row; the per-setting fallback
    again = A.assimilated_rollout(small_model, Xd.expand(S, -1, -1), p, td.expand(S, -1, -1).contiguous(), sw, **kw)
    assert torch.equal(again, got)
    ps = A.DASweepAssimilator(_grid(), settings, pool, 42, channels=channels, device=dev, per_setting=True)
    assert torch.equal(A.assimilated_rollout(small_model, Xd.expand(S, -1, -1), p, td, ps, **kw), got)
    # existing callers: observations of batch 1 are still refused for a plain assimilator
    with pytest.raises(ValueError):
        A.assimilated_rollout(small_model, Xd.expand(2, -1, -1), p, td, A.NudgingAssimilator(0.3, device=dev), **kw)


@pytest.mark.gpu
def test_captured_sweep_rollout(small_model, lib_built):
    A = _A()
    dev = torch.device("cuda:0")
    settings, p = _sweep_settings(), 3
    S = len(settings)
    sw = A.DASweepAssimilator(_grid(), settings, np.arange(G), 42, channels=[0, 3, 10], device=dev)
    cap = A.CapturedAssimilatedRollout(small_model, p, sw, use_residual=True, static_channels=[2])
    outs = []
    for seed in range(4):
        X, truth = _rollout_inputs(p, seed + 20)
        XS, td = X.to(dev).expand(S, -1, -1), truth.to(dev)
        eager = A.assimilated_rollout(small_model, XS, p, td, sw, use_residual=True, static_channels=[2])
        outs.append((cap(XS, td), eager))
    assert cap._graph is not None and cap.enabled
    for got, want in outs:
        assert torch.equal(got, want)
    assert not torch.equal(outs[2][0], outs[3][0])


class _SyntheticDS:
    """A `batch(indices) -> (X, Y)` data set of random windows on the device."""

    def __init__(self, n, p, dev):
        g = torch.Generator().manual_seed(11)
        self.device, self.coordinates, self.flat_grid = dev, _grid(), False
        self.X = torch.randn(n, G, 2 * C, generator=g).to(dev)
        self.Y = (self.X[:, :, C:].repeat(1, 1, p) + 0.3 * torch.randn(n, G, p * C, generator=g).to(dev)).contiguous()

    def __len__(self):
        return self.X.shape[0]

    def batch(self, indices):
        idx = torch.tensor([int(i) for i in indices], device=self.device)
        return self.X[idx], self.Y[idx]


@pytest.mark.gpu
def test_da_sweep_equals_separate_verifiers(small_model, lib_built):
    A = _A()
    from graphcast_lite_amd.pipeline import DaSweep, da_sweep_tables
    from graphcast_lite_amd.predict import rollout
    from graphcast_lite_amd.verify import ForecastVerifier, Persistence

    dev = torch.device("cuda:0")
    p, roi = 2, _roi()
    ds = _SyntheticDS(3, p, dev)
    S = A.DASetting
    settings = [S("oi", sigma_o=0.5, corr_len=800e3, sparsity=0.1, label="oi10_c800_s0.5"),
                S(label="baseline"),
                S("nudging", alpha=0.3, sparsity=0.1, label="nudg10_a0.3"),
                S("nudging", alpha=0.05, sparsity=0.1, label="nudg10_a0.05"),
                S("oi", sigma_o=0.3, corr_len=300e3, sparsity=0.1, label="oi10_c300_s0.3")]
    sweep = DaSweep(small_model, ds, settings, p, roi, region_idxs=roi, exclude_channels=[2], static_channels=[2])
    sweep.update([0, 1])
    sweep.update([2])
    assert sweep.graph_active  # two eager calls, then the capture
    res = sweep.results()
    # the parent's way: one run per setting at batch 1, one verifier each
    refs = []
    for s in settings:
        v = ForecastVerifier(C, p, exclude_channels=[2], region_idxs=roi)
        for i in range(3):
            X, Y = ds.batch([i])
            if s.method == "none":
                out = rollout(small_model, X, p, use_residual=False, static_channels=[2])
            else:
                asm, st = _own_assimilator(s, dev, None, roi, roi)
                obs = _predict_obs(Y[0].cpu(), st, C).unsqueeze(0).to(dev)
                out = A.assimilated_rollout(small_model, X, p, obs, asm, use_residual=False, static_channels=[2])
            v.update(Y[0], pred=out[0], base=Persistence(X[0], C))
        refs.append(v)
    want = da_sweep_tables(refs, settings)
    assert res.pop("n") == 3
    assert res == want
    v0 = refs[0]
    row = res["per_setting"]["oi10_c800_s0.5"]
    assert row["region_horizon"][0]["rmse"] == v0.region_horizon["pred"][0].rmse
    assert row["region"]["acc"] == v0.region["pred"].acc and row["global"]["base_rmse"] == v0.overall["base"].rmse
    skill6 = {s.label: 1.0 - v.region_horizon["pred"][0].rmse / (v.region_horizon["base"][0].rmse + 1e-12)
              for s, v in zip(settings, refs)}
    for method in ("nudging", "oi"):
        mine = [s.label for s in settings if s.method == method]
        assert res["best"][(method, "10")] == max(mine, key=lambda n: skill6[n])
    assert skill6["nudg10_a0.3"] > skill6["baseline"]  # assimilating the truth helps
