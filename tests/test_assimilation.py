"""Data assimilation (graphcast_lite_amd.assimilation, csrc/assim.hip) against fixtures produced by running the
reference's `src/assimilation/` (tests/golden/make_assim_golden.py), against torch CPU restatements of its arithmetic,
and against a float64 matrix-free restatement where the reference cannot run."""
import os
import time
import tracemalloc

import numpy as np
import pytest
import torch

from conftest import GOLDEN

R_EARTH = 6371000.0


@pytest.fixture(scope="module")
def gv():
    return dict(np.load(os.path.join(GOLDEN, "assim_vectors.npz")))


def _A():
    from graphcast_lite_amd import assimilation

    return assimilation


def _oi_restated(oi, xb: np.ndarray, y: np.ndarray, nodes=None) -> np.ndarray:
    """float64 matrix-free OI: S = sb2 K(J, J) + (so2 + 1e-5) I, W = S^-1 (y - x_b[J]), x_a = x_b + sb2 K(i, J) W, per
    channel with its own station set; only OI rows change.  `nodes`: OI positions to evaluate (None: all)."""
    A = _A()
    coords = oi._oi_coords
    rows = oi._rows
    xa = xb.astype(np.float64).copy()
    nodes = np.arange(len(rows)) if nodes is None else np.asarray(nodes)
    sb2, diag = oi.sigma_b ** 2, oi.sigma_o ** 2 + 1e-5
    for c in range(xb.shape[1]):
        pos = np.nonzero(~np.isnan(y[rows, c]))[0]
        if len(pos) == 0:
            continue
        J = oi._canon[pos]
        S = sb2 * np.exp(-(A._haversine_m(coords[J], coords[J]) ** 2) / oi.L ** 2) + diag * np.eye(len(J))
        w = np.linalg.solve(S, y[rows[pos], c].astype(np.float64) - xb[rows[J], c].astype(np.float64))
        K = sb2 * np.exp(-(A._haversine_m(coords[nodes], coords[J]) ** 2) / oi.L ** 2)
        xa[rows[nodes], c] = xb[rows[nodes], c] + K @ w
    return xa


def _fp64_rule(x_hip, x32, x64, tag):
    """tests/parity.py's arbitration: the HIP result may be at most twice as far from float64 as the reference's own
    float32 result, plus 1e-5 of the float64 magnitude (in norm and in max-abs)."""
    x_hip, x32, x64 = (np.asarray(v, dtype=np.float64) for v in (x_hip, x32, x64))
    dh, d32 = x_hip - x64, x32 - x64
    assert np.linalg.norm(dh) <= 2 * np.linalg.norm(d32) + 1e-5 * np.linalg.norm(x64), \
        (tag, np.linalg.norm(dh), np.linalg.norm(d32), np.linalg.norm(x64))
    assert np.abs(dh).max() <= 2 * np.abs(d32).max() + 1e-5 * np.abs(x64).max(), \
        (tag, np.abs(dh).max(), np.abs(d32).max())


def _grid(nlat, nlon):
    return np.linspace(-90, 90, nlat, endpoint=True), np.linspace(0, 360, nlon, endpoint=False)


# ======================================================================================================================
# CPU
# ======================================================================================================================
def test_host_helpers_match_reference(gv):
    A = _A()
    feats = ["t2m", "u10", "v10", "msl", "tp"]
    assert np.array_equal(A.build_feature_mask(feats, ["u10", "tp", "nope"], 3, "cpu").numpy(), gv["helper_feature_mask"])
    assert np.array_equal(A.build_feature_mask_from_indices([0, 3, 7, -1], 5, 2, "cpu").numpy(),
                          gv["helper_feature_mask_idx"])
    assert np.array_equal(A.cosine_taper_2d(12, 9, 3).numpy(), gv["helper_taper"])
    assert np.array_equal(A.cosine_taper_2d(4, 5, 0).numpy(), gv["helper_taper_b0"])
    assert np.array_equal(A.build_boundary_taper_mask(9, 12, 2, 3).numpy(), gv["helper_boundary"])


def test_nearest_node_tie_rule_matches_reference(gv):
    A = _A()
    oi = A.OptimalInterpolation(gv["oidup_lat"], gv["oidup_lon"], 0.8, 0.5, float(gv["oidup_L"]), "cpu",
                                flat_grid=True)
    assert np.array_equal(oi._canon, gv["oidup_nearest"])
    assert not np.array_equal(oi._canon, np.arange(len(oi._canon)))  # the fixture does contain duplicates


def test_roi_node_order_is_latitude_major(gv):
    A = _A()
    lats, lons = _grid(256, 512)
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 150e3, "cpu", roi_idx=gv["oiroi_roi"])
    g = gv["oiroi_roi"]
    assert np.array_equal(oi._oi_coords[:, 0], lats[g // 512]) and np.array_equal(oi._oi_coords[:, 1], lons[g % 512])


def test_matrix_free_restatement_matches_reference_fp64(gv):
    """The algebra the HIP path implements (nearest-node canonicalisation, ROI semantics, S from coordinates) equals the
    reference's dense float64 arithmetic."""
    A = _A()
    for tag in ("oifull", "oidup"):
        if tag == "oifull":
            oi = A.OptimalInterpolation(gv["oifull_lats"], gv["oifull_lons"], 0.8, 0.5, float(gv["oifull_L"]), "cpu")
        else:
            oi = A.OptimalInterpolation(gv["oidup_lat"], gv["oidup_lon"], 0.8, 0.5, float(gv["oidup_L"]), "cpu",
                                        flat_grid=True)
        x = _oi_restated(oi, gv[f"{tag}_xb"], gv[f"{tag}_y"])
        np.testing.assert_allclose(x, gv[f"{tag}_x64"], rtol=1e-9, atol=1e-9)


def test_construction_on_full_512x256_builds_no_B():
    A = _A()
    lats, lons = _grid(256, 512)
    tracemalloc.start()
    t0 = time.time()
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 150e3, "cpu")
    dt = time.time() - t0
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    assert oi._B is None
    assert dt < 20.0, dt
    assert peak < 256 * 2 ** 20, peak  # a dense B would be 68 GB (float32)


def test_lazy_B_has_reference_values(gv):
    A = _A()
    oi = A.OptimalInterpolation(gv["oidup_lat"], gv["oidup_lon"], 0.8, 0.5, 300e3, "cpu", flat_grid=True)
    d = A._haversine_m(oi._oi_coords, oi._oi_coords)
    B = oi.B
    assert B.dtype == torch.float32 and B.shape == (40, 40)
    assert torch.equal(B, torch.from_numpy(0.64 * np.exp(-(d ** 2) / 300e3 ** 2)).float())


def test_station_limit_is_a_value_error(lib_built):
    A = _A()
    from graphcast_lite_amd import hip

    lim = hip.oi_max_stations()
    assert lim >= 8192
    lats, lons = _grid(256, 512)
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 150e3, "cpu")
    with pytest.raises(ValueError, match=str(lim)):
        oi.prepare_network(np.arange(lim + 1))


# ======================================================================================================================
# GPU
# ======================================================================================================================
def _torch_nudge_seq(f, o, alpha, mask_flat=None):
    """nudging.py:74-94 in torch CPU."""
    if f.shape != o.shape:
        return f
    mask = ~torch.isnan(o)
    if mask_flat is not None and mask_flat.shape[0] == f.shape[-1]:
        mask = mask & mask_flat.unsqueeze(0)
    a = f.clone()
    if mask.any():
        a[mask] = f[mask] + alpha * (o[mask] - f[mask])
    return a


def _torch_nudge_off(f, o, alpha):
    mask = ~torch.isnan(o)
    a = f.clone()
    if mask.any():
        a[mask] = (1 - alpha) * f[mask] + alpha * o[mask]
    return a


def _bits(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.gpu
def test_nudging_bit_exact(gv, lib_built):
    A = _A()
    f, o, m = torch.from_numpy(gv["nudge_f"]), torch.from_numpy(gv["nudge_o"]), torch.from_numpy(gv["nudge_mask"])
    dev = torch.device("cuda:0")
    na = A.NudgingAssimilator(alpha=0.3, device=dev, feature_mask_flat=m)
    r = na.apply(f[0].to(dev), o[0].to(dev))
    assert r.is_cuda and _bits(r, gv["nudge_seq_masked"])
    assert _bits(A.NudgingAssimilator(alpha=0.3, device=dev).apply(f[1], o[1]), gv["nudge_seq"])  # CPU in, CPU out
    assert _bits(A.NudgingAssimilator(alpha=0.3, device=dev, feature_mask_flat=m[:5]).apply(f[0].to(dev), o[0].to(dev)),
                 gv["nudge_seq_badmask"])
    fm = f[0].to(dev)
    assert A.NudgingAssimilator(alpha=0.3).apply(fm, o[0, :, :5].to(dev)) is fm  # shape mismatch: the forecast itself
    assert _bits(A.nudge_sequence_offline(f.to(dev), o.to(dev), alpha=0.37), gv["nudge_offline"])
    # against torch CPU on a larger batch, awkward alphas
    g = torch.Generator().manual_seed(3)
    f = torch.randn(3, 1000, 13, generator=g) * 50
    o = f + torch.randn(3, 1000, 13, generator=g)
    o[torch.rand(3, 1000, 13, generator=g) < 0.5] = float("nan")
    for alpha in (0.1, 0.25, 1 / 3, 0.7777):
        assert _bits(A.NudgingAssimilator(alpha=alpha).apply(f.to(dev), o.to(dev)), _torch_nudge_seq(f, o, alpha))
        assert _bits(A.nudge_sequence_offline(f.to(dev), o.to(dev), alpha=alpha), _torch_nudge_off(f, o, alpha))


def _oi_case(gv, tag, dev):
    A = _A()
    if tag == "oifull":
        oi = A.OptimalInterpolation(gv["oifull_lats"], gv["oifull_lons"], 0.8, 0.5, float(gv["oifull_L"]), dev)
        return oi, gv["oifull_xb"], gv["oifull_y"], gv["oifull_x32"], gv["oifull_x64"], np.arange(len(gv["oifull_xb"]))
    if tag == "oidup":
        oi = A.OptimalInterpolation(gv["oidup_lat"], gv["oidup_lon"], 0.8, 0.5, float(gv["oidup_L"]), dev,
                                    flat_grid=True)
        return oi, gv["oidup_xb"], gv["oidup_y"], gv["oidup_x32"], gv["oidup_x64"], np.arange(len(gv["oidup_xb"]))
    lats, lons = _grid(256, 512)
    roi = gv["oiroi_roi"]
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, float(gv["oiroi_L"]), dev, roi_idx=roi)
    G, C = 256 * 512, gv["oiroi_xb"].shape[1]
    xb = np.full((G, C), gv["oiroi_fill"], dtype=np.float32)
    y = np.full((G, C), np.nan, dtype=np.float32)
    xb[roi], y[roi] = gv["oiroi_xb"], gv["oiroi_y"]
    x32, x64 = xb.copy(), xb.astype(np.float64)
    x32[roi], x64[roi] = gv["oiroi_x32"], gv["oiroi_x64"]
    return oi, xb, y, x32, x64, roi


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["oifull", "oiroi", "oidup"])
def test_oi_apply_matches_reference(gv, tag, lib_built):
    dev = torch.device("cuda:0")
    oi, xb, y, x32, x64, rows = _oi_case(gv, tag, dev)
    out = oi.apply(torch.from_numpy(xb).to(dev), torch.from_numpy(y).to(dev))
    assert out.is_cuda and out.shape == xb.shape
    xh = out.cpu().numpy()
    observed = ~np.isnan(y[rows]).all(axis=0)
    assert observed.any() and (tag == "oidup" or not observed.all())
    _fp64_rule(xh[rows][:, observed], x32[rows][:, observed], x64[rows][:, observed], tag)
    # non-OI rows and channels without observations: bit-identical to the input
    other = np.setdiff1d(np.arange(len(xb)), rows)
    assert np.array_equal(xh[other].view(np.int32), xb[other].view(np.int32))
    assert np.array_equal(xh[:, ~observed].view(np.int32), xb[:, ~observed].view(np.int32))
    # CPU tensors in -> CPU result
    out_cpu = oi.apply(torch.from_numpy(xb), torch.from_numpy(y))
    assert out_cpu.device.type == "cpu" and _bits(out_cpu, out)


@pytest.mark.gpu
def test_oi_size_check(gv, lib_built):
    oi, xb, y, *_ = _oi_case(gv, "oidup", torch.device("cuda:0"))
    with pytest.raises(RuntimeError):
        oi.apply(torch.zeros(len(xb) + 1, 3, device="cuda:0"), torch.zeros(len(xb) + 1, 3, device="cuda:0"))


@pytest.mark.gpu
def test_oi_full_512x256_one_percent(lib_built):
    """Full-grid OI on 131072 nodes (the reference would need a 68 GB B): against the float64 restatement at a seeded
    sample of nodes, within a memory bound far below a dense B."""
    A = _A()
    dev = torch.device("cuda:0")
    lats, lons = _grid(256, 512)
    G, C = 256 * 512, 3
    rng = np.random.RandomState(5)
    st = np.sort(rng.choice(G, G // 100, replace=False))
    xb = rng.randn(G, C).astype(np.float32)
    y = np.full((G, C), np.nan, dtype=np.float32)
    y[st] = xb[st] + rng.randn(len(st), C).astype(np.float32)
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 150e3, dev)
    xbt, yt = torch.from_numpy(xb).to(dev), torch.from_numpy(y).to(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = oi.apply(xbt, yt)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 256 * 2 ** 20, extra  # a dense float32 B: 68.7e9 bytes
    nodes = np.unique(np.concatenate([rng.choice(G, 3000, replace=False), st[:200]]))
    ref = _oi_restated(oi, xb, y, nodes)[nodes]
    got = out.cpu().numpy()[nodes].astype(np.float64)
    inc = ref - xb[nodes]
    assert np.abs(inc).max() > 0.1  # the analysis does change the sampled nodes
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), np.abs(got - ref).max()


@pytest.mark.gpu
def test_factor_cache(gv, lib_built):
    dev = torch.device("cuda:0")
    oi, xb, y, *_ = _oi_case(gv, "oifull", dev)
    xbt, yt = torch.from_numpy(xb).to(dev), torch.from_numpy(y).to(dev)
    a = oi.apply(xbt, yt)
    n1 = oi.factorizations
    assert n1 == 2  # channels 0 and 1 share a station set, channel 2 has its own, channel 3 none
    b = oi.apply(xbt, yt)
    assert oi.factorizations == n1 and _bits(a, b)
    y2 = y.copy()
    y2[np.nonzero(~np.isnan(y2[:, 2]))[0][0], 2] = np.nan
    oi.apply(xbt, torch.from_numpy(y2).to(dev))
    assert oi.factorizations == n1 + 1


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


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["full", "roi"])
def test_network_apply_equals_apply(gv, mode, lib_built):
    A = _A()
    dev = torch.device("cuda:0")
    lats, lons = _grid(32, 64)
    G, C = 2048, 6
    roi = None
    pool = np.arange(G)
    if mode == "roi":
        li, lj = np.where((lats >= 20) & (lats <= 70))[0], np.where((lons >= 30) & (lons <= 120))[0]
        roi = (lj[:, None] * 32 + li[None, :]).ravel()
        pool = roi
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 800e3, dev, roi_idx=roi)
    st = np.sort(np.random.RandomState(42).choice(pool, max(1, len(pool) // 10), replace=False))
    g = torch.Generator().manual_seed(9)
    for chans in (None, [0, 2, 5]):
        net = oi.prepare_network(st, channels=chans)
        xs = torch.randn(3, G, C, generator=g)
        ys = xs + torch.randn(3, G, C, generator=g)
        obs = torch.stack([_predict_obs(ys[b], st, C, chans) for b in range(3)])
        per = [oi.apply(xs[b].to(dev), obs[b].to(dev)) for b in range(3)]
        for b in range(3):
            assert _bits(net.apply(xs[b].to(dev), obs[b].to(dev)), per[b])
        assert _bits(net.apply(xs.to(dev), obs.to(dev)), torch.stack(per))
        inp = xs.to(dev)
        net.apply(inp, obs.to(dev), out=inp)  # in place
        assert _bits(inp, torch.stack(per))


def _small_model(dev):
    import __graft_entry__ as ge
    from graphcast_lite_amd.models import WeatherPrediction

    cfg = ge._small_config()
    torch.manual_seed(42)
    lats, lons = _grid(32, 64)
    return WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, dev)


class _Wrap(torch.nn.Module):
    """A model of another output width built on the HIP model: 'multi' = P*C channels, 'odd' = 5 channels."""

    def __init__(self, m, kind, P=2):
        super().__init__()
        self.m, self.kind, self.P = m, kind, P
        self.obs_window = m.obs_window

    def forward(self, X, attention_threshold=0.0):
        out = self.m(X, attention_threshold=attention_threshold)
        if self.kind == "multi":
            return torch.cat([out * (1 + 0.5 * p) for p in range(self.P)], dim=-1)
        return out[..., :5]


def _restated_nudged_loop(model, X4, y_obs, p, alpha, k):
    """nudging.py:124-194 restated over the same model, with torch CPU nudging."""
    N, G, T, C = X4.shape
    dev = X4.device
    out = model(X4.reshape(N, G, -1), attention_threshold=0.0).cpu()
    if out.shape[-1] == y_obs.shape[-1]:
        return torch.stack([_torch_nudge_seq(out[i], y_obs[i], alpha) for i in range(N)])
    if out.shape[-1] != C:
        return out
    yo = y_obs.view(N, G, p, C)
    state, preds = X4, []
    for s in range(p):
        if s > 0:
            state = torch.cat([state[:, :, 1:], out.to(dev).unsqueeze(2)], dim=2)
            out = model(state.reshape(N, G, -1), attention_threshold=0.0).cpu()
        if k is None or s < k:
            out = torch.stack([_torch_nudge_seq(out[i], yo[i, :, s], alpha) for i in range(N)])
        preds.append(out)
    return torch.stack(preds, dim=2).view(N, G, -1)


@pytest.fixture(scope="module")
def small_model():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return _small_model(torch.device("cuda:0"))


def _rollout_data(N, G, C, p, seed=4):
    g = torch.Generator().manual_seed(seed)
    X4 = torch.randn(N, G, 2, C, generator=g)
    truth = torch.randn(N, G, p * C, generator=g)
    obs = torch.full_like(truth, float("nan"))
    st = np.sort(np.random.RandomState(42).choice(G, G // 10, replace=False))
    obs[:, st] = truth[:, st]
    return X4, obs, st


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k", [("one", None), ("one", 2), ("one", 0), ("multi", None), ("odd", None)])
def test_sequential_nudged_rollout(small_model, kind, k, lib_built):
    A = _A()
    dev = torch.device("cuda:0")
    model = small_model if kind == "one" else _Wrap(small_model, kind)
    N, G, C, p = 2, 2048, 33, 3 if kind == "one" else 2
    X4, obs, _ = _rollout_data(N, G, C, p)
    got = A.sequential_nudged_rollout(model, X4.to(dev), obs, p, alpha=0.3, k=k, device=dev)
    ref = _restated_nudged_loop(model, X4.to(dev), obs, p, 0.3, k)
    assert got.device.type == "cpu" and _bits(got, ref)


def _restated_oi_loop(model, X4, obs, p, oi):
    """scripts/predict.py:499-510 restated: raw model output, OI per step, window shift."""
    N, G, T, C = X4.shape
    state, outs = X4, []
    for s in range(p):
        o = model(state.reshape(N, G, -1), attention_threshold=0.0)
        o = torch.stack([oi.apply(o[i], obs[i, :, s * C:(s + 1) * C]) for i in range(N)])
        outs.append(o)
        state = torch.cat([state[:, :, 1:], o.unsqueeze(2)], dim=2)
    return torch.cat(outs, dim=-1)


@pytest.mark.gpu
def test_assimilated_rollout_reduces_to_reference_loops(small_model, lib_built):
    A = _A()
    dev = torch.device("cuda:0")
    N, G, C, p = 3, 2048, 33, 3
    X4, obs, st = _rollout_data(N, G, C, p)
    X, obs_d = X4.reshape(N, G, -1).to(dev), obs.to(dev)
    # nudging
    nud = A.NudgingAssimilator(alpha=0.3, device=dev)
    for k in (None, 2):
        got = A.assimilated_rollout(small_model, X, p, obs_d, nud, k=k, use_residual=False)
        ref = _restated_nudged_loop(small_model, X4.to(dev), obs, p, 0.3, k)
        assert _bits(got, ref)
        singles = torch.cat([A.assimilated_rollout(small_model, X[b:b + 1], p, obs_d[b:b + 1], nud, k=k,
                                                   use_residual=False) for b in range(N)])
        assert _bits(got, singles)
    # OI on a fixed network
    lats, lons = _grid(32, 64)
    oi = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 800e3, dev)
    net = oi.prepare_network(st)
    got = A.assimilated_rollout(small_model, X, p, obs_d, net, use_residual=False)
    ref = _restated_oi_loop(small_model, X4.to(dev), obs_d, p, oi)
    assert _bits(got, ref)
    singles = torch.cat([A.assimilated_rollout(small_model, X[b:b + 1], p, obs_d[b:b + 1], net, use_residual=False)
                         for b in range(N)])
    assert _bits(got, singles)


@pytest.mark.gpu
def test_assimilated_rollout_with_residual_static_forcing(small_model, lib_built):
    """With the residual, static and forcing channels: each step is `predict.rollout`'s step, then assimilated."""
    A = _A()
    from graphcast_lite_amd.predict import rollout

    dev = torch.device("cuda:0")
    N, G, C, p = 2, 2048, 33, 3
    X4, obs, st = _rollout_data(N, G, C, p)
    X, obs_d = X4.reshape(N, G, -1).to(dev), obs.to(dev)
    y = torch.randn(N, G, p * C, generator=torch.Generator().manual_seed(8)).to(dev)
    nan_obs = torch.full_like(obs_d, float("nan"))
    nud = A.NudgingAssimilator(alpha=0.3, device=dev)
    kw = dict(static_channels=[1, 4], forcing_channels=[7], y=y)
    # no observations: exactly predict.rollout
    assert _bits(A.assimilated_rollout(small_model, X, p, nan_obs, nud, **kw), rollout(small_model, X, p, **kw))
    # the first step is rollout's first step, nudged
    one = rollout(small_model, X, 1, **kw)
    got = A.assimilated_rollout(small_model, X, p, obs_d, nud, **kw)
    want0 = torch.stack([_torch_nudge_seq(one[b].cpu(), obs[b, :, :C], 0.3) for b in range(N)])
    assert _bits(got[..., :C], want0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["nudging", "oi"])
def test_captured_assimilated_rollout(small_model, which, lib_built):
    A = _A()
    dev = torch.device("cuda:0")
    N, G, C, p = 2, 2048, 33, 3
    X4, obs, st = _rollout_data(N, G, C, p)
    if which == "nudging":
        asm = A.NudgingAssimilator(alpha=0.3, device=dev, feature_mask_flat=torch.arange(C) % 3 != 0)
    else:
        lats, lons = _grid(32, 64)
        asm = A.OptimalInterpolation(lats, lons, 0.8, 0.5, 800e3, dev).prepare_network(st, channels=[0, 3, 10])
    cap = A.CapturedAssimilatedRollout(small_model, p, asm, use_residual=True, static_channels=[2])
    outs = []
    for seed in range(4):
        X4, obs, _ = _rollout_data(N, G, C, p, seed=seed + 20)
        X, obs_d = X4.reshape(N, G, -1).to(dev), obs.to(dev)
        eager = A.assimilated_rollout(small_model, X, p, obs_d, asm, use_residual=True, static_channels=[2])
        outs.append((cap(X, obs_d), eager))
    assert cap._graph is not None and cap.enabled
    for got, want in outs:
        assert _bits(got, want)
