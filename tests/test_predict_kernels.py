"""Contract of `gcl_obs_pack` and `gcl_region_interp_scores` (csrc/predict.hip) as include/gcl.h states it, against
restatements in numpy (tests/helpers/predict_case.py), on padded, strided and offset rows.

`gcl_obs_pack` copies or writes one constant: bit-equal, NaN bits included (the int32 views are compared).

`gcl_region_interp_scores`: the stored fields are single float64 -> float32 roundings of IEEE-exact arithmetic (four
products rounded one by one, three additions, one subtraction and one division), so they equal the restatement bit for
bit.  The sums are compared with their restatement in extended precision at relative 1e-12 and the scores derived from
them at 1e-10; these bounds and their derivation are those stated at the top of test_eval_step_kernels.py: every term is
formed in float64 from float32 / fp16 data (relative error about 1e-16 per term) and a sum of fewer than 10^4 such terms
in any fixed order stays far below 1e-12 (the signed sums about the pivot lose the factor sum |t| / |sum t| to
cancellation, a few hundred at most on these inputs); a score is a few hundred float64 operations on those sums."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import predict_case as pc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -777.25


# ----------------------------------------------------------------------------------------------------------------------
# gcl_obs_pack
# ----------------------------------------------------------------------------------------------------------------------
def _views(B, G, K, ld, off, seed):
    """y and out as [B, G, K] views at column `off` of [B, G + 1, ld] buffers (padded rows, a padded batch stride)."""
    g = torch.Generator().manual_seed(seed)
    ybuf = torch.randn(B, G + 1, ld, generator=g).to(DEV)
    obuf = torch.full((B, G + 1, ld), SENTINEL, device=DEV)
    return ybuf, ybuf[:, :G, off:off + K], obuf, obuf[:, :G, off:off + K]


def _masks(G, C, stations, chans):
    kr, kc = np.zeros(G, bool), np.zeros(C, bool)
    kr[stations], kc[chans] = True, True
    up = lambda m: torch.from_numpy(m.astype(np.uint8)).to(DEV)  # noqa: E731
    return kr, kc, up(kr), up(kc)


# (B, G, P, C): one element; a row of 15 floats (no 16-byte path); whole aligned rows with G across a 64-row block
@pytest.mark.parametrize("B,G,P,C", [(1, 1, 1, 1), (2, 5, 3, 5), (3, 67, 2, 4)])
def test_obs_pack_is_bit_equal_on_every_layout(B, G, P, C, lib_built):
    from graphcast_lite_amd import hip

    K = P * C
    rng = np.random.default_rng(G)
    some = np.unique(rng.integers(0, G, size=max(1, G // 3)))
    station_sets = {"some": some, "none": np.zeros(0, np.int64), "all": np.arange(G)}
    chan_sets = {"some": np.arange(0, C, 2), "all": np.arange(C)}
    n = 0
    for ld, off in ((K, 0), (K + 4, 0), (K + 8, 4), (K + 3, 1), (K + 5, 2)):  # dense, padded, offset, unaligned bases
        for sname, st in station_sets.items():
            for cname, ch in chan_sets.items():
                kr, kc, kr_d, kc_d = _masks(G, C, st, ch)
                ybuf, y, obuf, out = _views(B, G, K, ld, off, 100 * G + n)
                want = pc.obs_pack_ref(y.cpu().numpy(), kr, kc)
                before = ybuf.clone()
                assert hip.obs_pack(y, kr_d, kc_d, out) is out
                got = out.cpu().numpy().view(np.int32)
                assert np.array_equal(got, want), (ld, off, sname, cname)
                assert torch.equal(ybuf, before), "the source is only read"
                pad = obuf.clone()
                pad[:, :G, off:off + K] = SENTINEL
                assert bool((pad == SENTINEL).all()), "nothing outside the [B, G, K] view is written"
                # in place
                assert hip.obs_pack(y, kr_d, kc_d, y) is y
                assert np.array_equal(y.cpu().numpy().view(np.int32), want), ("in place", ld, off, sname, cname)
                n += 1
    # a fresh output when none is given; the 16-byte path and the element path agree on the same values
    kr, kc, kr_d, kc_d = _masks(G, C, some, np.arange(0, C, 2))
    y = torch.randn(B, G, K, generator=torch.Generator().manual_seed(5)).to(DEV)
    assert np.array_equal(hip.obs_pack(y, kr_d, kc_d).cpu().numpy().view(np.int32), pc.obs_pack_ref(y.cpu().numpy(), kr, kc))


def test_obs_pack_refuses_bad_arguments(lib_built):
    from graphcast_lite_amd import hip

    L = hip.lib()
    y = torch.zeros(1, 2, 4, device=DEV)
    m = torch.ones(4, dtype=torch.uint8, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    assert L.gcl_obs_pack(y.data_ptr(), 3, 8, m.data_ptr(), m.data_ptr(), 1, 2, 4, 4, y.data_ptr(), 4, 8, s) != 0
    assert b"leading dimension" in L.gcl_last_error()
    assert L.gcl_obs_pack(None, 4, 8, m.data_ptr(), m.data_ptr(), 1, 2, 4, 4, y.data_ptr(), 4, 8, s) != 0
    with pytest.raises(ValueError):
        hip.obs_pack(y, m[:2].contiguous(), m[:3].contiguous())  # 4 columns are not whole steps of 3 channels


def test_sparse_observations_is_what_the_reference_loop_builds(lib_built):
    """scripts/predict.py:474-483 on the host against `sparse_observations` on the device."""
    from graphcast_lite_amd.observations import sparse_observations

    g = torch.Generator().manual_seed(3)
    G, P, C = 37, 3, 5
    y = torch.randn(2, G, P * C, generator=g)
    stations, chans = [30, 2, 11, 2], [4, 1]
    want = torch.full_like(y, float("nan"))
    want[:, stations] = y[:, stations]
    flat = want.view(2, G, P, C)
    hide = torch.ones(C, dtype=torch.bool)
    hide[chans] = False
    flat[:, :, :, hide] = float("nan")
    got = sparse_observations(y.to(DEV), stations, channels=chans, num_channels=C)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.numpy().view(np.int32))
    one = sparse_observations(y[0].to(DEV), np.asarray(stations))  # [G, K], every channel
    all_ch = torch.full_like(y[0], float("nan"))
    all_ch[stations] = y[0][stations]
    assert np.array_equal(one.cpu().numpy().view(np.int32), all_ch.numpy().view(np.int32))
    with pytest.raises(ValueError):
        sparse_observations(y.to(DEV), [G])


# ----------------------------------------------------------------------------------------------------------------------
# gcl_region_interp_scores
# ----------------------------------------------------------------------------------------------------------------------
def _region_case(one_node: bool, seed=11, wide: bool = False):
    """The 16 x 8 -> 7 x 5 grids of the fixture (descending regional latitudes, regional longitudes past the last global
    one) or a 1-node region; N = 5 with a first sample whose base step would be -1 and an unmatched one in the middle;
    P = 2; C = 3 of n_feat = 4; channel 1 sits 10^4 standard deviations from 0.  wide: C = 19 of n_feat = 20 on 23 x 21
    regional nodes inside the global axes (the three channels' scalers repeated)."""
    from graphcast_lite_amd.verify import regrid_tables

    f = pc.interp_inputs(pc.fixture())
    r_lats, r_lons = (f["r_lats"][2:3], f["r_lons"][6:7]) if one_node else (f["r_lats"], f["r_lons"])
    if wide:
        r_lats = np.linspace(f["g_lats"][-2], f["g_lats"][1], 23)
        r_lons = np.linspace(f["g_lons"][1], f["g_lons"][-2], 21)
    cell, w = regrid_tables(f["g_lats"], f["g_lons"], r_lats, r_lons)
    rng = np.random.default_rng(seed)
    N, P, C, NF, NT, Gg = 5, 2, 19 if wide else 3, 20 if wide else 4, 12, f["nlg"] * f["ntg"]
    nr = cell.shape[0]
    mean, std = np.resize([280.0, -1e4, 1.5], C), np.resize([11.0, 1.0, 4.0], C)
    raw = rng.standard_normal((NT, nr, NF)) * np.append(std, 1.0) + np.append(np.resize([280.0, 0.0, 1.5], C), 7.0)
    series = raw.astype(np.float16)
    pred = rng.standard_normal((N, Gg, P * C)).astype(np.float32)
    pred[:, :, 1::C] += np.float32(1e4)
    t0 = np.asarray([0, 2, -1, 5, 10], np.int32)  # base step -1; matched; skipped; matched; matched (ends at the last step)
    return dict(cell=cell, w=w, series=series, pred=pred, t0=t0, mean=mean, std=std, N=N, P=P, C=C, NF=NF, NT=NT, nr=nr,
                nlat=f["ntg"], Gg=Gg)


def _launch(c, pred3, store: bool):
    from graphcast_lite_amd import hip

    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    sums = torch.full((c["P"], c["C"], hip.REGION_NS), float("nan"), dtype=torch.float64, device=DEV)
    vout = tout = None
    if store:
        vout = torch.full((c["N"], c["P"], c["nr"], c["C"]), SENTINEL, device=DEV)
        tout = torch.full_like(vout, SENTINEL)
    hip.region_interp_scores(pred3, c["nlat"], d(c["cell"]), d(c["w"]), d(c["series"]), d(c["t0"]), 1, d(c["mean"]),
                             d(c["std"]), c["P"], c["C"], sums, vout, tout)
    return sums, vout, tout


@pytest.mark.parametrize("one_node", [False, True])
def test_region_sums_scores_and_fields_match_the_restatement(one_node, lib_built):
    from graphcast_lite_amd.verify import RegionBundleScores

    c = _region_case(one_node)
    v, t, b = pc.region_fields(c["pred"], c["nlat"], c["cell"], c["w"], c["series"], c["t0"], c["mean"], c["std"], c["P"],
                               c["C"])
    want = pc.region_sums(v, t, b, c["t0"], c["NT"])
    # the forecast as a column block of a wider, offset buffer
    buf = torch.full((c["N"], c["Gg"] + 2, c["P"] * c["C"] + 5), 9e9, device=DEV)
    pred3 = buf[:, 1:c["Gg"] + 1, 3:3 + c["P"] * c["C"]]
    pred3.copy_(torch.from_numpy(c["pred"]))
    sums, vout, tout = _launch(c, pred3, store=True)
    got = sums.cpu().numpy()
    assert np.array_equal(got[..., 3], want[..., 3]) and got[0, 0, 3] == 3 * c["nr"]
    assert np.array_equal(got[..., 9:], want[..., 9:]), "the pivots are values of the data"
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[want == 0] = np.abs(got[want == 0])
    print(f"one_node={one_node}: worst relative error of a sum {err.max():.2e} (sum {int(err.argmax()) % 11})")
    assert err.max() <= 1e-12, (err.max(), got, want)
    ok = (c["t0"] >= 1) & (c["t0"] + c["P"] <= c["NT"])
    assert ok.tolist() == [False, True, False, True, True]
    gv, gt = vout.cpu().numpy(), tout.cpu().numpy()
    assert np.array_equal(gv[ok].view(np.int32), v[ok].astype(np.float32).view(np.int32))
    assert np.array_equal(gt[ok].view(np.int32), t[ok].astype(np.float32).view(np.int32))
    assert (gv[~ok] == SENTINEL).all() and (gt[~ok] == SENTINEL).all(), "skipped samples are left as they are"
    n_ok = int(ok.sum())
    a, r = RegionBundleScores(got, n_ok, c["N"], c["nr"]), RegionBundleScores(want, n_ok, c["N"], c["nr"])
    worst = 0.0
    pairs = [(a.overall, r.overall)] + [(a.horizon(p), r.horizon(p)) for p in range(c["P"])]
    pairs += [(a.channel(p, k), r.channel(p, k)) for p in range(c["P"]) for k in range(c["C"])]
    for x, y in pairs:
        for key in ("rmse", "base", "mae", "skill", "acc"):
            e = abs(x[key] - y[key]) / max(1.0, abs(y[key]))
            worst = max(worst, e)
            assert e <= 1e-10, (key, x, y)
    print(f"one_node={one_node}: worst error of a score {worst:.2e}")
    # the ACC of the offset channel survives: a direct float64 evaluation on the centred fields agrees
    if not one_node:
        tt, vv = t[ok][:, 0, :, 1].ravel(), v[ok][:, 0, :, 1].ravel()
        ta, va = tt - tt.mean(), vv - vv.mean()
        direct = float((ta * va).sum() / (np.linalg.norm(ta) * np.linalg.norm(va) + 1e-8))
        assert abs(a.channel(0, 1)["acc"] - direct) <= 1e-10
    # two runs, with and without the stored fields: the same bits
    again, _, _ = _launch(c, pred3, store=False)
    assert torch.equal(again, sums)


def test_region_sums_with_19_channels_and_a_partial_last_chunk(lib_built):
    """C = 19: a block is 13 node lanes x 19 channels (9 threads idle) and a chunk 13 x 32 = 416 nodes; 483 nodes leave a
    last chunk of 67, whose lanes 2 .. 12 hold 5 nodes and lanes 0, 1 hold 6.  Same restatement and same 1e-12 as above:
    a float64 sum of 3 x 483 terms in any order lies within 1449 x 2^-53 = 1.6e-13 of its sum of absolute values, and
    the sums about the pivot are no random walks (their mean term is the column mean minus the pivot)."""
    c = _region_case(False, wide=True)
    assert (c["C"], c["nr"]) == (19, 483) and c["nr"] % ((256 // 19) * 32) != 0
    v, t, b = pc.region_fields(c["pred"], c["nlat"], c["cell"], c["w"], c["series"], c["t0"], c["mean"], c["std"], c["P"],
                               c["C"])
    want = pc.region_sums(v, t, b, c["t0"], c["NT"])
    pred3 = torch.from_numpy(c["pred"]).to(DEV)
    sums, vout, tout = _launch(c, pred3, store=True)
    got = sums.cpu().numpy()
    assert np.array_equal(got[..., 3], want[..., 3]) and got[0, 0, 3] == 3 * c["nr"]
    assert np.array_equal(got[..., 9:], want[..., 9:]), "the pivots are values of the data"
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err[want == 0] = np.abs(got[want == 0])
    print(f"C=19, nr=483: worst relative error of a sum {err.max():.2e} (sum {int(err.argmax()) % 11})")
    assert err.max() <= 1e-12, (err.max(), got, want)
    ok = (c["t0"] >= 1) & (c["t0"] + c["P"] <= c["NT"])
    gv, gt = vout.cpu().numpy(), tout.cpu().numpy()
    assert np.array_equal(gv[ok].view(np.int32), v[ok].astype(np.float32).view(np.int32))
    assert np.array_equal(gt[ok].view(np.int32), t[ok].astype(np.float32).view(np.int32))
    assert (gv[~ok] == SENTINEL).all() and (gt[~ok] == SENTINEL).all(), "skipped samples are left as they are"
    again, _, _ = _launch(c, pred3, store=False)
    assert torch.equal(again, sums)


def test_region_scores_refuse_bad_arguments(lib_built):
    from graphcast_lite_amd import hip

    c = _region_case(True)
    L = hip.lib()
    assert L.gcl_region_interp_scores_ws_bytes(5, 2, 35, 3) > 0
    assert L.gcl_region_interp_scores_ws_bytes(5, 2, 35, 257) == 0
    pred3 = torch.from_numpy(c["pred"]).to(DEV)
    with pytest.raises(ValueError):
        sums = torch.empty(c["P"], c["C"], 10, dtype=torch.float64, device=DEV)
        hip.region_interp_scores(pred3, c["nlat"], torch.zeros(1, 2, dtype=torch.int32, device=DEV),
                                 torch.zeros(1, 4, dtype=torch.float64, device=DEV),
                                 torch.zeros(12, 1, 4, dtype=torch.float16, device=DEV),
                                 torch.zeros(5, dtype=torch.int32, device=DEV), 0,
                                 torch.zeros(3, dtype=torch.float64, device=DEV),
                                 torch.ones(3, dtype=torch.float64, device=DEV), c["P"], c["C"], sums)
