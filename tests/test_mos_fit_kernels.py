"""Contracts of the fitting kernels (csrc/mos_fit.hip) against the numpy restatement tests/helpers/hgb_ref.py, which
tests/test_mos_fit.py checks against sklearn.  Shapes are the smallest at which each kernel can go wrong: segments
around the wave size, more than one partition block (1 024 rows) and more than one histogram row range (256 rows)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import hgb_ref  # noqa: E402

from graphcast_lite_amd import hip  # noqa: E402

pytestmark = pytest.mark.gpu
SEGMENTS = [1, 63, 64, 65, 1000, 2500]  # 2 500: three partition blocks, ten histogram ranges
DEV = "cuda"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ws_for(n, n_val=0, F=32, leaves=31):
    need = int(hip.lib().gcl_mos_fit_ws_bytes(n, n_val, F, leaves, 1))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=DEV), need


def thr_table(thresholds):
    thr = np.zeros((len(thresholds), 256))
    for f, t in enumerate(thresholds):
        thr[f, :len(t)] = t
    return dev(thr), dev(np.array([len(t) for t in thresholds], dtype=np.int32))


def device_bins(X, thresholds, ld):
    n, F = X.shape
    d_thr, d_nthr = thr_table(thresholds)
    bins = torch.full((F, ld), 255, dtype=torch.uint8, device=DEV)
    d_X = dev(X)
    hip._check(hip.lib().gcl_mos_fit_bin(d_X.data_ptr(), n, F, d_thr.data_ptr(), d_nthr.data_ptr(), bins.data_ptr(),
                                         ld, hip._stream()))
    return bins.cpu().numpy()


# ---- bin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,F,ld", [(1, 3, 1), (63, 20, 100), (257, 32, 257)])
def test_bin(n, F, ld):
    rng = np.random.default_rng(n)
    thresholds = [np.sort(rng.normal(0, 1, 254)) for _ in range(F)]
    thresholds[0] = np.zeros(0)              # a one-valued feature
    thresholds[1] = np.array([0.25])         # two bins
    X = rng.normal(0, 1, (n, F))
    for i in range(n):                       # on a threshold, below the first, above the last
        f = 2 + i % (F - 2)
        X[i, f] = (thresholds[f][(7 * i) % 254], thresholds[f][0] - 1.0, thresholds[f][-1] + 1.0)[i % 3]
    X[0, 1] = 0.25
    got = device_bins(X, thresholds, ld)
    assert np.array_equal(got[:, :n], hgb_ref.bin_rows(X, thresholds))
    assert np.all(got[:, n:] == 255), "bytes of the padding were written"
    assert got[0, :n].max() == 0 and got[1, 0] == 0
    if n >= 3:
        assert got[:, :n].max() == 254 and np.any(got[2:, :n] == 0)


def test_gradients():
    rng = np.random.default_rng(1)
    raw, y = rng.normal(0, 3, 1000), rng.normal(0, 3, 1000)
    g = torch.empty(1000, dtype=torch.float32, device=DEV)
    d_raw, d_y = dev(raw), dev(y)
    hip._check(hip.lib().gcl_mos_fit_gradients(d_raw.data_ptr(), d_y.data_ptr(), g.data_ptr(), 1000, hip._stream()))
    assert np.array_equal(g.cpu().numpy(), hgb_ref.gradients(raw, y))
    assert not np.array_equal(g.cpu().numpy(), raw.astype(np.float32) - y.astype(np.float32))


# ---- histogram ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hist_case():
    """4 000 rows, 20 features (one with every row in one bin), gradients that are multiples of 2^-10 (float64 sums are
    then exact in any order), a shuffled partition array."""
    rng = np.random.default_rng(11)
    n, F = 4000, 20
    bins = rng.integers(0, 255, (F, n)).astype(np.uint8)
    bins[3] = 7
    bins[4] = rng.integers(0, 3, n)
    g = (rng.integers(-4096, 4096, n) / 1024.0).astype(np.float32)
    part = rng.permutation(n).astype(np.int32)
    return dict(n=n, F=F, bins=bins, g=g, part=part, d_bins=dev(bins), d_g=dev(g), d_part=dev(part), ws=ws_for(n, 0, F))


def device_hist(c, start, count):
    F = c["F"]
    hs = torch.full((F, 256), -1.0, dtype=torch.float64, device=DEV)
    hc = torch.full((F, 256), 77, dtype=torch.int32, device=DEV)
    ws, need = c["ws"]
    hip._check(hip.lib().gcl_mos_fit_histogram(c["d_bins"].data_ptr(), c["n"], F, c["d_part"].data_ptr(),
                                               c["d_g"].data_ptr(), start, count, hs.data_ptr(), hc.data_ptr(),
                                               ws.data_ptr(), need, hip._stream()))
    return hs, hc


@pytest.mark.parametrize("count", SEGMENTS)
def test_histogram_exact(hist_case, count):
    c, start = hist_case, 777
    hs, hc = device_hist(c, start, count)
    rs, rc = hgb_ref.histogram(c["bins"], c["part"][start:start + count], c["g"])
    assert np.array_equal(hc.cpu().numpy().astype(np.uint32), rc)
    assert hs.cpu().numpy().tobytes() == rs.tobytes()
    assert hc.cpu().numpy()[3, 7] == count and hc.cpu().numpy()[3].sum() == count


def test_histogram_subtraction_equals_direct_build(hist_case):
    c = hist_case
    ps, pc = device_hist(c, 100, 3000)
    ss, sc = device_hist(c, 100, 1100)
    ls, lc = torch.empty_like(ps), torch.empty_like(pc)
    hip._check(hip.lib().gcl_mos_fit_hist_subtract(ps.data_ptr(), pc.data_ptr(), ss.data_ptr(), sc.data_ptr(),
                                                   ls.data_ptr(), lc.data_ptr(), c["F"], hip._stream()))
    ds, dc = device_hist(c, 1200, 1900)
    assert torch.equal(lc, dc) and ls.cpu().numpy().tobytes() == ds.cpu().numpy().tobytes()


def test_histogram_repeats_its_bits():
    """Inexact sums (random float32 gradients): the same bytes twice, and the reference within float64 rounding."""
    rng = np.random.default_rng(12)
    n, F = 3000, 5
    c = dict(n=n, F=F, bins=rng.integers(0, 16, (F, n)).astype(np.uint8), g=rng.normal(0, 1, n).astype(np.float32),
             part=rng.permutation(n).astype(np.int32), ws=ws_for(n, 0, F))
    c.update(d_bins=dev(c["bins"]), d_g=dev(c["g"]), d_part=dev(c["part"]))
    a, _ = device_hist(c, 0, n)
    b, _ = device_hist(c, 0, n)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    rs, rc = hgb_ref.histogram(c["bins"], c["part"], c["g"])
    # two summation orders of m float64 terms differ by at most 2 (m - 1) 2^-53 sum |g| (Higham, Accuracy and
    # Stability of Numerical Algorithms, eq. 4.4)
    mag, _ = hgb_ref.histogram(c["bins"], c["part"], np.abs(c["g"]))
    assert np.all(np.abs(a.cpu().numpy() - rs) <= 2.0 * rc * 2.0 ** -53 * mag)


# ---- split -------------------------------------------------------------------------------------------------------------
def device_split(hs, hc, nthr, n, G, msl, l2=0.1):
    F = hs.shape[0]
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    iout = torch.zeros(4, dtype=torch.int32, device=DEV)
    ws, need = ws_for(0, 0, F)
    d_hs, d_hc, d_nthr = dev(hs), dev(hc.astype(np.uint32)), dev(np.asarray(nthr, dtype=np.int32))
    hip._check(hip.lib().gcl_mos_fit_split(d_hs.data_ptr(), d_hc.data_ptr(), F, d_nthr.data_ptr(), n, float(G), msl, l2,
                                           out.data_ptr(), iout.data_ptr(), ws.data_ptr(), need, hip._stream()))
    o, i = out.cpu().numpy(), iout.cpu().numpy()
    return dict(gain=float(o[0]), sum_g_left=float(o[1]), feature=int(i[0]), bin=int(i[1]), n_left=int(i[2]),
                missing_left=int(i[3]))


def check_split(hs, hc, nthr, n, G, msl, l2=0.1):
    got = device_split(hs, hc, nthr, n, G, msl, l2)
    ref = hgb_ref.best_split(hs, hc, nthr, n, G, msl, l2)
    if ref["gain"] <= 0:
        assert got["gain"] <= 0
    else:
        assert got == ref, (got, ref)
    return got


def hist_of(rows):
    """rows: {feature: [(bin, count, sum_g), ...]} -> histogram planes [F, 256]."""
    F = max(rows) + 1
    hs, hc = np.zeros((F, 256)), np.zeros((F, 256), dtype=np.uint32)
    for f, entries in rows.items():
        for b, cnt, s in entries:
            hc[f, b], hs[f, b] = cnt, s
    return hs, hc


def test_split_min_samples_leaf_runner_up_wins():
    # the cut after bin 0 separates the gradients best but leaves 5 rows on the left
    hs, hc = hist_of({0: [(0, 5, -50.0), (1, 45, 9.0), (2, 50, 41.0)]})
    got = check_split(hs, hc, [2], 100, 0.0, 20)
    assert (got["bin"], got["n_left"]) == (1, 50)
    free = check_split(hs, hc, [2], 100, 0.0, 1)
    assert free["bin"] == 0 and free["gain"] > got["gain"]


def test_split_equal_gain_lowest_feature_and_bin():
    same = [(0, 30, -12.0), (5, 40, 12.0)]
    hs, hc = hist_of({0: [(0, 70, 0.0)], 1: same, 2: same})
    got = check_split(hs, hc, [3, 9, 9], 70, 0.0, 20)
    assert got["feature"] == 1 and got["gain"] > 0
    # bins 1 .. 4 are empty: cutting after bin 0, 1, 2, 3 or 4 gives the same gain
    assert got["bin"] == 0 and got["n_left"] == 30


def test_split_no_valid_split():
    hs, hc = hist_of({0: [(0, 10, -5.0), (1, 25, 5.0)], 1: [(3, 35, 0.0)]})
    assert check_split(hs, hc, [4, 4], 35, 0.0, 20)["gain"] <= 0          # no side reaches 20 rows
    hs, hc = hist_of({0: [(0, 30, 0.0), (1, 30, 0.0)]})
    assert check_split(hs, hc, [1], 60, 0.0, 20)["gain"] <= 0             # no gradient: gain 0 is a leaf
    hs, hc = hist_of({0: [(0, 60, 3.0)]})
    assert check_split(hs, hc, [0], 60, 3.0, 20)["gain"] <= 0             # a feature without thresholds


def test_split_missing_go_to_left_on_a_tie():
    hs, hc = hist_of({0: [(0, 30, -6.0), (1, 30, 6.0)]})
    assert check_split(hs, hc, [1], 60, 0.0, 20)["missing_left"] == 0     # n_left == n_right
    hs, hc = hist_of({0: [(0, 31, -6.0), (1, 29, 6.0)]})
    assert check_split(hs, hc, [1], 60, 0.0, 20)["missing_left"] == 1


def test_split_random_histograms():
    rng = np.random.default_rng(21)
    for F, n in ((3, 500), (20, 1500), (32, 4000)):
        bins = rng.integers(0, 255, (F, n)).astype(np.uint8)
        bins[0] = rng.integers(0, 2, n)
        g = rng.normal(0, 1, n).astype(np.float32)
        hs, hc = hgb_ref.histogram(bins, np.arange(n), g)
        nthr = [1] + [254] * (F - 1)
        got = check_split(hs, hc, nthr, n, float(np.cumsum(hs[0])[-1]), 20)
        assert got["gain"] > 0


# ---- partition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", SEGMENTS[1:])
def test_partition_stable(count):
    rng = np.random.default_rng(count)
    n, F, start = 4000, 3, 333
    bins = rng.integers(0, 10, (F, n)).astype(np.uint8)
    part = rng.permutation(n).astype(np.int32)
    seg = part[start:start + count]
    b = 4
    while not 0 < np.count_nonzero(bins[2, seg] <= b) < count:  # an empty side never reaches the kernel
        bins[2, seg[0]], bins[2, seg[-1]] = 0, 9
    d_part, d_bins, n_left = dev(part), dev(bins), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws, need = ws_for(n, 0, F)
    hip._check(hip.lib().gcl_mos_fit_partition(d_bins.data_ptr(), n, d_part.data_ptr(), start, count, 2, b,
                                               n_left.data_ptr(), ws.data_ptr(), need, hip._stream()))
    left, right = hgb_ref.partition(bins, seg, 2, b)
    got = d_part.cpu().numpy()
    assert int(n_left.item()) == len(left) and len(left) + len(right) == count
    assert np.array_equal(got[start:start + len(left)], left)
    assert np.array_equal(got[start + len(left):start + count], right)
    assert np.array_equal(got[:start], part[:start]) and np.array_equal(got[start + count:], part[start + count:])


# ---- tree --------------------------------------------------------------------------------------------------------------
def device_tree(X, y, thresholds, max_leaf_nodes=31, max_depth=8, msl=20, l2=0.1, lr=0.05, trees=1):
    n, F = X.shape
    L = hip.lib()
    ld = (n + 255) // 256 * 256
    d_thr, d_nthr = thr_table(thresholds)
    bins = dev(np.pad(hgb_ref.bin_rows(X, thresholds), ((0, 0), (0, ld - n))))
    raw0, d_y = float(np.mean(y)), dev(y)
    raw = torch.full((n,), raw0, dtype=torch.float64, device=DEV)
    ws, need = ws_for(n, 0, F, max_leaf_nodes)
    nodes = torch.zeros(trees * (2 * max_leaf_nodes - 1) * 16, dtype=torch.uint8, device=DEV)
    roots = torch.zeros(trees + 1, dtype=torch.int32, device=DEV)
    state = torch.zeros(2, dtype=torch.int32, device=DEV)
    for _ in range(trees + 1):  # the call past max_iter must change nothing
        hip._check(L.gcl_mos_fit_tree(bins.data_ptr(), ld, n, F, d_nthr.data_ptr(), d_thr.data_ptr(), d_y.data_ptr(),
                                      raw.data_ptr(), None, 0, 0, None, None, max_leaf_nodes, max_depth, msl, l2, lr,
                                      trees, nodes.data_ptr(), roots.data_ptr(), None, state.data_ptr(), ws.data_ptr(),
                                      need, hip._stream()))
    grown, total = state.cpu().tolist()
    assert grown == trees
    p = nodes[:total * 16].cpu().numpy().view([("v", "<f8"), ("a", "<u4"), ("b", "<u4")])
    b = p["b"]
    flat = dict(feature=(b >> 24) & 31, value=p["v"], left=p["a"].astype(np.int64), right=(b & 0xFFFFFF).astype(np.int64),
                missing_left=(b >> 29) & 1, is_leaf=(b >> 30) & 1)
    return flat, roots.cpu().numpy()[:trees], raw.cpu().numpy(), raw0


@pytest.fixture(scope="module")
def tree_table():
    rng = np.random.default_rng(31)
    n, F = 1300, 6
    X = np.column_stack([rng.normal(0, 1, n), np.round(rng.uniform(0, 20, n)), np.full(n, 2.0),
                         np.where(rng.random(n) < 0.6, 0.0, rng.exponential(1, n)), rng.normal(0, 1, n),
                         rng.uniform(-1, 1, n)]).astype(np.float32).astype(np.float64)
    y = (np.sin(2 * X[:, 0]) + 0.1 * X[:, 1] + (X[:, 3] > 0) + rng.normal(0, 0.3, n)).astype(np.float32).astype(np.float64)
    from graphcast_lite_amd import mos
    return X, y, mos.bin_thresholds(X), F


@pytest.mark.parametrize("n,leaves,depth", [(1300, 31, 8), (1300, 2, 8), (1300, 31, 1), (1300, 5, 3), (40, 31, 8),
                                            (39, 31, 8)])
def test_tree(tree_table, n, leaves, depth):
    X, y, th, F = tree_table
    X, y = X[:n], y[:n]
    trees = 2 if n == 1300 and leaves == 31 else 1
    flat, roots, raw, raw0 = device_tree(X, y, th, leaves, depth, trees=trees)
    ref = hgb_ref.fit(X, y, th, trees, max_leaf_nodes=leaves, max_depth=depth)
    rflat, rroots = hgb_ref.flatten(ref["trees"])
    bad = hgb_ref.same_forest(flat, roots, rflat, rroots, rtol=1e-12)
    assert not bad, "\n".join(bad)
    n_leaf = int(flat["is_leaf"].sum())
    assert len(flat["value"]) == len(rflat["value"]) and n_leaf <= leaves * trees
    if n == 39:
        assert len(flat["value"]) == 1 and n_leaf == 1, "fewer than 2 min_samples_leaf rows: a single leaf"
    if n == 40:
        assert len(flat["value"]) in (1, 3)
    if depth == 1 and n == 1300:
        assert len(flat["value"]) == 3 * trees
    if leaves == 2 and n == 1300:
        assert n_leaf == 2
    idx = np.arange(len(flat["value"]))
    sp = flat["is_leaf"] == 0
    assert np.all(flat["left"][sp] > idx[sp]) and np.all(flat["right"][sp] > idx[sp]), "children follow parents"
    # raw: every training row moved exactly once per tree, by its leaf's value
    np.testing.assert_allclose(raw, ref["raw"], rtol=1e-12, atol=0)
    if trees == 1:
        leaf_values = flat["value"][flat["is_leaf"] == 1]
        step = raw - raw0
        assert np.all(np.min(np.abs(step[:, None] - leaf_values[None, :]), axis=1) <= 1e-15)
