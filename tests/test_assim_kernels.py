"""The data-assimilation kernels (csrc/assim.hip) called directly through their hip.py wrappers, on operands laid out by
tests/helpers/layouts.py (NaN around every input, the sentinel around every output), against restatements written here
from the formulas in the kernel file's comments.  Nothing here imports assimilation.py.

Rules:
  factor, solve  W is float64 work rounded to float32 once, so |W - W64| <= spacing(float32(|W64|)) element-wise against
                 np.linalg.solve on the same covariance.  The CPU part shows that the inputs leave that bound to the
                 kernel: np.linalg.solve, a Cholesky solve and a numpy restatement of the root-free elimination agree to
                 1e-2 of a float32 spacing on the same stations.  The factor's strict upper triangle is the bit-exact
                 transpose of the strict lower one, and X S X^T = D within the backward error of an m-step float64 elimination.
  innovation     exact float64 differences: torch.equal
  analysis       float64 with the full haversine and no cut as the arbiter; the kernel may be at most twice as far from
                 it as a numpy float32 restatement of the kernel's arithmetic, plus 1e-5 of the float64 magnitude, in norm
                 and in max-abs; everything outside (node_row, chans) keeps its bits; each sample of the per-sample
                 kernel has the bits of the one-setting kernel run alone with its setting and its own cut
  nudging        bit-equal to torch CPU float32; in place, what is not nudged keeps its bits, NaN payloads included
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, Guarded, Rows, Worst, launched, same_bits, targs  # noqa: E402

gpu = pytest.mark.gpu
R_EARTH = 6371000.0
SB2, DIAG = 0.64, 0.25
W_ = Worst("assimilation kernels")


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64).to(DEV).contiguous()


def triple(lat, lon):
    """(lat float64, lon float64, cos(lat) float32) in radians on the device: what the analysis kernels take."""
    return f64(lat), f64(lon), torch.from_numpy(np.cos(lat).astype(np.float32)).to(DEV)


def hav(la1, lo1, la2, lo2):
    """Pairwise haversine angle (radians, float64) of points 1 [p] and 2 [q]: 2 asin(sqrt(a))."""
    s1 = np.sin(0.5 * (la1[:, None] - la2[None, :]))
    s2 = np.sin(0.5 * (lo1[:, None] - lo2[None, :]))
    a = s1 * s1 + np.cos(la1)[:, None] * np.cos(la2)[None, :] * (s2 * s2)
    return 2.0 * np.arcsin(np.sqrt(np.minimum(a, 1.0)))


def rl2_of(L):
    return (R_EARTH / L) ** 2


def cut_of(rl2):
    """th_cut, a_cut: weights below exp(-120) are 0 in float32; a correlation length too long for that disables both."""
    th = math.sqrt(120.0 / rl2)
    return (th, math.sin(0.5 * th) ** 2) if th < math.pi else (10.0, 2.0)


# ------------------------------------------------------------------------------------------------------------------
# Station covariance, factor, solve
# ------------------------------------------------------------------------------------------------------------------
MS = [1, 2, 31, 32, 33, 64, 65, 128, 129, 255, 256, 257]  # 32 x 32 mirror tiles, 64 lanes, four rows per block, 256 threads
LS = [150e3, 800e3, 3000e3]
NRHS = [1, 7, 8, 9, 17]  # eight right-hand sides per block


def stations(m):
    """m seeded stations (radians) in a 50 x 90 degree box across the 0 / 360 seam, the last a duplicate of the first."""
    rng = np.random.default_rng(500 + m)
    lat, lon = np.radians(10 + 50 * rng.random(m)), np.radians((330 + 90 * rng.random(m)) % 360)
    if m > 2:
        lat[m - 1], lon[m - 1] = lat[0], lon[0]
    return lat, lon


def covariance(lat, lon, L):
    th = hav(lat, lon, lat, lon)
    return SB2 * np.exp(-rl2_of(L) * th * th) + DIAG * np.eye(len(lat))


def rhs_of(n, m):
    return np.random.default_rng(n * 1000 + m).standard_normal((n, m)) * 2


def factor_np(S):
    """assim.hip's root-free elimination in numpy: pivot by pivot, U^-T grows in the strict lower triangle while the
    upper one is reduced; the strict lower triangle is then mirrored."""
    M = S.copy()
    m = len(M)
    for j in range(m - 1):
        li = M[j, j + 1:] / M[j, j]
        M[j + 1:, :j] -= li[:, None] * M[j, :j][None, :]
        M[j + 1:, j] = -li
        M[j + 1:, j + 1:] -= np.triu(li[:, None] * M[j, j + 1:][None, :])
    iu = np.triu_indices(m, 1)
    M[iu] = M.T[iu]
    return M


def solve_np(M, rhs):
    """W = X^T D^-1 X rhs with X unit lower (strict part in M), X^T in the upper triangle, D on the diagonal."""
    z = (rhs + rhs @ np.tril(M, -1).T) / np.diag(M)
    return z + z @ np.triu(M, 1).T


def spacing32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def factor_residual(M, S):
    """max |X S X^T - D| over max bound, bound = 8 m 2^-53 |X| (|X^-1| |D| |X^-T| + |S|) |X|^T: the backward error of
    an m-step elimination, a few m 2^-53 of |X^-1| |D| |X^-T|, carried through X . X^T, plus the rounding of this
    product itself.  Both maxima are over the whole matrix: at the short length far stations have covariances of 1e-250
    and below, whose products underflow along the way, so an element-wise ratio would say nothing there."""
    m = len(S)
    X = np.tril(M, -1) + np.eye(m)
    aX, aXi = np.abs(X), np.abs(np.linalg.inv(X))
    res = np.abs(X @ S @ X.T - np.diag(np.diag(M)))
    bound = 8 * m * 2.0 ** -53 * (aX @ ((aXi * np.abs(np.diag(M))[None, :]) @ aXi.T + np.abs(S)) @ aX.T)
    return float(res.max() / bound.max())


@pytest.mark.parametrize("L", LS)
def test_solvers_agree_on_these_stations(L):
    """CPU: np.linalg.solve, a Cholesky solve and the restated root-free elimination agree to 1e-2 of a float32
    spacing for every station set and length of the GPU test, so the one-spacing bound there is left to the kernel."""
    worst = 0.0
    for m in MS:
        S = covariance(*stations(m), L)
        rhs = rhs_of(17, m)
        W64 = np.linalg.solve(S, rhs.T).T
        C = np.linalg.cholesky(S)
        Wc = np.linalg.solve(C.T, np.linalg.solve(C, rhs.T)).T
        M = factor_np(S)
        Wf = solve_np(M, rhs)
        assert np.array_equal(np.triu(M, 1), np.tril(M, -1).T)
        assert factor_residual(M, S) <= 1.0
        sp = spacing32(W64)
        worst = max(worst, float((np.abs(Wc - W64) / sp).max()), float((np.abs(Wf - W64) / sp).max()))
    print(f"[assimilation kernels] L={L / 1e3:.0f} km: solvers agree to {worst:.2e} of a float32 spacing")
    assert worst < 1e-2


@gpu
@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("m", MS)
def test_oi_factor_and_solve(hip, m, L):
    lat, lon = stations(m)
    S = covariance(lat, lon, L)
    M = hip.oi_factor(f64(lat), f64(lon), SB2, rl2_of(L), DIAG)
    Mh = M.cpu().numpy()
    assert np.array_equal(np.triu(Mh, 1), np.tril(Mh, -1).T), "the upper triangle is not the transpose of the lower one"
    r = factor_residual(Mh, S)
    W_.worst["factor X S X^T = D"] = max(W_.worst.get("factor X S X^T = D", 0.0), r)
    assert r <= 1.0, f"X S X^T differs from D by {r:.2f} of the bound"
    for n in NRHS:
        rhs = rhs_of(n, m)
        R = torch.full((n + 2, m), NAN, dtype=torch.float64, device=DEV)  # a NaN row on either side of the n rows
        R[1:n + 1] = torch.from_numpy(rhs).to(DEV)
        tmp, Wd = Guarded((n, m), torch.float64), Guarded((n, m))
        hip.oi_solve(M, R[1:n + 1], tmp.view, Wd.view)
        torch.cuda.synchronize()
        assert tmp.untouched() and Wd.untouched()
        W64 = np.linalg.solve(S, rhs.T).T
        W_.within("solve", Wd.view, torch.from_numpy(W64).to(DEV), torch.from_numpy(spacing32(W64)).to(DEV),
                  f"m={m} L={L} n={n}")
    W_.report("factor X S X^T = D", "solve")


# ------------------------------------------------------------------------------------------------------------------
# Innovation
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("m,nch", [(1, 1), (129, 3), (300, 5)])
def test_oi_innovation(hip, B, m, nch):
    rng = np.random.default_rng(m + B)
    G, C = 400, nch + 3
    chans = rng.permutation(C)[:nch]  # a subset, not ascending
    obs_row, node_row = rng.integers(0, G, m), rng.integers(0, G, m)
    assert m == 1 or (obs_row != node_row).any()
    obs = np.full((B, G, C), NAN, np.float32)
    xb = np.full((B, G, C), NAN, np.float32)
    for a, rows in ((obs, obs_row), (xb, node_row)):  # only what the kernel may read is a number
        a[:, rows[:, None], chans[None, :]] = rng.standard_normal((B, m, nch)) * 30 + 270
    O, X = Rows.of(torch.from_numpy(obs), "pad_nan", NAN), Rows.of(torch.from_numpy(xb), "odd_ld", NAN)
    rhs = Guarded((B * nch, m), torch.float64)
    hip.oi_innovation(O.view, X.view, i32(obs_row), i32(node_row), i32(chans), rhs.view)
    torch.cuda.synchronize()
    ref = obs[:, obs_row][:, :, chans].astype(np.float64) - xb[:, node_row][:, :, chans].astype(np.float64)  # [B, m, nch]
    assert rhs.untouched()
    assert torch.equal(rhs.view.cpu(), torch.from_numpy(ref.transpose(0, 2, 1).reshape(B * nch, m)))


# ------------------------------------------------------------------------------------------------------------------
# Analysis
# ------------------------------------------------------------------------------------------------------------------
def geometry(n_nodes, m, seed):
    """Nodes and stations (radians) over the globe.  Node 0 and station 0 are 1.4 degrees apart across the 0 / 360 seam;
    node 1 is the north pole with station 2 half a degree from it, node 2 the south pole with station 3 beside it;
    station 1 is far from everything."""
    rng = np.random.default_rng(seed)
    nlat, nlon = rng.uniform(-90, 90, n_nodes), rng.uniform(0, 360, n_nodes)
    slat, slon = rng.uniform(-90, 90, m), rng.uniform(0, 360, m)
    for arr, fixed in ((nlat, [10.0, 90.0, -90.0]), (nlon, [359.5, 123.0, 0.0]), (slat, [11.0, -40.0, 89.5, -89.7]),
                       (slon, [0.5, 170.0, 200.0, 0.0])):
        k = min(len(arr), len(fixed))
        arr[:k] = fixed[:k]
    return np.radians(nlat), np.radians(nlon), np.radians(slat), np.radians(slon)


def analysis_f64(xb, Wm, chans, node_row, geo, sb2, rl2):
    """float64, full haversine, no cut: x_a[b, node_row[i], chans[q]] = x_b + sum_k sb2 K(i, k) W[b nch + q, k]; sb2 and
    rl2 scalars or one per sample."""
    nlat, nlon, slat, slon = geo
    B, nch = xb.shape[0], len(chans)
    th = hav(nlat, nlon, slat, slon)
    xa = xb.astype(np.float64).copy()
    for b in range(B):
        s, r = (sb2[b], rl2[b]) if np.ndim(sb2) else (sb2, rl2)
        K = float(s) * np.exp(-float(r) * th * th)
        inc = K @ Wm[b * nch:(b + 1) * nch].astype(np.float64).T  # [n_nodes, nch]
        xa[b][node_row[:, None], chans[None, :]] += inc
    return xa


def analysis_f32(xb, Wm, chans, node_row, geo, sb2, rl2, cut):
    """The kernel's stated arithmetic in numpy float32: float64 coordinate differences rounded to float32, the haversine
    and the weight in float32, pairs beyond the cut weightless, the stations added one by one in float32."""
    nlat, nlon, slat, slon = geo
    B, nch = xb.shape[0], len(chans)
    f = np.float32
    dlat = (nlat[:, None] - slat[None, :]).astype(f)
    dlon = (nlon[:, None] - slon[None, :]).astype(f)
    s1, s2 = np.sin(f(0.5) * dlat), np.sin(f(0.5) * dlon)
    a = s1 * s1 + (np.cos(nlat).astype(f)[:, None] * np.cos(slat).astype(f)[None, :]) * (s2 * s2)
    inside = (np.abs(dlat) <= f(cut[0])) & (a <= f(cut[1]))
    th = f(2) * np.arcsin(np.sqrt(np.minimum(a, f(1))))
    xa = xb.copy()
    for b in range(B):
        s, r = (sb2[b], rl2[b]) if np.ndim(sb2) else (sb2, rl2)
        w = np.where(inside, f(s) * np.exp(-f(r) * (th * th)), f(0))
        Wb = Wm[b * nch:(b + 1) * nch]
        acc = np.zeros((len(nlat), nch), f)
        for k in range(len(slat)):
            acc = acc + w[:, k, None] * Wb[None, :, k]
        assert acc.dtype == f
        xa[b][node_row[:, None], chans[None, :]] += acc
    return xa, inside


def fp64_rule(x_hip, x32, x64, tag):
    """The project's arbitration rule (tests/test_assimilation.py::_fp64_rule), with the two ratios recorded."""
    x_hip, x32, x64 = (np.asarray(v, dtype=np.float64) for v in (x_hip, x32, x64))
    dh, d32 = x_hip - x64, x32 - x64
    bn = 2 * np.linalg.norm(d32) + 1e-5 * np.linalg.norm(x64)
    bm = 2 * np.abs(d32).max() + 1e-5 * np.abs(x64).max()
    rn, rm = np.linalg.norm(dh) / bn, np.abs(dh).max() / bm
    W_.worst["analysis"] = max(W_.worst.get("analysis", 0.0), rn, rm)
    assert np.isfinite(dh).all() and rn <= 1.0 and rm <= 1.0, (tag, rn, rm)


class Field:
    """A background [B, G, C] on padded rows with a batch gap, the analysis written in place or into a second,
    sentinel-filled layout, and what may change: the (node_row, chans) elements."""

    def __init__(self, xb, chans, node_row, in_place):
        B, G, C = xb.shape
        self.xb = Rows.of(torch.from_numpy(xb), "pad_nan", NAN)
        self.xa = self.xb if in_place else Rows(G, C, "odd_ld", SENT, "out", B=B)
        self.before = self.xa.buf.clone()
        self.may = torch.zeros(B, G, C, dtype=torch.bool)
        self.may[:, torch.from_numpy(node_row)[:, None], torch.from_numpy(chans)[None, :]] = True
        self.may = self.may.to(DEV)

    def written(self, what):
        """The analysis at the (node_row, chans) elements, after checking that nothing else changed."""
        xa = self.xa
        assert same_bits(xa.buf[~xa.inside], self.before[~xa.inside]), f"{what}: the kernel wrote outside the view"
        before = torch.as_strided(self.before, xa.view.shape, xa.view.stride(), xa.view.storage_offset())
        assert same_bits(xa.view[~self.may], before[~self.may]), f"{what}: rows or channels outside the analysis changed"
        return xa.view


NN = [1, 255, 256, 257]  # 256 nodes per block
MM = [1, 127, 128, 129, 300]  # station tiles of 128
COLS = [(1, 1), (1, 8), (3, 3), (2, 8), (1, 17), (3, 8), (5, 5), (4, 8), (3, 11), (5, 8)]  # B nch = 1 .. 40


def analysis_case(n_nodes, m, B, nch, use_rows, seed):
    rng = np.random.default_rng(seed)
    geo = geometry(n_nodes, m, seed)
    C = nch + 3
    chans = rng.permutation(C)[:nch]
    G = n_nodes + 9 if use_rows else n_nodes
    node_row = rng.permutation(G)[:n_nodes] if use_rows else np.arange(n_nodes)
    xb = (rng.standard_normal((B, G, C)) * 5 + 270).astype(np.float32)
    z = rng.standard_normal((B * nch, m))
    Wm = (np.sign(z) * (1 + np.abs(z))).astype(np.float32)
    return geo, chans, node_row, xb, Wm


@gpu
@pytest.mark.parametrize("L", [150e3, 3000e3])
@pytest.mark.parametrize("B,nch", COLS)
def test_oi_analysis(hip, B, nch, L):
    """Four (nodes, stations, node_row, in place) combinations per column count, walking through every node and station
    count; L = 150 km has the cut active, L = 3000 km disabled."""
    ci = COLS.index((B, nch))
    rl2 = rl2_of(L)
    cut = cut_of(rl2)
    assert (cut == (10.0, 2.0)) == (L == 3000e3)
    want = 8 if B * nch <= 8 else 16 if B * nch <= 16 else 24 if B * nch <= 24 else 32
    for j in range(4):
        n_nodes, m = NN[(ci + j) % 4], MM[(ci + 2 * j + (L > 1e6)) % 5]
        use_rows, in_place = j % 2 == 0, j // 2 == (ci % 2)
        what = f"nodes={n_nodes} m={m} B={B} nch={nch} L={L} rows={use_rows} in_place={in_place}"
        geo, chans, node_row, xb, Wm = analysis_case(n_nodes, m, B, nch, use_rows, seed=100 * ci + j)
        x64 = analysis_f64(xb, Wm, chans, node_row, geo, SB2, rl2)
        x32, inside = analysis_f32(xb, Wm, chans, node_row, geo, SB2, rl2, cut)
        assert inside.any() and np.abs(x64 - xb).max() > 0.1, what
        if L == 150e3 and n_nodes * m > 1:
            assert (~inside).any(), what
        F = Field(xb, chans, node_row, in_place)
        _, names = launched(lambda: hip.oi_analysis(F.xb.view, F.xa.view, i32(chans), i32(node_row) if use_rows else None,
                                                    triple(*geo[:2]), triple(*geo[2:]), torch.from_numpy(Wm).to(DEV),
                                                    SB2, rl2, cut[0], cut[1]))
        assert targs(names, "oi_analysis_kernel") == [[str(want)]], names
        xa = F.written(what)
        may = F.may.cpu().numpy()
        fp64_rule(xa.cpu().numpy()[may], x32[may], x64[may], what)
    W_.report("analysis")


ROWS_CASES = [(2, 3, (2, 4)), (3, 4, (4, 4)), (5, 3, (8, 4)), (9, 2, (8, 4)), (1, 11, (1, 8)), (2, 8, (2, 8)),
              (3, 11, (4, 8)), (7, 11, (4, 8)), (5, 9, (6, 8))]


def pick(B, nch):
    """(NS, CC) as gcl_oi_analysis_rows picks them: CC = 4 up to four channels, else 8; of the widths on offer the one
    with the fewest sample groups, the narrowest among equals."""
    widths, CC = ((2, 4, 8), 4) if nch <= 4 else ((1, 2, 4, 6), 8)
    return min(widths, key=lambda ns: (-(-B // ns), ns)), CC


@gpu
@pytest.mark.parametrize("B,nch,inst", ROWS_CASES)
def test_oi_analysis_rows(hip, B, nch, inst):
    """Every (NS, CC) instance, with a partial last sample group ((3, 4), (5, 3), (9, 2), (3, 11), (7, 11), (5, 9)), a
    partial last channel chunk (nch = 2, 3, 9, 11), correlation lengths in runs of one and of several samples, one of
    them 150 km against the widest 800 km."""
    assert pick(B, nch) == inst
    assert {c[2] for c in ROWS_CASES} == {(2, 4), (4, 4), (8, 4), (1, 8), (2, 8), (4, 8), (6, 8)}
    ci = [c[:2] for c in ROWS_CASES].index((B, nch))
    n_nodes, m, use_rows, in_place = NN[ci % 4], MM[1 + ci % 4], ci % 2 == 0, ci % 3 == 0
    Ls = ([800e3, 800e3, 400e3, 150e3, 150e3, 150e3, 300e3, 200e3, 200e3] if B > 1 else [800e3])[:B]
    rl2_row = np.array([rl2_of(v) for v in Ls], np.float32)
    sb2_row = (0.3 + 0.1 * np.arange(B)).astype(np.float32)
    cut = cut_of(rl2_of(max(Ls)))
    assert cut[0] < math.pi
    what = f"B={B} nch={nch} nodes={n_nodes} m={m} rows={use_rows} in_place={in_place}"
    geo, chans, node_row, xb, Wm = analysis_case(n_nodes, m, B, nch, use_rows, seed=7000 + ci)
    F = Field(xb, chans, node_row, in_place)
    nodes, stns, Wd = triple(*geo[:2]), triple(*geo[2:]), torch.from_numpy(Wm).to(DEV)
    rows_d = i32(node_row) if use_rows else None
    _, names = launched(lambda: hip.oi_analysis_rows(F.xb.view, F.xa.view, i32(chans), rows_d, nodes, stns, Wd,
                                                     torch.from_numpy(sb2_row).to(DEV), torch.from_numpy(rl2_row).to(DEV),
                                                     cut[0], cut[1]))
    assert targs(names, "oi_analysis_rows_kernel") == [[str(inst[0]), str(inst[1])]], names
    xa = F.written(what)
    for b in range(B):  # the one-setting kernel, alone, with this sample's setting and its own cut
        own = cut_of(float(rl2_row[b]))
        alone = Field(xb[b:b + 1], chans, node_row, False)
        hip.oi_analysis(alone.xb.view, alone.xa.view, i32(chans), rows_d, nodes, stns, Wd[b * nch:(b + 1) * nch],
                        float(sb2_row[b]), float(rl2_row[b]), own[0], own[1])
        assert same_bits(alone.written(what)[0][F.may[0]], xa[b][F.may[b]]), f"{what}: sample {b} differs from the " \
            "one-setting kernel run alone"
    x64 = analysis_f64(xb, Wm, chans, node_row, geo, sb2_row, rl2_row)
    x32, inside = analysis_f32(xb, Wm, chans, node_row, geo, sb2_row, rl2_row, cut)
    assert inside.any() and (n_nodes * m == 1 or (~inside).any()) and np.abs(x64 - xb).max() > 0.1, what
    may = F.may.cpu().numpy()
    fp64_rule(xa.cpu().numpy()[may], x32[may], x64[may], what)
    W_.report("analysis")


# ------------------------------------------------------------------------------------------------------------------
# Nudging
# ------------------------------------------------------------------------------------------------------------------
def nudge_data(B, G, C, seed):
    """Forecast and observations (half of them NaN); where the observation is NaN some forecast values are NaNs with a
    payload, which nothing may alter."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, G, C, generator=g) * 50
    o = f + torch.randn(B, G, C, generator=g)
    o[torch.rand(B, G, C, generator=g) < 0.5] = NAN
    payload = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)
    f[torch.isnan(o) & (torch.rand(B, G, C, generator=g) < 0.1)] = payload
    return f, o


def nudge_ref(f, o, c0, c1, form, cmask):
    """nudging.py's two formulas in torch CPU float32, one rounding per operation; untouched elements keep f's bits."""
    mask = ~torch.isnan(o)
    if cmask is not None:
        mask = mask & cmask.bool()
    a = f.clone()
    a[mask] = f[mask] + c1 * (o[mask] - f[mask]) if form == 0 else c0 * f[mask] + c1 * o[mask]
    return a


@gpu
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("B,G,C,masked", [(1, 1, 1, False), (3, 211, 13, True), (2, 40, 19, False), (2, 0, 5, True)])
def test_nudge(hip, form, in_place, B, G, C, masked):
    f, o = nudge_data(B, G, C, seed=G + C)
    cmask = (torch.arange(C) % 3 != 1).to(torch.uint8) if masked else None
    for alpha in (0.25, 1 / 3, 0.7777):
        Fr, Or = Rows.of(f, "pad_nan", NAN), Rows.of(o, "odd_ld", NAN)
        Out = Fr if in_place else Rows(G, C, "offset", SENT, "out", B=B)
        before = Out.buf.clone()
        hip.nudge(Fr.view, Or.view, Out.view, 1 - alpha, alpha, form, cmask.to(DEV) if masked else None)
        torch.cuda.synchronize()
        assert same_bits(Out.buf[~Out.inside], before[~Out.inside]), "nudge wrote outside its view"
        assert same_bits(Out.view, nudge_ref(f, o, 1 - alpha, alpha, form, cmask).to(DEV)), (form, in_place, alpha)
    W_.exact("nudging (bit-equal)")


@gpu
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("B,G,C,masked", [(1, 1, 1, False), (5, 211, 13, True), (4, 40, 19, False), (2, 0, 5, True)])
def test_nudge_rows(hip, in_place, broadcast, B, G, C, masked):
    """Row b nudged with alpha[b] at the stations of its network, or not at all (net_of_row = -1); the truth one per
    row or one for all."""
    g = torch.Generator().manual_seed(B * 100 + G)
    f, o = nudge_data(B, G, C, seed=G + C + 1)
    if broadcast:
        o = o[:1].contiguous()
        f[torch.isnan(f) & ~torch.isnan(o)] = 1.5  # a NaN forecast stays where no row is nudged
    n_net = 3
    smask = (torch.rand(n_net, G, generator=g) < 0.4).to(torch.uint8)
    net = (torch.arange(B) % (n_net + 1) - 1).to(torch.int32)  # -1, 0, 1, 2, -1, ..
    if B == 1:
        net[0] = 1
    alpha = (0.1 + 0.8 * torch.rand(B, generator=g)).float()
    cmask = (torch.arange(C) % 3 != 1).to(torch.uint8) if masked else None
    Fr, Or = Rows.of(f, "pad_nan", NAN), Rows.of(o, "odd_ld", NAN)
    Out = Fr if in_place else Rows(G, C, "offset", SENT, "out", B=B)
    before = Out.buf.clone()
    hip.nudge_rows(Fr.view, Or.view, Out.view, smask.to(DEV), net.to(DEV), alpha.to(DEV), cmask.to(DEV) if masked else None)
    torch.cuda.synchronize()
    ref = f.clone()
    for b in range(B):
        if net[b] < 0:
            continue
        ob = o[0 if broadcast else b]
        mask = smask[net[b]].bool()[:, None] & ~torch.isnan(ob)
        if masked:
            mask = mask & cmask.bool()
        ref[b][mask] = f[b][mask] + alpha[b] * (ob[mask] - f[b][mask])
    assert same_bits(Out.buf[~Out.inside], before[~Out.inside]), "nudge_rows wrote outside its view"
    assert same_bits(Out.view, ref.to(DEV)), (in_place, broadcast)
