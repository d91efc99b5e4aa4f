"""The WRF-benchmark kernels (csrc/wrf.hip) called through their thin hip.py wrappers on operands laid out by
tests/helpers/layouts.py (NaN around every float input, the sentinel around every output, 0 around the index tables).
Nothing here uses WrfBenchmark or compare_wrf_era5; the arithmetic is restated from include/gcl.h in numpy.

Rules:
  wrf_sample      bit-equal to the float64 restatement (four products added in corner order onto 0.0, NaN outside) and,
                  on the fixture, to what scipy produced (tests/golden/wrf_vectors.npz); guard bytes untouched
  wrf_scores      n exact; sum d^2, sum |d|, sum a, sum b within 4 P 2^-53 sum|x| of numpy's float64 sums (the bound on
                  two differently ordered float64 sums of P terms), sum d within the same bound taken against sum |d|;
                  an all-NaN job gives n = 0, an inf stays in the sums; two runs give the same bits
  wrf_box_means   bit-equal to numpy's float32 (x * std + mean)[:, rows].mean(axis=1)
  all three       two runs of every case give the same bits
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import wrf_case as WC  # noqa: E402
from layouts import DEV, NAN, SENT, Guarded, Rows, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
GRIDS = {"9x6": (np.linspace(10.0, 14.0, 9), np.linspace(-3.0, 2.0, 6)), "25x17": WC.axes()}


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(scope="module")
def W():
    from graphcast_lite_amd import wrf

    return wrf


def query(grid, P, seed):
    """P float32 points over the grid's extent and a little beyond it on every side; from the third point on, one
    exactly on the last longitude node and one on the last latitude node."""
    lons, lats = GRIDS[grid]
    rng = np.random.default_rng(seed)
    dx, dy = 0.08 * (lons[-1] - lons[0]), 0.08 * (lats[-1] - lats[0])
    lon = rng.uniform(lons[0] - dx, lons[-1] + dx, P)
    lat = rng.uniform(lats[0] - dy, lats[-1] + dy, P)
    if P == 1:
        lon[0], lat[0] = lons[3] + 0.1, lats[2] + 0.1
    if P >= 3:
        lon[1], lat[1] = lons[-1], lats[2] + 0.05
        lon[2], lat[2] = lons[4] + 0.05, lats[-1]
    return lon.astype(np.float32), lat.astype(np.float32)


def tables(W, grid, P, seed):
    lons, lats = GRIDS[grid]
    lon, lat = query(grid, P, seed)
    pos, w = W.wrf_point_tables(lons, lats, lon, lat)
    if P >= 63:
        sides = (lon < lons[0], lon > lons[-1], lat < lats[0], lat > lats[-1])
        assert all(s.any() for s in sides), "the case must have points outside on every side"
    if P >= 3:
        assert pos[1, 0] >= 0 and pos[2, 0] >= 0
    return pos, w


class Src:
    """nf fields of a grid inside a NaN buffer: stride 1 lays them back to back, a larger stride interleaves them as
    channels of a node.  `host` holds the float32 (or fp16) values, `offs` the element offset of every field."""

    def __init__(self, hip, pos, w, grid, nf, stride, dtype, seed, lead=5):
        lons, lats = GRIDS[grid]
        self.n = n = lons.size * lats.size
        assert stride == 1 or stride >= nf
        rng = np.random.default_rng(seed)
        vals = (250.0 + 30.0 * rng.standard_normal((nf, n))).astype(np.float16 if dtype == torch.float16 else np.float32)
        size = lead + (nf * n if stride == 1 else n * stride) + 3
        host = np.full(size, np.nan, dtype=vals.dtype)
        self.offs = [lead + (f * n if stride == 1 else f) for f in range(nf)]
        for f in range(nf):
            host[self.offs[f]:self.offs[f] + (n - 1) * stride + 1:stride] = vals[f]
        self.host, self.stride, self.vals = host, stride, vals
        self.buf = torch.from_numpy(host).to(DEV)
        self.pos = Guarded(pos.shape, torch.int32, 0, torch.from_numpy(np.array(pos)))
        self.w = Guarded(w.shape, torch.float64, NAN, torch.from_numpy(np.array(w)))
        self.source = hip.WrfSource(self.buf, stride, n, self.pos.view, self.w.view)
        self.np_pos, self.np_w = pos, w

    def sample(self, f, mul=None, add=None):
        """The restatement: float64 [P] of field f."""
        v = self.vals[f].astype(np.float32)
        if mul is not None:
            v = (v * np.float32(mul)).astype(np.float32)
            v = (v + np.float32(add)).astype(np.float32)
        safe = np.where(self.np_pos < 0, 0, self.np_pos)
        acc = np.zeros(self.np_pos.shape[0])
        for k in range(4):
            acc = acc + v[safe[:, k]].astype(np.float64) * self.np_w[:, k]
        acc[self.np_pos[:, 0] < 0] = np.nan
        return acc


# ----------------------------------------------------------------------------------------------------------------------
# gcl_wrf_sample
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["9x6", "25x17"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 257])
def test_wrf_sample_contract(hip, W, P, grid):
    pos, w = tables(W, grid, P, seed=P)
    nf = 3
    for dtype in (torch.float32, torch.float16):
        for stride in (1, WC.C, WC.P * WC.C):
            src = Src(hip, pos, w, grid, nf, stride, dtype, seed=11 * P + stride)
            for conv in (False, True):
                mul = np.float32([1.5, 0.01, 9.25]) if conv else None
                add = np.float32([-3.0, 273.15, 0.0]) if conv else None
                out = Guarded((nf, P), torch.float64, SENT)
                conv_t = (torch.from_numpy(mul).to(DEV), torch.from_numpy(add).to(DEV)) if conv else (None, None)
                hip.wrf_sample(src.source, src.offs, mul=conv_t[0], add=conv_t[1], out=out.view)
                again = hip.wrf_sample(src.source, src.offs, mul=conv_t[0], add=conv_t[1])
                torch.cuda.synchronize()
                assert same_bits(out.view, again), "two runs must give the same bits"
                for f in range(nf):
                    want = src.sample(f, mul[f] if conv else None, add[f] if conv else None)
                    assert same_bits(out.view[f].cpu(), torch.from_numpy(want)), (dtype, stride, conv, f)
                assert out.untouched() and src.pos.untouched() and bool(src.w.buf[:8].isnan().all())
                outside = pos[:, 0] < 0
                got = out.view.cpu()
                assert bool(got[:, torch.from_numpy(outside)].isnan().all())
                assert not bool(got[:, torch.from_numpy(~outside)].isnan().any())


def test_wrf_sample_reproduces_scipy_on_the_fixture(hip, W):
    gv = WC.golden()
    _, lat, lon, _, _ = W.load_wrf_json(WC.WRF_JSON)
    lons, lats = WC.axes()
    pos, w = W.wrf_point_tables(lons, lats, lon, lat)
    series = torch.from_numpy(WC.series()).to(DEV)
    source = hip.WrfSource(series, WC.C, 425, torch.from_numpy(np.array(pos)).to(DEV), torch.from_numpy(np.array(w)).to(DEV))
    offs = [(8 + h) * 425 * WC.C + WC.VAR_NAMES.index(n) for n in ("t2m", "10u", "10v", "sp") for h in range(5)]
    out = hip.wrf_sample(source, offs)
    assert same_bits(out.cpu().view(4, 5, 12, 10), torch.from_numpy(gv["interp"]))
    f32 = torch.from_numpy(WC.series()[8, :, :, 0].astype(np.float32) * np.float32(1.5)).to(DEV)
    source = hip.WrfSource(f32, 1, 425, source.pos, source.w)
    assert same_bits(hip.wrf_sample(source, [0]).cpu().view(12, 10), torch.from_numpy(gv["interp_f32"]))


def test_wrf_sample_rejects_what_leaves_the_buffer(hip, W):
    pos, w = tables(W, "9x6", 5, seed=1)
    src = Src(hip, pos, w, "9x6", 2, 1, torch.float32, seed=2)
    with pytest.raises(ValueError, match="leaves the source buffer"):
        hip.wrf_sample(src.source, [src.buf.numel() - 53])
    with pytest.raises(ValueError):
        hip.wrf_sample(src.source, [-1])
    with pytest.raises(ValueError):
        hip.wrf_sample(src.source, [])
    with pytest.raises(ValueError):
        hip.wrf_sample(src.source, src.offs, mul=torch.ones(2, device=DEV))


# ----------------------------------------------------------------------------------------------------------------------
# gcl_wrf_scores
# ----------------------------------------------------------------------------------------------------------------------
def six(a, b):
    m = ~(np.isnan(a) | np.isnan(b))
    with np.errstate(invalid="ignore", over="ignore"):
        d = a[m] - b[m]
        return np.array([m.sum(), d.sum(), (d * d).sum(), np.abs(d).sum(), a[m].sum(), b[m].sum()]), \
            np.array([0.0, np.abs(d).sum(), (d * d).sum(), np.abs(d).sum(), np.abs(a[m]).sum(), np.abs(b[m]).sum()])


def check_stats(got, want, mag, P, what):
    """n exact; the sums within 4 P 2^-53 of their magnitudes; non-finite sums equal as they are."""
    assert got[0] == want[0], (what, got[0], want[0])
    for q in range(1, 6):
        if not np.isfinite(want[q]):
            assert np.array_equal(got[q:q + 1], want[q:q + 1], equal_nan=True), (what, q, got[q], want[q])
        else:
            assert abs(got[q] - want[q]) <= WC.sum_bound(P, mag[q]), (what, q, got[q], want[q], WC.sum_bound(P, mag[q]))


class ScoreCase:
    """J jobs over P points cycling through the four pairings of side kinds - (point, grid 0), (grid 1, point),
    (point, point), (grid 0, grid 1) - with two sources that have different grids, dtypes, strides and tables.  From
    three jobs on, job 1 reads an all-NaN point field (n = 0) and job 2 a point field holding an inf."""

    def __init__(self, hip, W, P, J):
        self.P, self.J = P, J
        self.s0 = Src(hip, *tables(W, "25x17", P, seed=P), "25x17", 3, WC.C, torch.float16, seed=P + 1)
        self.s1 = Src(hip, *tables(W, "9x6", P, seed=P + 7), "9x6", 2, 1, torch.float32, seed=P + 2)
        rng = np.random.default_rng(P + 3)
        pts = (251.0 + 25.0 * rng.standard_normal((4, P))).astype(np.float32)
        pts[0, rng.random(P) < 0.03] = np.nan
        pts[2] = np.nan
        pts[3, P // 2] = np.inf
        self.pts_host = pts
        self.pts = Guarded((4, P), torch.float32, NAN, torch.from_numpy(pts))
        self.jobs, self.conv, self.want, self.mag = [], [], [], []
        for j in range(J):
            conv = j % 2 == 1
            flag = hip.WRF_CONVERT if conv else 0
            pf = 2 if (J >= 3 and j == 1) else 3 if (J >= 3 and j == 2) else j % 2
            point = (hip.WRF_POINT | flag, pf * P, 0.01 if conv else 1.0, 0.0)
            other = (hip.WRF_POINT | flag, (1 - j % 2) * P, 0.01 if conv else 1.0, 0.0)
            g0 = (hip.WRF_SRC0 | flag, self.s0.offs[j % 3], 1.25 if conv else 1.0, -7.5 if conv else 0.0)
            g1 = (hip.WRF_SRC1 | flag, self.s1.offs[j % 2], 0.5 if conv else 1.0, 100.0 if conv else 0.0)
            a, b = ((point, g0), (g1, point), (point, other), (g0, g1))[j % 4]
            self.jobs.append((a[0], a[1], b[0], b[1], 0, 0))
            self.conv.append((a[2], a[3], b[2], b[3]))
            want, mag = six(self.value(a, conv), self.value(b, conv))
            self.want.append(want)
            self.mag.append(mag)

    def value(self, side, conv):
        kind, off, mul, add = side
        which = kind & 3
        if which == 0:
            v = self.pts_host.reshape(-1)[off:off + self.P]
            if conv:
                v = (v * np.float32(mul)).astype(np.float32)
            return v.astype(np.float64)
        s = self.s0 if which == 1 else self.s1
        return s.sample(s.offs.index(off), mul if conv else None, add if conv else None)

    def run(self, hip):
        out = Guarded((self.J, 6), torch.float64, SENT)
        hip.wrf_scores(self.P, self.jobs, self.conv, src0=self.s0.source, src1=self.s1.source, pts=self.pts.view.view(-1),
                       out=out.view)
        torch.cuda.synchronize()
        assert out.untouched()
        return out.view.cpu()


@pytest.mark.parametrize("J", [1, 3, 40])
@pytest.mark.parametrize("P", [1, 255, 256, 257, 120, 8064])
def test_wrf_scores_contract(hip, W, P, J):
    case = ScoreCase(hip, W, P, J)
    got = case.run(hip)
    again = case.run(hip)
    assert same_bits(got, again), "two runs must give the same bits"
    g = got.numpy()
    for j in range(J):
        check_stats(g[j], case.want[j], case.mag[j], P, f"job {j}")
    if J >= 3:
        assert g[1, 0] == 0 and (g[1] == 0).all(), "an all-NaN job gives n = 0 and empty sums"
        assert not np.isfinite(g[2, 4]) or not np.isfinite(g[2, 5]), "an inf stays in the sums"
    if P >= 255:
        assert 0 < g[0, 0] < P, "the first job masks some points and keeps others"


def test_wrf_scores_float64_point_fields(hip):
    P = 300
    rng = np.random.default_rng(4)
    a = rng.standard_normal(P)
    b = (a + 0.1 * rng.standard_normal(P)).astype(np.float32)
    a[::17] = np.nan
    got = hip.wrf_scores(P, [(hip.WRF_POINT64, 0, hip.WRF_POINT, 0, 0, 0)], [(1.0, 0.0, 1.0, 0.0)],
                         pts=torch.from_numpy(b).to(DEV), pts64=torch.from_numpy(a).to(DEV)).cpu().numpy()[0]
    want, mag = six(a, b.astype(np.float64))
    check_stats(got, want, mag, P, "float64 against float32")


def test_wrf_scores_slots_accumulate_and_gate(hip, W):
    """Three samples x two slots: slot 0 adds every sample in sample order onto the state, slot 1 is gated on the
    sample offset and takes the first sample at target + delta only - also across calls."""
    P = 130
    rng = np.random.default_rng(9)
    pts = rng.standard_normal((6, P)).astype(np.float32)
    ref = rng.standard_normal(P).astype(np.float32)
    arena = torch.from_numpy(np.concatenate([pts.reshape(-1), ref])).to(DEV)
    jobs, conv = [], []
    for b in range(3):
        jobs += [(hip.WRF_POINT, (2 * b) * P, hip.WRF_POINT, 6 * P, 0, 0),
                 (hip.WRF_POINT, (2 * b + 1) * P, hip.WRF_POINT, 6 * P, 1, -1)]
        conv += [(1.0, 0.0, 1.0, 0.0)] * 2
    state = torch.zeros(2, 6, dtype=torch.float64, device=DEV)
    state[0, 1] = 5.0
    filled = torch.zeros(2, dtype=torch.int32, device=DEV)
    offsets = torch.tensor([4, 6, 6], dtype=torch.int64, device=DEV)  # target 7, delta -1: samples 1 and 2 qualify
    hip.wrf_scores(P, jobs, conv, pts=arena, slots=2, offsets=offsets, target=7, filled=filled, accumulate=True,
                   out=state)
    got = state.cpu().numpy()
    want0 = sum(six(pts[2 * b].astype(np.float64), ref.astype(np.float64))[0] for b in range(3))
    want0[1] += 5.0
    assert got[0, 0] == 3 * P and np.allclose(got[0], want0, rtol=1e-13, atol=1e-12)
    want1 = six(pts[3].astype(np.float64), ref.astype(np.float64))[0]
    assert got[1, 0] == P and np.allclose(got[1], want1, rtol=1e-13, atol=1e-12)
    assert filled.cpu().tolist() == [0, 1]
    hip.wrf_scores(P, jobs, conv, pts=arena, slots=2, offsets=offsets, target=7, filled=filled, accumulate=True,
                   out=state)
    again = state.cpu().numpy()
    assert again[0, 0] == 6 * P and same_bits(torch.from_numpy(again[1]), torch.from_numpy(got[1]))
    with pytest.raises(ValueError):
        hip.wrf_scores(P, jobs, conv, pts=arena, slots=4)
    with pytest.raises(ValueError):
        hip.wrf_scores(P, jobs, conv, pts=arena, slots=2)  # gated jobs without offsets
    with pytest.raises(ValueError):
        hip.wrf_scores(P, [(hip.WRF_POINT, 6 * P + 1, hip.WRF_POINT, 0, 0, 0)], conv[:1], pts=arena)


# ----------------------------------------------------------------------------------------------------------------------
# gcl_wrf_box_means
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [7, 28])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [1, 6, 45])
def test_wrf_box_means_contract(hip, R, B, K):
    G, C = 61, 7
    rng = np.random.default_rng(100 * R + 10 * B + K)
    x = rng.standard_normal((B, G, K)).astype(np.float32)
    mean, std = WC.scalers()
    mean, std = mean[:C].copy(), std[:C].copy()
    rows = rng.permutation(G)[:R].astype(np.int32)  # out of order
    xs = Rows.of(torch.from_numpy(x).to(DEV), "pad_nan", NAN)
    out = Guarded((B, K), torch.float32, SENT)
    hip.wrf_box_means(xs.view, torch.from_numpy(rows).to(DEV), G, torch.from_numpy(std).to(DEV),
                      torch.from_numpy(mean).to(DEV), out=out.view)
    torch.cuda.synchronize()
    phys = x.reshape(B, G, K // C, C) * std[None, None, None, :] + mean[None, None, None, :]
    want = phys[:, rows].mean(axis=1).reshape(B, K)
    assert want.dtype == np.float32
    assert same_bits(out.view.cpu(), torch.from_numpy(want))
    assert out.untouched()
    again = hip.wrf_box_means(xs.view, torch.from_numpy(rows).to(DEV), G, torch.from_numpy(std).to(DEV),
                              torch.from_numpy(mean).to(DEV))
    assert same_bits(out.view, again), "two runs must give the same bits"


def test_wrf_box_means_appends_at_the_device_count(hip):
    G, C, K, B = 40, 7, 28, 3
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((B, G, K)).astype(np.float32)).to(DEV)
    mean, std = (torch.from_numpy(a[:C].copy()).to(DEV) for a in WC.scalers())
    rows = torch.from_numpy(rng.permutation(G)[:9].astype(np.int32)).to(DEV)
    alone = hip.wrf_box_means(x, rows, G, std, mean)
    state = Guarded((5, K), torch.float32, SENT)
    count = torch.tensor([1], dtype=torch.int64, device=DEV)
    hip.wrf_box_means(x, rows, G, std, mean, out=state.view, count=count)
    assert same_bits(state.view[1:4], alone) and bool((state.view[0] == SENT).all()) and bool((state.view[4] == SENT).all())
    count.fill_(3)  # two rows fit, the third is dropped
    hip.wrf_box_means(x, rows, G, std, mean, out=state.view, count=count)
    assert same_bits(state.view[3:5], alone[:2]) and state.untouched()
    with pytest.raises(ValueError, match="empty row list"):
        hip.wrf_box_means(x, rows[:0], G, std, mean)
    with pytest.raises(ValueError, match="outside"):
        hip.wrf_box_means(x, torch.tensor([0, G], dtype=torch.int32, device=DEV), G, std, mean)
    with pytest.raises(ValueError):
        hip.wrf_box_means(x, rows, G + 1, std, mean)
