"""The dataset kernels (csrc/dataset.hip) called through their thin hip.py wrappers, entry point by entry point.

Rules:
  fp16 bytes   equal numpy's ndarray.astype(np.float16) of the float32 product x * float32(scale), bit for bit (NaN: any
               NaN).  Everything a call must not write - the rows before and after the block, the guard halves around
               the series, the unlisted channels - keeps its bytes.
  sums         against math.fsum (exact) of the same float32 values / float32 squares: |s - exact| <= (N - 1) 2^-53
               sum|x|, the a-priori bound of ANY order of N float64 additions, so nothing is measured.  Bit-equal where
               every partial sum is exact (small whole numbers), bit-equal from run to run, NaN / inf as numpy.
  welford      bit-equal to the reference's welford_update after every block (tests/golden/dataset_vectors.npz).
  widen        byte-equal to the reference's add_time_features data.npy.
  stats        counts and min / max exact under every flag setting; sums by the rule above.
Shapes are the smallest that reach each path: one point; 35 points with odd t0 (1330 B per step: the span starts off
any 16-byte boundary); 2501 (61 x 41, five tiles, the last partial); 4096; more tiles than blocks (2100 steps); Ct of 1,
2, 8, 19 and 23; and one series of more than 2^31 halves.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import dataset_case as DC  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = np.float16(-7.25)
SENT = -7.25


@pytest.fixture(scope="module")
def H(lib_built):
    from graphcast_lite_amd import hip

    return hip


@pytest.fixture(scope="module")
def gv():
    return DC.golden()


class Series:
    """A contiguous fp16 series of `shape` inside a buffer with `guard` sentinel halves either side, filled with the
    sentinel (or the given bits)."""

    def __init__(self, shape, guard=8, init=None):
        n = math.prod(shape)
        self.guard, self.n = guard, n
        self.buf = torch.full((n + 2 * guard,), float(SENT16), dtype=torch.float16, device=DEV)
        self.view = self.buf[guard:guard + n].view(shape)
        if init is not None:
            self.view.copy_(torch.from_numpy(init).to(DEV))

    def host(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:self.guard] == SENT16).all() and (b[self.guard + self.n:] == SENT16).all()


def same_f16(a, b):
    """Bit-equal, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and (a.view(np.uint16)[~nan] == b.view(np.uint16)[~nan]).all()


def planes_for(rng, nsrc, nt, P, static=()):
    """Float32 planes of mixed magnitudes ([nt, P], or [P] for the static ones) and their factors."""
    mags = [1.0, 1e5, 300.0, 1e-6, 2e4, 0.05, 7.0, 6e4]
    planes, scales = [], []
    for j in range(nsrc):
        x = rng.standard_normal(P if j in static else (nt, P)) * mags[j % 8] * 0.1 + mags[j % 8]
        planes.append(x.astype(np.float32))
        scales.append([1.0, 0.01, 1.0, 1.0, 1 / 9.80665, 1.0, 3.0, 1.0][j % 8])
    return planes, scales


def expect(plane, scale, nt):
    """(v float32 [nt, P], its fp16) as numpy forms them."""
    v = plane * np.float32(scale)
    assert v.dtype == np.float32
    v = np.broadcast_to(v, (nt, v.shape[-1])) if v.ndim == 1 else v
    with np.errstate(over="ignore"):
        return v, v.astype(np.float16)


def check_sum(got, values, what):
    """|got - fsum(values)| <= (N - 1) 2^-53 sum|values| (float32 values widened exactly to float64)."""
    x = values.astype(np.float64).ravel()
    exact = math.fsum(x)
    bound = (x.size - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
    assert abs(got - exact) <= bound, f"{what}: got {got!r}, exact {exact!r}, bound {bound:.3e}"


def run_pack(H, planes, chans, scales, nt, grid, Ct, series, t0):
    sums = torch.full((Ct,), SENT, dtype=torch.float64, device=DEV)
    sumsq = torch.full((Ct,), SENT, dtype=torch.float64, device=DEV)
    H.dataset_pack([torch.from_numpy(p).to(DEV) for p in planes], chans, scales, nt, series, t0, sums, sumsq,
                   grid=(grid[0], grid[1], Ct))
    return sums.cpu().numpy(), sumsq.cpu().numpy()


FULL = [  # (n_lon, n_lat), Ct, nt, t0, T, guard
    ((1, 1), 1, 1, 0, 1, 8),
    ((1, 1), 19, 3, 1, 5, 8),
    ((7, 5), 19, 3, 1, 5, 8),       # 1330 B per step, odd t0
    ((7, 5), 23, 17, 3, 21, 5),     # base 10 B past a 16-byte boundary
    ((7, 5), 2, 2100, 1, 2102, 8),  # more tiles than blocks: a block walks several
    ((61, 41), 19, 3, 1, 5, 8),
    ((61, 41), 23, 1, 2, 4, 3),
    ((64, 64), 8, 17, 0, 17, 8),
    ((4096, 1), 19, 3, 2, 6, 8),    # the flat (T, N, Ct) layout
]


@gpu
@pytest.mark.parametrize("grid,Ct,nt,t0,T,guard", FULL, ids=lambda v: str(v).replace(" ", ""))
def test_pack_all_channels(H, grid, Ct, nt, t0, T, guard):
    """Every channel listed (in a shuffled order, one source time-invariant): the block's bytes, its surroundings and
    both sums."""
    P = grid[0] * grid[1]
    rng = np.random.default_rng(P * 100 + Ct)
    chans = [int(c) for c in rng.permutation(Ct)]
    static = (Ct // 2,) if Ct > 1 else ()
    planes, scales = planes_for(rng, Ct, nt, P, static)
    ser = Series((T, P, Ct) if grid[1] == 1 else (T, grid[0], grid[1], Ct), guard)
    sums, sumsq = run_pack(H, planes, chans, scales, nt, grid, Ct, ser.view, t0)
    got = ser.host().reshape(T, P, Ct)
    for j, c in enumerate(chans):
        v, h = expect(planes[j], scales[j], nt)
        assert same_f16(got[t0:t0 + nt, :, c], h), f"channel {c}"
        check_sum(sums[c], v, f"sum of channel {c}")
        check_sum(sumsq[c], v * v, f"sumsq of channel {c}")
    assert (got[:t0] == SENT16).all() and (got[t0 + nt:] == SENT16).all() and ser.guards_intact()


def rounding_plane():
    """For every finite fp16 value and its successor: the float32 midpoint and its two float32 neighbours; the fp16
    values themselves (subnormals, +-0 included); around the overflow threshold 65520; beyond it; below half the
    smallest subnormal."""
    bits = np.arange(0x7C00, dtype=np.uint16)  # +0 .. 65504
    a = bits.view(np.float16).astype(np.float32)
    b = np.append(a[1:], np.float32(65536.0))  # the successor of 65504 in an unbounded fp16
    mid = (a + b) / np.float32(2)
    assert ((mid.astype(np.float64) - a) == (b.astype(np.float64) - mid)).all()  # the midpoints are float32 numbers
    pos = np.concatenate([a, mid, np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(np.inf)),
                          np.array([65519.0, 65536.0, 1e5, 3e38, 2.0 ** -25, 2.0 ** -26, 1e-45], dtype=np.float32)])
    return np.concatenate([pos, -pos]).astype(np.float32)


@gpu
def test_pack_rounds_like_astype(H):
    x = rounding_plane()
    special = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    ser = Series((1, x.size + 3, 1))
    sums, sumsq = run_pack(H, [np.concatenate([x, special])[None]], [0], [1.0], 1, (x.size + 3, 1), 1, ser.view, 0)
    with np.errstate(over="ignore"):
        want = np.concatenate([x, special]).astype(np.float16)
    got = ser.host().ravel()
    assert same_f16(got, want)
    assert np.isinf(want[:x.size]).sum() >= 10 and (want[:x.size] == 0).sum() >= 8  # overflow and underflow both met
    assert np.isnan(sums[0]) and np.isnan(sumsq[0]) and ser.guards_intact()
    # without the NaN: +inf and -inf in the sum give NaN, in the sum of squares +inf, as numpy has it
    s2, q2 = run_pack(H, [np.concatenate([x, special[1:]])[None]], [0], [1.0], 1, (x.size + 2, 1), 1, None, 0)
    assert np.isnan(s2[0]) and q2[0] == np.inf
    s3, q3 = run_pack(H, [np.abs(x)[None]], [0], [1.0], 1, (x.size, 1), 1, None, 0)
    with np.errstate(over="ignore"):
        sq = np.abs(x) * np.abs(x)
    assert np.isfinite(s3[0]) and q3[0] == np.inf == sq.sum(dtype=np.float64)  # 3e38^2 overflows float32 first
    check_sum(s3[0], np.abs(x), "sum of the rounding plane")


@gpu
@pytest.mark.parametrize("grid,Ct,chans", [((7, 5), 19, [3, 7, 5]), ((61, 41), 23, [22, 0, 9, 10]), ((1, 1), 2, [1]),
                                           ((64, 64), 8, [2])], ids=["35x19", "2501x23", "1x2", "4096x8"])
def test_pack_some_channels_leave_the_rest(H, grid, Ct, chans):
    """The repair case: the listed columns are rewritten, every other byte of the series (random bit patterns, NaNs
    among them) and every other entry of the sums stay."""
    P, T, t0, nt = grid[0] * grid[1], 6, 1, 3
    rng = np.random.default_rng(P + Ct)
    before = rng.integers(0, 1 << 16, (T, P, Ct)).astype(np.uint16).view(np.float16)
    planes, scales = planes_for(rng, len(chans), nt, P, static=(0,))
    ser = Series((T, grid[0], grid[1], Ct), init=before.reshape(T, grid[0], grid[1], Ct))
    sums, sumsq = run_pack(H, planes, chans, scales, nt, grid, Ct, ser.view, t0)
    want = before.copy()
    for j, c in enumerate(chans):
        v, h = expect(planes[j], scales[j], nt)
        want[t0:t0 + nt, :, c] = h
        check_sum(sums[c], v, f"sum of channel {c}")
        check_sum(sumsq[c], v * v, f"sumsq of channel {c}")
    assert (ser.host().reshape(T, P, Ct).view(np.uint16) == want.view(np.uint16)).all() and ser.guards_intact()
    rest = [c for c in range(Ct) if c not in chans]
    assert (sums[rest] == SENT).all() and (sumsq[rest] == SENT).all()


@gpu
def test_pack_sums_alone_repeatable_and_exact_on_whole_numbers(H):
    """series == NULL gives the sums of the packing call, bit for bit; twice the same call, the same bits; on small
    whole numbers (every partial sum exact) the exact sums."""
    grid, Ct, nt = (61, 41), 19, 17
    P = 2501
    rng = np.random.default_rng(3)
    planes, scales = planes_for(rng, Ct, nt, P)
    chans = list(range(Ct))
    ser = Series((nt, 61, 41, Ct))
    a = run_pack(H, planes, chans, scales, nt, grid, Ct, ser.view, 0)
    b = run_pack(H, planes, chans, scales, nt, grid, Ct, None, 0)
    c = run_pack(H, planes, chans, scales, nt, grid, Ct, None, 0)
    for x, y in zip(a + b, b + c):
        assert x.tobytes() == y.tobytes()
    ints = [rng.integers(-300, 300, (nt, P)).astype(np.float32) for _ in range(3)]
    s, q = run_pack(H, ints, [0, 1, 2], [1.0, 2.0, 1.0], nt, grid, 3, None, 0)
    for j, f in enumerate([1, 2, 1]):
        x = ints[j].astype(np.int64) * f
        assert s[j] == float(x.sum()) and q[j] == float((x * x).sum())


def finish(mean, m2, n):
    std = np.maximum(np.sqrt(m2 / max(n, 1)), 1e-6)
    return mean.astype(np.float32), std.astype(np.float32)


@gpu
def test_constant_channel_is_bit_equal_floor_included(H, gv):
    """The fixture's second build (lsm = 1.0 everywhere): sums only, block by block, merged on the device; the host's
    sqrt, floor and casts give the reference's mean and std of that channel bit for bit - the std is the 1e-6 floor."""
    f = {n: DC.const_field(n) for n in DC.CONST_VARS}
    mean, m2 = (torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2))
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    s, q = (torch.zeros(2, dtype=torch.float64, device=DEV) for _ in range(2))
    for a in range(0, DC.CONST_T, DC.CONST_CHUNK):
        e = min(a + DC.CONST_CHUNK, DC.CONST_T)
        src = [torch.from_numpy(f["t2m"][a:e].reshape(e - a, 35)).to(DEV), torch.from_numpy(f["lsm"].reshape(35)).to(DEV)]
        H.dataset_pack(src, [0, 1], [1.0, 1.0], e - a, None, 0, s, q, grid=(7, 5, 2))
        H.dataset_welford(mean, m2, n, s, q, (e - a) * 35)
    assert int(n) == int(gv["const_n"])
    m, sd = finish(mean.cpu().numpy(), m2.cpu().numpy(), int(n))
    assert m[1] == gv["const_mean"][1] == 1.0 and sd[1] == gv["const_std"][1] == np.float32(1e-6)
    assert float(m2[1]) == 0.0
    assert abs(float(m[0]) - float(gv["const_mean"][0])) <= DC.ulp32(gv["const_mean"][0])


@gpu
def test_welford_equals_the_reference_after_every_block(H, gv):
    mean, m2 = (torch.zeros(5, dtype=torch.float64, device=DEV) for _ in range(2))
    n = torch.zeros(1, dtype=torch.int64, device=DEV)
    for k, (bs, bq, bn) in enumerate(DC.welford_blocks()):
        H.dataset_welford(mean, m2, n, torch.from_numpy(bs).to(DEV), torch.from_numpy(bq).to(DEV), bn)
        assert mean.cpu().numpy().tobytes() == gv["welford_mean"][k].tobytes(), f"mean after block {k}"
        assert m2.cpu().numpy().tobytes() == gv["welford_m2"][k].tobytes(), f"m2 after block {k}"
        assert int(n) == int(gv["welford_n"][k])
    # NaN block statistics stay NaN through np.maximum(block_var, 0.0)
    bad = torch.tensor([float("nan")] * 5, dtype=torch.float64, device=DEV)
    H.dataset_welford(mean, m2, n, bad, bad, 7)
    assert bool(mean.isnan().all()) and bool(m2.isnan().all()) and int(n) == int(gv["welford_n"][-1]) + 7


@gpu
def test_widen_equals_the_reference(H, gv):
    src = Series((DC.T, DC.N_LON, DC.N_LAT, 19), init=gv["data"])
    dst = Series((DC.T, DC.N_LON, DC.N_LAT, 23), guard=5)
    extra = torch.from_numpy(gv["tf"].astype(np.float16)).to(DEV)
    H.dataset_widen(src.view, extra, out=dst.view)
    assert dst.host().tobytes() == gv["wide_data"].tobytes() and dst.guards_intact()
    assert src.host().tobytes() == gv["data"].tobytes()


@gpu
@pytest.mark.parametrize("shape,K", [((3, 61, 41, 19), 4), ((2, 4096, 1), 1), ((5, 1, 1, 2), 3), ((3, 64, 64, 8), 15)],
                         ids=["2501x19+4", "flat4096x1+1", "1x2+3", "4096x8+15"])
def test_widen_moves_bits(H, shape, K):
    """Random bit patterns (NaN payloads included) arrive unchanged; the new channels are extra[t] at every point."""
    rng = np.random.default_rng(shape[1] + K)
    a = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    ex = rng.integers(0, 1 << 16, (shape[0], K)).astype(np.uint16)
    src = Series(shape, guard=3, init=a.view(np.float16))
    dst = Series(shape[:-1] + (shape[-1] + K,), guard=8)
    H.dataset_widen(src.view, torch.from_numpy(ex.view(np.float16)).to(DEV), out=dst.view)
    got = dst.host().view(np.uint16)
    want = np.concatenate([a, np.broadcast_to(ex.reshape((shape[0],) + (1,) * (len(shape) - 2) + (K,)),
                                              shape[:-1] + (K,))], axis=-1)
    assert (got == want).all() and dst.guards_intact()


def stats_case(shape, seed):
    """fp16 data with NaN, +inf and -inf sprinkled in; channel 0 gets none, channel 1 (if any) only +inf."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(shape) * 50).astype(np.float16)
    r = rng.random(shape)
    x[r < 0.02] = np.nan
    x[(r >= 0.02) & (r < 0.04)] = np.inf
    x[(r >= 0.04) & (r < 0.05)] = -np.inf
    x[..., 0] = np.where(np.isfinite(x[..., 0]), x[..., 0], np.float16(1.5))
    if shape[-1] > 1:
        x[..., 1] = np.where(np.isnan(x[..., 1]) | (x[..., 1] == -np.inf), np.float16(-2.0), x[..., 1])
    return x


@gpu
@pytest.mark.parametrize("shape,t_s,t_e", [((5, 7, 5, 19), 1, 4), ((5, 7, 5, 19), 0, 5), ((4, 61, 41, 23), 1, 3),
                                           ((3, 1, 1, 1), 0, 3), ((4, 1, 1, 2), 1, 2), ((60, 4096, 19), 0, 60),
                                           ((6, 64, 64, 8), 2, 5)],
                         ids=["35x19-odd", "35x19-all", "2501x23", "1x1", "1x2", "flat4096x19-long", "4096x8"])
def test_stats(H, shape, t_s, t_e):
    """Counts and min / max exact whatever the flags; the sums of flags 3 within the a-priori bound of the values with
    the non-finite ones zeroed; with flags 0 NaN / inf reach the sums as numpy's sum has them.  The span of the odd case
    starts off a 16-byte boundary (the 2-byte loads), the others on one (the 16-byte loads); the long case gives a
    block several chunks."""
    x = stats_case(shape, shape[1] + shape[-1])
    Ct = shape[-1]
    ser = Series(shape, init=x)
    rows = x[t_s:t_e].reshape(-1, Ct).astype(np.float32)
    fin = np.isfinite(rows)
    big = np.float32(np.inf)
    want_min = np.where(fin, rows, big).min(axis=0)
    want_max = np.where(fin, rows, -big).max(axis=0)
    for flags in (0, 1, 2, 3):
        s, q, mn, mx, nn, ni = (t.cpu().numpy() for t in H.dataset_stats(ser.view, t_s, t_e, flags))
        assert (nn == np.isnan(rows).sum(axis=0)).all() and (ni == np.isinf(rows).sum(axis=0)).all(), flags
        assert (mn == want_min).all() and (mx == want_max).all() and mn.dtype == np.float32, flags
        v = rows.copy()
        if flags & 1:
            v[np.isnan(rows)] = 0
        if flags & 2:
            v[np.isinf(rows)] = 0
        with np.errstate(invalid="ignore"):
            ref_s, ref_q = v.sum(axis=0, dtype=np.float64), (v * v).sum(axis=0, dtype=np.float64)
        for c in range(Ct):
            if np.isfinite(ref_s[c]) and np.isfinite(v[:, c]).all():
                check_sum(s[c], v[:, c], f"flags {flags} sum of channel {c}")
                check_sum(q[c], v[:, c] * v[:, c], f"flags {flags} sumsq of channel {c}")
            else:
                assert (np.isnan(s[c]) and np.isnan(ref_s[c])) or s[c] == ref_s[c], (flags, c)
                assert (np.isnan(q[c]) and np.isnan(ref_q[c])) or q[c] == ref_q[c], (flags, c)
    assert ser.host().view(np.uint16).tobytes() == x.view(np.uint16).tobytes()
    again = H.dataset_stats(ser.view, t_s, t_e, 3)
    assert again[0].cpu().numpy().tobytes() == s.tobytes() and again[1].cpu().numpy().tobytes() == q.tobytes()


@gpu
def test_offsets_beyond_2_31(H):
    """A series of 27 597 x 4096 x 19 halves (4.3 GB, 2^31 + 225 280 elements), never initialised: pack three steps at
    its end, check them and the sentinel row before them, read nothing else."""
    T, P, Ct, nt = 27597, 4096, 19, 3
    assert T * P * Ct > 2 ** 31 > (T - nt) * P * Ct  # the block straddles element 2^31
    series = torch.empty(T, 64, 64, Ct, dtype=torch.float16, device=DEV)
    series[T - nt - 1].fill_(float(SENT16))
    rng = np.random.default_rng(31)
    planes, scales = planes_for(rng, Ct, nt, P, static=(4,))
    chans = [int(c) for c in rng.permutation(Ct)]
    sums, sumsq = run_pack(H, planes, chans, scales, nt, (64, 64), Ct, series, T - nt)
    got = series[T - nt:].cpu().numpy().reshape(nt, P, Ct)
    for j, c in enumerate(chans):
        v, h = expect(planes[j], scales[j], nt)
        assert same_f16(got[:, :, c], h), f"channel {c}"
        check_sum(sums[c], v, f"sum of channel {c}")
    assert bool((series[T - nt - 1] == float(SENT16)).all())
    s = H.dataset_stats(series, T - nt, T, 3)[0].cpu().numpy()
    for c in range(Ct):
        check_sum(s[c], got[:, :, c].astype(np.float32), f"stats sum of channel {c}")
    # one channel rewritten in the last step alone: the partial pack's 64-bit offsets
    one = (rng.standard_normal((1, P)) * 3).astype(np.float32)
    run_pack(H, [one], [7], [1.0], 1, (64, 64), Ct, series, T - 1)
    last = series[T - 1].cpu().numpy().reshape(P, Ct)
    assert same_f16(last[:, 7], one[0].astype(np.float16)) and same_f16(last[:, 8], got[2, :, 8])
    assert bool((series[T - nt - 1] == float(SENT16)).all())
    del series
    torch.cuda.empty_cache()


# ---- validation: returns before any HIP call, so no GPU is needed ----------------------------------------------------
def test_validation_without_gpu(lib_built):
    L = lib_built
    buf = (C.c_double * 64)()
    p = C.addressof(buf)
    ws_bytes = L.gcl_dataset_ws_bytes(19)
    assert ws_bytes >= 2048 * 19 * 6 * 8 and L.gcl_dataset_ws_bytes(1) >= 2048 * 32 * 2 * 8
    assert L.gcl_dataset_max_sources() == 32

    def pack(nsrc=2, nt=3, grid=(7, 5), T=10, Ct=19, t0=1, chans=(0, 1), strides=(35, 0), src=None, series=p, ws=p,
             wsb=ws_bytes, sums=p):
        n = max(len(chans), 1)
        srcs = (C.c_void_p * n)(*(src if src is not None else [p] * n))
        return L.gcl_dataset_pack(srcs, (C.c_int64 * n)(*strides), (C.c_int32 * n)(*chans), (C.c_float * n)(*[1.0] * n),
                                  nsrc, nt, grid[0], grid[1], series, T, Ct, t0, sums, p, ws, wsb, None)

    def err():
        return L.gcl_last_error().decode()

    assert pack(nsrc=0) == -1 and "sources" in err()
    assert pack(nsrc=33) == -1 and "sources" in err()
    assert pack(t0=8) == -1 and "rows [8, 11) of 10" in err()
    assert pack(t0=-1) == -1 and pack(nt=0) == -1 and pack(grid=(0, 5)) == -1 and pack(Ct=0) == -1
    assert pack(chans=(0, 19)) == -1 and "channel 19 of 19" in err()
    assert pack(chans=(4, 4)) == -1 and "listed twice" in err()
    assert pack(strides=(34, 0)) == -1 and "time stride" in err()
    assert pack(src=[p, None]) == -1 and "source 1 is null" in err()
    assert pack(sums=None) == -1 and "null" in err()
    assert pack(wsb=8) == -1 and "workspace" in err()
    assert pack(series=p + 1) == -1 and "aligned" in err()

    def stats(T=10, grid=(7, 5), Ct=19, t_s=0, t_e=10, flags=3, series=p, wsb=ws_bytes):
        return L.gcl_dataset_stats(series, T, grid[0], grid[1], Ct, t_s, t_e, flags, p, p, p, p, p, p, p, wsb, None)

    assert stats(t_s=5, t_e=5) == -1 and "rows [5, 5) of 10" in err()
    assert stats(t_e=11) == -1 and stats(t_s=-1) == -1 and stats(Ct=257) == -1 and stats(series=None) == -1
    assert stats(flags=4) == -1 and "flag" in err()
    assert stats(wsb=100) == -1 and "workspace" in err()
    assert L.gcl_dataset_welford(p, p, p, p, p, 0, 5, None) == -1 and "block_n=0" in err()
    assert L.gcl_dataset_welford(p, p, p, p, p, 10, 0, None) == -1 and L.gcl_dataset_welford(p, p, None, p, p, 10, 5, None) == -1
    assert L.gcl_dataset_widen(p, 10, 7, 5, 19, p, 19, p + 64, None) == -1 and "19 -> 19" in err()
    assert L.gcl_dataset_widen(p, 10, 7, 5, 19, p, 23, p, None) == -1 and "in place" in err()
    assert L.gcl_dataset_widen(p, 0, 7, 5, 19, p, 23, p + 64, None) == -1
    assert L.gcl_dataset_widen(p, 10, 7, 5, 19, None, 23, p + 64, None) == -1 and "null" in err()
