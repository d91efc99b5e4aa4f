"""The downscaler kernels (csrc/downscale.hip) called through their thin hip.py wrappers, entry point by entry point,
against float64 / float32 numpy restatements written here.

Rules:
  fp16 outputs  bit-equal to numpy (NaN: any NaN).  coarse: the four corner values widened to float64, each product
                rounded alone, added in corner order onto 0.0, ndarray.astype(np.float16) of that float64 (ONE
                rounding).  pred: the same sum rounded to float32, * std, + mean in float32, then fp16.  Everything a
                call must not write - the frames before and after, the frames of a skipped sample, the guard halves
                around the archive - keeps its bytes.
  batch         bit-equal to the numpy expression of DownscalerDataset.__getitem__.
  pair_mse      against math.fsum (exact) of the float64 squares of the float32 differences: |s - exact| <=
                (N - 1) 2^-53 sum|x|, the a-priori bound of ANY order of N float64 additions; bit-equal run to run.
Shapes are the smallest that reach each path: one point; 35 points x 19 channels with an odd frame offset and an odd
guard (no span is 16-byte aligned); 2501 points (61 x 41: several tiles, the last partial) with C of 1, 5, 19 and 23;
one frame; more tiles than launched blocks (2100 frames / samples of 3 points, for pred with skipped destinations in a
block's first and in its second trip); and 104 frames / samples of 2501 points, where the launch takes its largest
tiles (512 points; a launch of few frames takes tiles down to 32 to fill the device).  One batch has more items than
the largest launch has blocks.  Every output - archives, X, Y and the statistics - lies between guard elements.
"""
import math

import numpy as np
import pytest
import torch

# the four wrappers under test, reached below through the `H` fixture once the library is built
from graphcast_lite_amd.hip import downscale_batch, downscale_coarse, downscale_pair_mse, downscale_pred  # noqa: F401

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENT16 = np.float16(-7.25)
MAGS = [280.0, 3.0, 3.0, 900.0, 0.002, 3e-6, 6e4, 40.0]  # 3e-6: fp16 subnormals; 6e4: sums that overflow fp16


@pytest.fixture(scope="module")
def H(lib_built):
    from graphcast_lite_amd import hip

    return hip


class Archive:
    """A contiguous array of `shape` (fp16: an archive; float32 / float64: the outputs of batch and pair_mse) inside a
    buffer with `guard` sentinel elements either side.  The sentinel -7.25 is exact in all three formats."""

    def __init__(self, shape, guard=8, dtype=torch.float16):
        n = math.prod(shape)
        self.guard, self.n = guard, n
        self.buf = torch.full((n + 2 * guard,), float(SENT16), dtype=dtype, device=DEV)
        self.view = self.buf[guard:guard + n].view(shape)

    def host(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:self.guard] == SENT16).all() and (b[self.guard + self.n:] == SENT16).all()


def same(a, b):
    """Bit-equal, except that any NaN equals any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    bits = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a)
    return (nan == np.isnan(b)).all() and (a.view(bits)[~nan] == b.view(bits)[~nan]).all()


def series_for(rng, T, N, C):
    x = rng.standard_normal((T, N, C)) * 0.1 + 1.0
    x = x * np.array([MAGS[c % len(MAGS)] for c in range(C)])
    with np.errstate(over="ignore"):
        return x.astype(np.float16)


def table_for(rng, P, N):
    """Positions anywhere in the source, weights of interpolation and of extrapolation (-0.72 .. 1.85), and a point
    exactly on the last node (weights 0, 0, 0, 1) in the last row."""
    pos = rng.integers(0, N, size=(P, 4)).astype(np.int32)
    y = rng.uniform(-0.85, 1.0, size=(P, 2))
    w = np.stack([(1 - y[:, 0]) * (1 - y[:, 1]), (1 - y[:, 0]) * y[:, 1], y[:, 0] * (1 - y[:, 1]), y[:, 0] * y[:, 1]], 1)
    w[-1] = [0.0, 0.0, 0.0, 1.0]
    return pos, w


def corner_sum(v, w):
    """v float64 [..., P, 4, C], w [P, 4]: every product rounded on its own, added in corner order onto 0.0."""
    acc = np.zeros(v.shape[:-2] + v.shape[-1:])
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(4):
            acc = acc + v[..., m, :] * w[:, m, None]
    return acc


def coarse_ref(series, pos, w, t0, nt):
    v = series[t0:t0 + nt].astype(np.float64)[:, pos, :]
    with np.errstate(over="ignore"):
        return corner_sum(v, w).astype(np.float16)


def up(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


COARSE = [  # N, P, C, T, t0, nt, T_out, to0, guard
    (4, 1, 1, 1, 0, 1, 1, 0, 8),
    (30, 1, 19, 3, 1, 1, 3, 2, 3),
    (12 * 7, 35, 19, 5, 1, 3, 5, 1, 5),      # 1330 B per frame, odd offset, odd guard
    (21 * 14, 2501, 1, 3, 0, 2, 2, 0, 8),
    (21 * 14, 2501, 5, 3, 1, 2, 4, 1, 7),
    (21 * 14, 2501, 19, 2, 1, 1, 3, 1, 8),
    (21 * 14, 2501, 23, 2, 0, 2, 3, 1, 1),
    (6, 3, 2, 2101, 1, 2100, 2102, 1, 8),    # more tiles than launched blocks: a block walks several
    (21 * 14, 2501, 19, 105, 1, 104, 105, 1, 3),  # enough frames for tiles of 512 points (a short launch takes smaller)
]


@gpu
@pytest.mark.parametrize("case", COARSE, ids=lambda c: "N{}_P{}_C{}_nt{}".format(c[0], c[1], c[2], c[5]))
def test_coarse_bit_equal_and_bounded(H, case):
    N, P, C, T, t0, nt, T_out, to0, guard = case
    rng = np.random.default_rng(P * 131 + C)
    series = series_for(rng, T, N, C)
    pos, w = table_for(rng, P, N)
    out = Archive((T_out, P, C), guard)
    H.downscale_coarse(up(series), up(pos), up(w), t0, nt, out.view, to0)
    got = out.host()
    assert same(got[to0:to0 + nt], coarse_ref(series, pos, w, t0, nt))
    assert (got[:to0] == SENT16).all() and (got[to0 + nt:] == SENT16).all() and out.guards_intact()


@gpu
def test_coarse_special_values(H):
    """A zero-weight corner holding inf gives NaN (0 x inf, as scipy computes it); sums beyond 65504 give +-inf; tiny
    sums give fp16 subnormals; -0.0 products add onto +0.0."""
    vals = np.array([np.inf, -np.inf, 60000.0, -60000.0, 1.0, 6e-8, 3e-7, -0.0, 0.0, 2.0], dtype=np.float16)
    series = vals.reshape(1, -1, 1)
    rows = [([0, 4, 4, 4], [0.0, 0.5, 0.25, 0.25]),      # 0 * inf -> NaN
            ([1, 4, 4, 4], [0.0, 1.0, 0.0, 0.0]),        # 0 * -inf -> NaN
            ([0, 1, 4, 4], [0.5, 0.5, 0.0, 0.0]),        # inf - inf -> NaN
            ([2, 2, 4, 4], [0.6, 0.6, 0.0, 0.0]),        # 72000 -> inf
            ([3, 2, 3, 4], [1.85, -0.72, 0.3, 0.0]),     # -> -inf
            ([2, 4, 4, 4], [1.0916, 0.0, 0.0, 0.0]),     # 65496: below the midpoint 65520 -> 65504
            ([9, 4, 4, 4], [32760.0, 0.0, 0.0, 0.0]),    # 65520 exactly: the midpoint, tie to even -> inf
            ([5, 5, 6, 6], [0.5, 0.25, 0.5, -0.1]),      # subnormal
            ([5, 4, 4, 4], [0.4, 0.0, 0.0, 0.0]),        # 2.4e-8: below half the smallest subnormal -> 0
            ([5, 4, 4, 4], [-0.6, 0.0, 0.0, 0.0]),       # -> -(smallest subnormal)
            ([7, 7, 7, 7], [1.0, 1.0, 1.0, 1.0]),        # 0.0 + -0.0 ... -> +0.0
            ([8, 4, 9, 4], [0.0, 0.0, 0.0, 0.0])]
    pos = np.array([r[0] for r in rows], dtype=np.int32)
    w = np.array([r[1] for r in rows], dtype=np.float64)
    ref = coarse_ref(series, pos, w, 0, 1)
    assert np.isnan(ref[0, :3, 0]).all() and ref[0, 3, 0] == np.inf and ref[0, 4, 0] == -np.inf
    assert ref[0, 5, 0] == 65504 and ref[0, 6, 0] == np.inf and 0 < ref[0, 7, 0] < 6.2e-5 and ref[0, 8, 0] == 0
    assert ref[0, 9, 0] == -np.float16(6e-8) and not np.signbit(ref[0, 10, 0])
    out = Archive((1, len(rows), 1))
    H.downscale_coarse(up(series), up(pos), up(w), 0, 1, out.view, 0)
    assert same(out.host(), ref) and out.guards_intact()


def double_rounding_rows(rng, want=64):
    """float64 values d whose direct rounding to binary16 differs from the rounding through float32, found by search:
    just off the midpoint of two neighbouring halves, by less than float32 resolves."""
    found = []
    while len(found) < want:
        h = np.float16(rng.uniform(-1, 1) * 10.0 ** rng.uniform(-6, 4))
        nxt = np.nextafter(h, np.float16(np.inf))
        if not (np.isfinite(h) and np.isfinite(nxt)):
            continue
        mid = (float(h) + float(nxt)) / 2
        d = mid * (1 + rng.choice([-1, 1]) * 2.0 ** -rng.integers(27, 50))
        with np.errstate(over="ignore"):
            if np.float64(d).astype(np.float16) != np.float64(d).astype(np.float32).astype(np.float16):
                found.append(d)
    return np.array(found)


@gpu
def test_coarse_rounds_float64_to_half_once(H):
    d = double_rounding_rows(np.random.default_rng(5))
    assert len(d) >= 8
    # one corner holds 1.0 with weight d: the float64 sum is d itself
    series = np.array([1.0, 0.0], dtype=np.float16).reshape(1, 2, 1)
    pos = np.tile(np.array([[0, 1, 1, 1]], dtype=np.int32), (len(d), 1))
    w = np.zeros((len(d), 4))
    w[:, 0] = d
    direct = d.astype(np.float16)
    two_step = d.astype(np.float32).astype(np.float16)
    assert (direct != two_step).all()
    out = Archive((1, len(d), 1))
    H.downscale_coarse(up(series), up(pos), up(w), 0, 1, out.view, 0)
    assert same(out.host().ravel(), direct)


@gpu
@pytest.mark.parametrize("shape", [(3, 35, 19), (2, 2501, 23), (5, 1, 1)], ids=str)
def test_coarse_copy_moves_bits(H, shape):
    T, N, C = shape
    rng = np.random.default_rng(N)
    bits = rng.integers(0, 1 << 16, size=shape, dtype=np.uint16)  # NaN payloads and all
    out = Archive((T + 1, N, C), guard=3)
    H.downscale_coarse(up(bits.view(np.int16)).view(torch.float16), None, None, 1 if T > 1 else 0, T - 1 if T > 1 else 1, out.view, 1)
    got = out.view.view(torch.int16).cpu().numpy().view(np.uint16)
    src = bits[1:] if T > 1 else bits
    assert (got[1:1 + len(src)] == src).all() and out.guards_intact()
    assert (out.host()[:1] == SENT16).all() and (out.host()[1 + len(src):] == SENT16).all()


# ---- pred ------------------------------------------------------------------------------------------------------------
def pred_ref(pred, last, pos, w, std, mean):
    v = pred if last is None else last + pred
    assert v.dtype == np.float32
    acc = corner_sum(v.astype(np.float64)[:, pos, :], w)
    with np.errstate(over="ignore", invalid="ignore"):
        f = acc.astype(np.float32)
        f = f * std + mean
        assert f.dtype == np.float32
        return f.astype(np.float16)


PRED = [  # G, P, C, B, pad (extra columns: gs > C), with last, guard
    (4, 1, 1, 1, 0, False, 8),
    (84, 35, 19, 3, 0, True, 5),
    (84, 35, 19, 3, 7, False, 3),
    (294, 2501, 5, 2, 3, True, 7),
    (294, 2501, 19, 2, 19, True, 8),   # the obs-window layout: last and pred side by side
    (294, 2501, 23, 1, 0, False, 1),
    (294, 2501, 1, 2, 0, True, 8),
    (294, 2501, 19, 104, 0, True, 5),  # enough samples for tiles of 512 points
    (6, 3, 2, 2100, 0, True, 8),       # 2102 (sample, tile) items against 2048 blocks: blocks 0 .. 53 take two
    (6, 3, 2, 2100, 1, False, 3),
]
# Samples of the rows above whose destination lies outside the archive, besides samples 0 and 1 of every row.  With
# one tile per sample, block k takes sample k and then sample 2048 + k: blocks 0 and 1 skip their first sample and
# store their second, blocks 2, 12 and 13 store their first and skip their second (-1, T_out, -1), and the blocks
# between and after store both - into the LDS stage the first trip left behind.
LATE_SKIPS = {2050: -1, 2060: None, 2061: -1}  # None: T_out


@gpu
@pytest.mark.parametrize("case", PRED, ids=lambda c: "G{}_P{}_C{}_B{}_pad{}_{}".format(*c[:5], "res" if c[5] else "abs"))
def test_pred_bit_equal_and_skips(H, case):
    G, P, C, B, pad, with_last, guard = case
    rng = np.random.default_rng(P * 17 + C + pad)
    full = rng.standard_normal((B + 2, G, C + pad)).astype(np.float32)
    full[2, :, 0] = np.inf
    lastf = (rng.standard_normal((B + 2, G, C + pad)) * 0.5).astype(np.float32)
    mean = np.array([MAGS[c % 5] for c in range(C)], dtype=np.float32)
    std = (mean * 0.07 + 1e-4).astype(np.float32)
    pos, w = table_for(rng, P, G)
    T_out = 2 * B + 1
    dest = np.array([T_out, -1] + [T_out - 1 - 2 * i for i in range(B)], dtype=np.int64)  # the first two skip
    skipped = {0, 1}
    for b, d in LATE_SKIPS.items():
        if b < B + 2:
            dest[b] = T_out if d is None else d
            skipped.add(b)
    assert len(skipped) == (5 if B + 2 > 2048 else 2)
    out = Archive((T_out, P, C), guard)
    dfull, dlast = up(full), up(lastf)
    H.downscale_pred(dfull[:, :, :C], up(pos), up(w), up(std), up(mean), up(dest), out.view,
                     last3=dlast[:, :, pad:pad + C] if with_last else None)
    got = out.host()
    ref = pred_ref(full[:, :, :C], lastf[:, :, pad:pad + C] if with_last else None, pos, w, std, mean)
    written = set()
    for b in range(B + 2):
        if b in skipped:
            continue
        assert same(got[dest[b]], ref[b]), f"sample {b}"
        written.add(int(dest[b]))
    for t in range(T_out):
        assert t in written or (got[t] == SENT16).all(), f"frame {t} was written"
    assert out.guards_intact()


# ---- batch -----------------------------------------------------------------------------------------------------------
def batch_ref(coarse, fine, t, obs, mean, std, static, flip, neg, noise, sigma):
    """DownscalerDataset.__getitem__ in numpy, sample by sample."""
    T, W, Hh, C = coarse.shape
    norm = lambda x: (x - mean) / (std + np.float32(1e-8))  # noqa: E731
    Xs, Ys = [], []
    for b, tb in enumerate(t):
        frames = [norm(coarse[tb - obs + 1 + i].astype(np.float32)).transpose(1, 0, 2) for i in range(obs)]
        X = np.concatenate(frames, axis=-1).transpose(2, 0, 1).copy()
        Y = norm(fine[tb].astype(np.float32)).transpose(1, 0, 2).transpose(2, 0, 1).copy()
        assert X.dtype == np.float32 and Y.dtype == np.float32
        if static is not None:
            X = np.concatenate([X, static.transpose(1, 0, 2).transpose(2, 0, 1)], axis=0)
        if flip is not None and flip[b]:
            X, Y = X[:, :, ::-1].copy(), Y[:, :, ::-1].copy()
            for ch in neg:
                for i in range(obs):
                    X[i * C + ch] = -X[i * C + ch]
                Y[ch] = -Y[ch]
        if noise is not None:
            X[:obs * C] = X[:obs * C] + noise[b] * np.float32(sigma)
        Xs.append(X), Ys.append(Y)
    return np.stack(Xs), np.stack(Ys)


BATCH = [  # H, W, C, obs, Ns, B, flips, noise
    (1, 1, 1, 1, 0, 1, False, False),
    (1, 1, 5, 2, 2, 2, True, True),
    (7, 9, 5, 2, 2, 3, True, False),
    (7, 9, 19, 3, 0, 2, True, True),
    (41, 61, 19, 2, 2, 3, True, True),
    (41, 61, 5, 1, 0, 2, False, False),
    (41, 61, 23, 3, 2, 1, True, False),
    (1, 1, 2, 1, 2, 21900, True, True),  # 3 items per sample: 65700 against the 65536 blocks of the largest launch
]


@gpu
@pytest.mark.parametrize("case", BATCH, ids=lambda c: "{}x{}_C{}_obs{}_Ns{}_B{}{}{}".format(
    *c[:6], "_flip" if c[6] else "", "_noise" if c[7] else ""))
def test_batch_bit_equal(H, case):
    Hh, W, C, obs, Ns, B, flips, noisy = case
    rng = np.random.default_rng(Hh * 100 + C * 7 + obs)
    T = obs + 3
    coarse = series_for(rng, T, W * Hh, C).reshape(T, W, Hh, C)
    fine = series_for(rng, T, W * Hh, C).reshape(T, W, Hh, C)
    coarse[0, 0, 0, 0] = np.nan
    mean = np.array([MAGS[c % len(MAGS)] for c in range(C)], dtype=np.float32)
    std = (0.1 * mean).astype(np.float32)
    std[0] = 0.0  # std + 1e-8 is what divides
    t = np.array([obs - 1 + (2 * b) % 4 for b in range(B)], dtype=np.int64)
    static = rng.standard_normal((W, Hh, Ns)).astype(np.float32) if Ns else None
    flip = np.array([(b + 1) % 2 for b in range(B)], dtype=np.int32) if flips else None
    neg = [1, C - 1] if C > 2 else [0]
    negmask = np.zeros(C, dtype=np.int32)
    negmask[neg] = 1
    noise = rng.standard_normal((B, obs * C, Hh, W)).astype(np.float32) if noisy else None
    sigma = 0.05
    X = Archive((B, obs * C + Ns, Hh, W), 5, torch.float32)
    Y = Archive((B, C, Hh, W), 3, torch.float32)
    H.downscale_batch(up(coarse), up(fine), up(t), obs, up(mean), up(std), static=None if static is None else up(static),
                      flip=None if flip is None else up(flip), neg=up(negmask) if flips else None,
                      noise=None if noise is None else up(noise), sigma=sigma, out=(X.view, Y.view))
    with np.errstate(all="ignore"):
        Xr, Yr = batch_ref(coarse, fine, t, obs, mean, std, static, flip, neg, noise, sigma)
    assert same(X.host(), Xr) and same(Y.host(), Yr)
    assert X.guards_intact() and Y.guards_intact()


@gpu
def test_batch_leaves_a_sample_outside_the_archive_untouched(H):
    rng = np.random.default_rng(3)
    coarse = series_for(rng, 4, 12, 5).reshape(4, 4, 3, 5)
    mean, std = np.ones(5, dtype=np.float32), np.ones(5, dtype=np.float32)
    t = np.array([0, 2, 4], dtype=np.int64)  # obs 2: frame -1 for the first, frame 4 of 4 for the last
    X = torch.full((3, 10, 3, 4), -7.25, device=DEV)
    Y = torch.full((3, 5, 3, 4), -7.25, device=DEV)
    H.downscale_batch(up(coarse), up(coarse), up(t), 2, up(mean), up(std), out=(X, Y))
    Xr, Yr = batch_ref(coarse, coarse, t[1:2], 2, mean, std, None, None, [], None, 0.0)
    assert same(X[1:2].cpu().numpy(), Xr) and same(Y[1:2].cpu().numpy(), Yr)
    assert (X[[0, 2]] == -7.25).all() and (Y[[0, 2]] == -7.25).all()


# ---- pair mse --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(3, 1, 1), (6, 35, 19), (5, 2501, 5), (4, 2501, 23), (40, 63, 255)], ids=str)
def test_pair_mse_bounded_and_reproducible(H, shape):
    T, P, C = shape
    rng = np.random.default_rng(P + C)
    a, b = series_for(rng, T, P, C), series_for(rng, T, P, C)
    a[~np.isfinite(a)] = 1.0
    b[~np.isfinite(b)] = 2.0
    mean = np.array([MAGS[c % len(MAGS)] for c in range(C)], dtype=np.float32)
    std = (0.1 * mean).astype(np.float32)
    t = np.array([T - 1, -1, 0, T, T - 1] + list(range(T)), dtype=np.int64)  # two outside, one listed thrice
    da, db, dt, dm, ds = up(a), up(b), up(t), up(mean), up(std)
    stats = [Archive((C, 2), g, torch.float64) for g in (1, 4)]
    for s in stats:
        H.downscale_pair_mse(da, db, dt, dm, ds, out=s.view)
    got, again = stats[0].host(), stats[1].host()
    assert got.tobytes() == again.tobytes() and stats[0].guards_intact() and stats[1].guards_intact()
    tv = t[(t >= 0) & (t < T)]
    norm = lambda x: (x.astype(np.float32) - mean) / (std + np.float32(1e-8))  # noqa: E731
    d = norm(a[tv]) - norm(b[tv])
    assert d.dtype == np.float32
    sq = d.astype(np.float64) ** 2
    for c in range(C):
        x = sq[..., c].ravel()
        exact = math.fsum(x)
        bound = (x.size - 1) * 2.0 ** -53 * exact
        assert got[c, 0] == x.size
        assert abs(got[c, 1] - exact) <= bound, f"channel {c}: got {got[c, 1]!r}, exact {exact!r}, bound {bound:.3e}"


# ---- argument validation (no GPU: every check returns before the first HIP call) -------------------------------------
def test_argument_validation_without_gpu(lib_built):
    L, p = lib_built, 64  # p: a non-null address that is never read

    def err():
        return L.gcl_last_error().decode()

    assert L.gcl_downscale_pred(p, 10, 5, None, 0, 0, None, None, 7, 5, 1, p, p, p, p, 3, None) == -1
    assert "null point table (P=7)" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, 5, p, None, 7, 0, 1, p + 64, 2, 0, None) == -1
    assert "go together" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, 5, None, None, 7, 0, 1, p + 64, 2, 0, None) == -1
    assert "whole frames" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, 5, p, p, -7, 0, 1, p + 64, 2, 0, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, 5, p, p, 7, 1, 2, p + 64, 3, 0, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, -5, p, p, 7, 0, 1, p + 64, 2, 0, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_coarse(p, 2, 6, 5, p, p, 7, 0, 1, p + 65, 2, 0, None) == -1 and "2-byte aligned" in err()
    assert L.gcl_downscale_pred(p, 10, 4, None, 0, 0, p, p, 7, 5, 1, p, p, p, p, 3, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_pred(p, 10, 5, None, 0, 0, p, p, 7, 5, -1, p, p, p, p, 3, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_batch(p, p, 4, -3, 3, 5, p, 1, 2, p, p, None, 0, None, None, None, 0.0, p, p, None) == -1
    assert "bad shape" in err()
    assert L.gcl_downscale_batch(p, p, 4, 3, 3, 65, p, 1, 2, p, p, None, 0, None, None, None, 0.0, p, p, None) == -1
    assert "(1 .. 64)" in err()
    assert L.gcl_downscale_batch(p, p, 4, 3, 3, 5, p, 1, 2, p, p, None, 2, None, None, None, 0.0, p, p, None) == -1
    assert "static" in err()
    assert L.gcl_downscale_batch(p, p, 4, 3, 3, 5, p, 1, 2, p, None, None, 0, None, None, None, 0.0, p, p, None) == -1
    assert "null argument" in err()
    need = L.gcl_downscale_ws_bytes(19)
    assert need >= 19 * 2 * 8 and L.gcl_downscale_ws_bytes(0) > 0
    assert L.gcl_downscale_pair_mse(p, p, 4, 35, 19, p, 2, p, p, p, p, 8, None) == -1 and "too small" in err()
    assert L.gcl_downscale_pair_mse(p, p, 4, 35, 19, p, 0, p, p, p, p, need, None) == -1 and "bad shape" in err()
    assert L.gcl_downscale_pair_mse(p, p, 4, 35, 19, p, 2, p, p, p, None, need, None) == -1 and "null argument" in err()
