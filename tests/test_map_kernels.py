"""The error-map kernels (csrc/maps.hip) called directly through their hip.py wrappers, on operands laid out by
tests/helpers/layouts.py (NaN around every input, the sentinel around every output), against restatements written here
from the formulas in the kernel file's header comment.  Nothing here imports verify.py.

Rules:
  maps_colstats    against torch.mean / torch.std (float64) of the converted float32 values: the mean to
                   n 2^-52 max|x|, the std to 1e-9 max(1, std) under the first-row condition of stat_columns (the
                   derivation is in test_scoring_kernels.colstats_ref); n = 1 gives a NaN std on both sides, a constant
                   column a std of exactly 0
  maps_accumulate  every way out of the `flat` gate runs the generic kernel and is bit-equal to the flat kernel on a
                   contiguous copy of the same data; the state agrees with a float64 restatement of add_sample summed in
                   sample order to (samples added) 2^-52 of the sum of the absolute terms; count is exact
  maps_finalize    float64 arithmetic rounded once: bit-equal to numpy
  maps_convert     bit-equal to numpy float32 with a true division by float32(9.80665)
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, Guarded, Rows, Worst, has, launched, same_bits, targs  # noqa: E402
from stat_columns import GMAX, KS, NS, columns, deviates, first_row_within_4_sigma, row_list  # noqa: E402

gpu = pytest.mark.gpu
E52 = 2.0 ** -52
G0 = np.float32(9.80665)
W = Worst("map kernels")


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(scope="module")
def pool(lib_built):
    return deviates(GMAX).to(DEV)


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# Unit conversion: maps.hip's header, float32, one rounding per operation
# ------------------------------------------------------------------------------------------------------------------
def conv_table(K, seed, flag0=0):
    """conv float32 [K, 4] = {scale, mean, factor, offset} and flags int32 [K] that walk through 0, 1, 2, 3."""
    rng = np.random.default_rng(seed)
    conv = np.stack([rng.random(K) * 5 + 0.5, rng.standard_normal(K) * 100, rng.random(K) * 2 + 0.01,
                     rng.standard_normal(K) * 10], 1).astype(np.float32)
    return conv, ((np.arange(K) + flag0) % 4).astype(np.int32)


def to_units_np(x, conv, flags):
    """x [..., K] float32 in numpy: v = x scale; v = v + mean (flag 1); v = v / 9.80665f (flag 2); v = v factor;
    v = v + offset."""
    assert x.dtype == np.float32 and conv.dtype == np.float32
    v = x
    v = np.where(flags & 1, v * conv[:, 0] + conv[:, 1], v)
    v = np.where(flags & 2, v / G0, v)
    v = v * conv[:, 2] + conv[:, 3]
    assert v.dtype == np.float32
    return v


def to_units(x, conv, flags):
    """The same in torch, on x's device.  The division goes through float64: a float64 quotient of two float32 values
    rounded to float32 is the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits), whatever the device's own
    float32 division does; `test_to_units_restatements_agree` holds it to numpy's division on the CPU."""
    if conv is None:
        return x
    conv, flags = torch.as_tensor(conv, device=x.device), torch.as_tensor(flags, device=x.device)
    v = torch.where((flags & 1) != 0, x * conv[:, 0] + conv[:, 1], x)
    v = torch.where((flags & 2) != 0, (v.double() / float(G0)).float(), v)
    return v * conv[:, 2] + conv[:, 3]


def test_to_units_restatements_agree():
    """CPU: the torch restatement used for the large cases is bit-equal to the numpy one (true float32 division)."""
    rng = np.random.default_rng(0)
    for K in (1, 4, 19, 33):
        for flag0 in range(4):
            conv, flags = conv_table(K, K, flag0)
            x = (rng.standard_normal((4001, K)) * 300).astype(np.float32)
            a, b = to_units_np(x, conv, flags), to_units(torch.from_numpy(x), conv, flags)
            assert np.array_equal(a.view(np.int32), b.numpy().view(np.int32))


# ------------------------------------------------------------------------------------------------------------------
# maps_colstats
# ------------------------------------------------------------------------------------------------------------------
def colstats_ref(t, p, rows):
    """[B, K, 4] = {mean_p, std_p, mean_t, std_t}: torch.mean / torch.std (unbiased) in float64 of the converted
    values; asserts the first-row condition."""
    sel = (lambda x: x[:, rows.long()]) if rows is not None else (lambda x: x)
    T, P = sel(t).double(), sel(p).double()
    assert first_row_within_4_sigma(T) and first_row_within_4_sigma(P), "first scored row beyond 4 sigma"
    amax = torch.stack([P.abs().amax(1), T.abs().amax(1)], -1)
    return torch.stack([P.mean(1), P.std(1), T.mean(1), T.std(1)], -1), amax


class ColCase:
    """Truth on padded rows; the prediction on an odd row stride or, with `use_map`, wider and through a column map
    (a permutation with a repeat); unscored rows NaN; conversion with every flag, or none."""

    def __init__(self, z, n, K, B, use_rows, use_map, use_conv, seed):
        g = torch.Generator().manual_seed(seed)
        G = n + 5 if use_rows else n
        self.rows, first = None, 0
        if use_rows:
            r = row_list(n, g)
            self.rows, first = i32(r), int(r[0])
        t, preds = columns(z[:, :B, :G], first)
        Wm = K + 3
        self.pmap = None
        if use_map:
            m = torch.randperm(Wm, generator=g)[:K]
            if K > 1:
                m[K - 1] = m[0]
            self.pmap = i32(m)
        self.conv = self.flags = None
        conv = flags = None
        if use_conv:
            conv, flags = conv_table(K, seed, flag0=seed % 4)
            self.conv, self.flags = torch.from_numpy(conv).to(DEV), i32(flags)
        self.T = Rows.of(t[..., :K], "pad_nan", NAN)
        self.P = Rows.of(preds[0][..., :Wm], "colblock", NAN) if use_map else Rows.of(preds[0][..., :K], "odd_ld", NAN)
        if use_rows:
            unscored = torch.ones(G, dtype=torch.bool, device=DEV)
            unscored[self.rows.long()] = False
            self.T.view[:, unscored] = NAN
            self.P.view[:, unscored] = NAN
        p = preds[0][..., self.pmap.long()] if use_map else preds[0][..., :K]
        self.n, self.K, self.B = n, K, B
        self.ref, self.amax = colstats_ref(to_units(t[..., :K], conv, flags), to_units(p, conv, flags), self.rows)

    def run(self, hip):
        out = Guarded((self.B, self.K, 4), torch.float64)
        hip.maps_colstats(self.T.view, self.P.view, self.pmap, self.rows, self.conv, self.flags, out.view)
        torch.cuda.synchronize()
        assert out.untouched(), "maps_colstats wrote outside cs"
        return out.view

    def check(self, cs, what):
        W.within("colstats mean", cs[..., 0::2], self.ref[..., 0::2], self.n * E52 * self.amax, f"{what}: mean")
        got, ref = cs[..., 1::2], self.ref[..., 1::2]
        if self.n == 1:
            assert bool(torch.isnan(got).all()) and bool(torch.isnan(ref).all()), f"{what}: std of one row is NaN"
            return
        W.within("colstats std", got, ref, 1e-9 * ref.clamp_min(1.0), f"{what}: std")
        const = torch.arange(self.K, device=DEV) % 3 == 2
        assert bool((cs[:, const, 3] == 0).all()), f"{what}: std of a constant truth column is not exactly 0"


@gpu
@pytest.mark.parametrize("n", NS)
def test_maps_colstats(hip, pool, n):
    """Every K at this n, B alternating between 1 and 3, with and without a row list, a column map and a conversion
    (K = 19: 19 columns x 3 chunks per block; K = 33: 32 columns x 2 chunks)."""
    i = NS.index(n)
    for iK, K in enumerate(KS):
        for v in range(8):
            B = (1, 3)[(i + iK + v) % 2]
            case = ColCase(pool, n, K, B, bool(v & 1), bool(v & 2), bool(v & 4), seed=1000 * i + 10 * iK + v)
            case.check(case.run(hip), f"n={n} K={K} B={B} rows/map/conv={v:03b}")
    W.report("colstats mean", "colstats std")


@gpu
def test_maps_colstats_column_alone(hip, pool):
    """A column's result depends on its own data and n, never on K: same bits alone and inside K = 33."""
    for n in (65, 32769):
        case = ColCase(pool, n, 33, 3, True, False, False, seed=n)
        full = case.run(hip)
        for k in (0, 19, 32):
            alone = Guarded((3, 1, 4), torch.float64)
            hip.maps_colstats(case.T.view[:, :, k:k + 1], case.P.view[:, :, k:k + 1], None, case.rows, None, None,
                              alone.view)
            assert same_bits(alone.view, full[:, k:k + 1]), f"n={n}: column {k} alone differs"


# ------------------------------------------------------------------------------------------------------------------
# maps_accumulate
# ------------------------------------------------------------------------------------------------------------------
def accumulate_ref(state, tol, vt, vp, cs, sums, C):
    """add_sample (maps.hip) in float64 torch, summed in sample order into state [leads, nsums, n * C]; vt, vp the
    converted float32 values [B, n, K]; tol collects the sum of the absolute terms."""
    B, n, K = vt.shape
    leads = K // C

    def plane(x):  # [n, K] -> [leads, n * C]
        return x.view(n, leads, C).permute(1, 0, 2).reshape(leads, n * C)
    for b in range(B):
        dp, dt = vp[b].double(), vt[b].double()
        e = dp - dt
        terms = [e, e * e, e.abs()]
        if sums & 8:
            terms.append(((dp - cs[b, :, 0]) / (cs[b, :, 1] + 1e-8)) * ((dt - cs[b, :, 2]) / (cs[b, :, 3] + 1e-8)))
        p = 0
        for slot in range(4):
            if sums & (1 << slot):
                state[:, p] += plane(terms[slot])
                tol[:, p] += plane(terms[slot].abs())
                p += 1


def strided(src, off, bs_extra, ld_extra=0):
    """src [B, n, K] as a view `off` floats into a NaN buffer, rows ld_extra and samples bs_extra floats apart."""
    B, n, K = src.shape
    ld = K + ld_extra
    bs = n * ld + bs_extra
    buf = torch.full((off + B * bs + 4,), NAN, device=DEV)
    v = torch.as_strided(buf, (B, n, K), (bs, ld, 1), off)
    v.copy_(src)
    return v


class AccCase:
    """Truth and prediction [B, n, leads * C] (float32, ordinary columns and columns far from zero), a conversion
    table, the kernel's own column statistics, and two batches for the two updates."""

    def __init__(self, hip, n, leads, C, B, seed):
        g = torch.Generator().manual_seed(seed)
        K = leads * C
        self.n, self.leads, self.C, self.B, self.K = n, leads, C, B, K
        far = (torch.arange(K) % 3 == 1).float() * 1e3
        self.t = [(torch.randn(B, n, K, generator=g) * 3 + far).to(DEV) for _ in range(2)]
        self.p = [(t.cpu() + torch.randn(B, n, K, generator=g)).to(DEV) for t in self.t]
        self.conv_np, self.flags_np = conv_table(K, seed, seed % 4)
        self.conv, self.flags = torch.from_numpy(self.conv_np).to(DEV), i32(self.flags_np)
        self.cs = []
        for t, p in zip(self.t, self.p):
            cs = torch.empty(B, K, 4, dtype=torch.float64, device=DEV)
            hip.maps_colstats(t, p, None, None, self.conv, self.flags, cs)
            self.cs.append(cs)

    def run(self, hip, sums, view_t, view_p, pmap=None, rows=None, state0=None):
        """Two updates into one sentinel-guarded state (from state0, or from a random one), operands as view_t / view_p
        lay them out; the kernels the first update launched, and the state."""
        if state0 is None:
            g = torch.Generator().manual_seed(sums)
            state0 = torch.randn(self.leads, bin(sums).count("1"), self.n * self.C, generator=g, dtype=torch.float64).to(DEV)
        self.state0 = state0
        st = Guarded(tuple(state0.shape), torch.float64, init=state0)
        count = torch.full((3,), 40, dtype=torch.int64, device=DEV)

        def update(u):
            hip.maps_accumulate(view_t(self.t[u]), view_p(self.p[u]), pmap, rows, self.conv, self.flags,
                                self.cs[u] if sums & 8 else None, sums, self.C, st.view, count[1:2])
        _, names = launched(lambda: update(0))
        update(1)
        torch.cuda.synchronize()
        assert st.untouched(), "maps_accumulate wrote outside the state"
        assert count.tolist() == [40, 40 + 2 * self.B, 40], "count is not exact"
        return names, st.view

    def check(self, state, sums, what):
        ref = self.state0.clone()
        tol = self.state0.abs()
        for u in range(2):
            accumulate_ref(ref, tol, to_units(self.t[u], self.conv_np, self.flags_np),
                           to_units(self.p[u], self.conv_np, self.flags_np), self.cs[u], sums, self.C)
        W.within("accumulate", state, ref, 2 * self.B * E52 * tol, what)


FLAT = "maps_accumulate_flat_kernel"
GENERIC = "maps_accumulate_kernel"


@gpu
@pytest.mark.parametrize("leads,C,B,cslds", [(1, 19, 1, True), (1, 19, 4, True), (1, 64, 5, False), (3, 19, 4, True),
                                             (3, 19, 5, False), (3, 5, 1, True)])
def test_maps_accumulate_flat(hip, leads, C, B, cslds):
    """The four <VSTATE, CSLDS> instances (one lead or three; a statistics table of 32 B K bytes below and above 8 KB),
    all 15 sets of sums, B around the four samples whose loads are issued together."""
    case = AccCase(hip, 8, leads, C, B, seed=leads * 100 + C + B)
    assert (32 * B * leads * C <= 8192) == cslds
    for sums in range(1, 16):
        names, state = case.run(hip, sums, lambda x: x, lambda x: x)
        assert has(names, FLAT) and not has(names, GENERIC), names
        want = ["true" if leads == 1 else "false", "true" if cslds and sums & 8 else "false"]
        assert targs(names, FLAT) == [want], (targs(names, FLAT), want)
        case.check(state, sums, f"flat leads={leads} C={C} B={B} sums={sums}")
    W.report("accumulate")


@gpu
@pytest.mark.parametrize("way", ["rows", "pmap", "ld", "nK", "base", "bs"])
@pytest.mark.parametrize("leads", [1, 3])
def test_maps_accumulate_generic(hip, way, leads):
    """One case for each way out of the `flat` gate, everything else as the flat kernel wants it: the generic kernel
    runs, agrees with float64, and is bit-equal to the flat kernel on a contiguous copy of the same data (for
    n K % 4 != 0: of the same rows followed by one more)."""
    n, C, B = (3, 5, 1) if way == "nK" else (8, 19, 5)
    case = AccCase(hip, n, leads, C, B, seed=leads + len(way))
    K = leads * C
    g = torch.Generator().manual_seed(3)
    rows = pmap = None

    def plain(x):
        return strided(x, 0, 0)
    view_t = view_p = plain
    if way == "rows":  # unsorted, not from row 0 (none twice: the copy below scatters the rows to their places)
        r = 2 + torch.randperm(n + 3, generator=g)[:n]
        rows = i32(r)

        def view_t(x):
            f = torch.full((B, n + 5, K), NAN, device=DEV)
            f[:, r.to(DEV)] = x
            return f
        view_p = view_t
    elif way == "pmap":  # a permutation of the K columns: the rows stay K floats long
        m = torch.randperm(K, generator=g)
        pmap = i32(m)

        def view_p(x):
            f = torch.empty_like(x)
            f[:, :, m.to(DEV)] = x
            return f
    elif way == "ld":
        def view_t(x):
            return strided(x, 0, 0, ld_extra=4)
    elif way == "nK":
        assert n * K % 4 != 0
    elif way == "base":
        def view_p(x):
            return strided(x, 1, 0)
    elif way == "bs":
        assert n * K % 4 == 0 and B > 1

        def view_t(x):
            return strided(x, 0, 2)
    n2 = n if n * K % 4 == 0 else n + 1

    def grown(x):
        f = torch.zeros(B, n2, K, device=DEV)
        f[:, :n] = x
        return f
    for sums in (15, 5, 2):
        names, state = case.run(hip, sums, view_t, view_p, pmap, rows)
        assert has(names, GENERIC) and not has(names, FLAT), names
        case.check(state, sums, f"{way} leads={leads} sums={sums}")
        start = torch.zeros(leads, state.shape[1], n2 * C, dtype=torch.float64, device=DEV)
        start[:, :, :n * C] = case.state0
        names, flat = case.run(hip, sums, grown, grown, state0=start)
        assert has(names, FLAT) and not has(names, GENERIC), names
        assert same_bits(flat[:, :, :n * C], state), f"{way} leads={leads} sums={sums}: generic and flat kernels differ"
    W.report("accumulate")


# ------------------------------------------------------------------------------------------------------------------
# maps_finalize, maps_convert
# ------------------------------------------------------------------------------------------------------------------
def finalize_ref(v, n, kind, rv=None, rn=0):
    """maps.hip's finalize: float64 arithmetic rounded once to float32 (twice for skill: the two RMSEs, then the ratio)."""
    if kind == 4:
        r = np.sqrt(v / n).astype(np.float32) if n > 0 else np.zeros(v.shape, np.float32)
        rr = np.sqrt(rv / rn).astype(np.float32) if rn > 0 else np.zeros(v.shape, np.float32)
        return (1.0 - r.astype(np.float64) / np.maximum(rr.astype(np.float64), 1e-9)).astype(np.float32)
    if n <= 0:
        return np.zeros(v.shape, np.float32)
    return (np.sqrt(v / n) if kind == 0 else v / n).astype(np.float32)


@gpu
@pytest.mark.parametrize("nsums", [1, 2, 3, 4])
@pytest.mark.parametrize("count", [0, 7])
def test_maps_finalize(hip, nsums, count):
    """Every kind from every plane of 1 to 4 sums, leads * nE = 105 elements; skill against a reference state with
    zeros (the 1e-9 floor) and with a zero count."""
    rng = np.random.default_rng(nsums + count)
    leads, nE = 3, 35
    state = rng.standard_normal((leads, nsums, nE)) * 50
    rstate = np.abs(rng.standard_normal((leads, 2, nE))) * 50
    rstate[:, 1, ::4] = 0.0
    S, R = torch.from_numpy(state).to(DEV), torch.from_numpy(rstate).to(DEV)
    Sa = S.abs()
    cnt = torch.tensor([count], dtype=torch.int64, device=DEV)
    for plane in range(nsums):
        for kind in range(5):
            for rcount in ((0, 5) if kind == 4 else (0,)):
                src = Sa if kind in (0, 4) else S
                out = Guarded((leads, nE))
                hip.maps_finalize(src, cnt, plane, kind, out.view, R if kind == 4 else None,
                                  torch.tensor([rcount], dtype=torch.int64, device=DEV) if kind == 4 else None, 1)
                torch.cuda.synchronize()
                v = (np.abs(state) if kind in (0, 4) else state)[:, plane]
                ref = finalize_ref(v, count, kind, rstate[:, 1], rcount)
                assert out.untouched()
                assert same_bits(out.view, torch.from_numpy(ref).to(DEV)), (plane, kind, rcount)
    W.exact("finalize / convert (bit-equal)")


@gpu
@pytest.mark.parametrize("K", [1, 4, 19, 33])
def test_maps_convert(hip, K):
    rng = np.random.default_rng(K)
    rows = 4001 if K == 1 else 301  # rows * K is no multiple of 256
    assert rows * K % 256 != 0
    for flag0 in range(4):
        conv, flags = conv_table(K, K, flag0)
        x = (rng.standard_normal((rows, K)) * 300).astype(np.float32)
        X = Rows.of(torch.from_numpy(x), "contig", NAN)
        got = hip.maps_convert(X.view, torch.from_numpy(conv).to(DEV), i32(flags))
        ref = to_units_np(x, conv, flags)
        assert same_bits(got, torch.from_numpy(ref).to(DEV)), f"K={K} flags from {flag0}"
