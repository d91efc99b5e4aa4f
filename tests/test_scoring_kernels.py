"""The forecast-scoring kernels (csrc/verify.hip) and the evaluation glue (csrc/pipeline.hip) called directly through their
hip.py wrappers, on operands laid out by tests/helpers/layouts.py (NaN around every input, the sentinel around every
output), at the sizes where a chunk, a tile, a row lane or a lane count runs out, against float64 / float32
restatements written here from the formulas in the kernel files' header comments.  Nothing here imports verify.py or
pipeline.py.

Rules:
  verify_colstats    se, ae (sums of non-negative float64 terms) to n 2^-52 relative; corr to 1e-9 absolute under the
                     first-row condition (see `colstats_ref`); a constant column's corr exactly 0; a column has the same
                     bits alone and inside K = 33, as B = 1 and as sample 2 of B = 3
  verify_accumulate  bit-equal to a float64 loop in the kernel's documented order
  regrid / taper     bit-equal to numpy (float64 in the stated order rounded once; the blend float32, one rounding per
                     operation)
  pipeline_sqerr     float32 difference and square, float64 sums: to G 2^-52 relative (S 2^-52 for more stations than
                     rows); other horizons' slots keep their bits
  pipeline glue      bit-equal to numpy in the rounding order the kernel header states
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, Guarded, Rows, Worst, launched, same_bits, targs  # noqa: E402
from stat_columns import GMAX, KS, NS, WMAX, columns, deviates, first_row_within_4_sigma, row_list  # noqa: E402

gpu = pytest.mark.gpu
E52 = 2.0 ** -52
W = Worst("scoring kernels")


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------------------------
# verify_colstats
# ------------------------------------------------------------------------------------------------------------------
PRED_LAYOUTS = ["odd_ld", "pad_nan", "colblock", "offset"]  # predictions 1 and 3 go through a column map


@pytest.fixture(scope="module")
def pool(lib_built):
    return deviates(GMAX).to(DEV)


def colstats_ref(t, preds, rows):
    """Two-pass float64 statistics [B, npred, K, 3] of truth t [B, G, K] and predictions [B, G, K] over `rows`.

    Asserts the condition the corr bound rests on: the first scored row x_0 of every column lies within 4 sigma of the
    column's mean.  The kernel sums x' = x - x_0 in one pass and forms sum x'^2 - (sum x')^2 / n = n sigma^2 out of
    sum x'^2 = n sigma^2 + n (x_0 - mean)^2 <= 17 n sigma^2, so the subtraction amplifies the relative error of the
    sums by at most 17, and so for the cross sum by Cauchy-Schwarz.  A float64 sum of n terms in any order is within
    n 2^-53 of its sum of absolute values; at n = 32 769 that is 3.6e-12, times 17 is 6.2e-11 on the covariance
    relative to n sigma_t sigma_p and on each variance, i.e. at most 1.3e-10 on corr with the worst chain of additions
    (the kernel's longest chain is about 30 additions, not n).  1e-9 leaves 8x over the worst case."""
    sel = (lambda x: x[:, rows.long()]) if rows is not None else (lambda x: x)
    T = sel(t).double()
    out = []
    for p in preds:
        P = sel(p).double()
        assert first_row_within_4_sigma(T) and first_row_within_4_sigma(P), "first scored row beyond 4 sigma"
        d = P - T
        tc, pc = T - T.mean(1, keepdim=True), P - P.mean(1, keepdim=True)
        corr = (tc * pc).sum(1) / ((tc * tc).sum(1).sqrt() * (pc * pc).sum(1).sqrt() + 1e-8)
        out.append(torch.stack([(d * d).sum(1), d.abs().sum(1), corr], -1))
    return torch.stack(out, 1)


def colstats_one_pass(t, preds, rows):
    """The kernel's formula (shifted one-pass sums, verify.hip's header) in float64 torch, for the CPU cross-check."""
    sel = (lambda x: x[:, rows.long()]) if rows is not None else (lambda x: x)
    T = sel(t).double()
    n = T.shape[1]
    ts = T - T[:, :1]
    St, Stt = ts.sum(1), (ts * ts).sum(1)
    out = []
    for p in preds:
        P = sel(p).double()
        ps, d = P - P[:, :1], P - T
        Sp, Spp, Stp = ps.sum(1), (ps * ps).sum(1), (ts * ps).sum(1)
        vt, vp = (Stt - St * (St / n)).clamp_min(0), (Spp - Sp * (Sp / n)).clamp_min(0)
        corr = (Stp - St * (Sp / n)) / (vt.sqrt() * vp.sqrt() + 1e-8)
        out.append(torch.stack([(d * d).sum(1), d.abs().sum(1), corr], -1))
    return torch.stack(out, 1)


class ColCase:
    """One layout case: truth on padded rows, prediction q as PRED_LAYOUTS[q] (1 and 3 wider, through a column map with
    a permutation and, for K > 1, a repeated column), every unscored row NaN, and the float64 reference."""

    def __init__(self, z, n, K, npred, B, use_rows, seed):
        g = torch.Generator().manual_seed(seed)
        G = n + 5 if use_rows else n
        self.rows = None
        first = 0
        if use_rows:  # unsorted, from row 2 on, with a duplicate
            r = row_list(n, g)
            self.rows, first = i32(r), int(r[0])
        t, preds = columns(z[:, :B, :G], first)
        Wm = K + 3
        self.maps = [None, torch.randperm(Wm, generator=g)[:K], None, torch.arange(Wm - 1, Wm - 1 - K, -1)]
        if K > 1:
            self.maps[1][K - 1] = self.maps[1][0]
        self.maps = [None if m is None else i32(m) for m in self.maps[:npred]]
        self.T = Rows.of(t[..., :K], "pad_nan", NAN)
        self.P = [Rows.of(preds[q][..., :K if self.maps[q] is None else Wm], PRED_LAYOUTS[q], NAN,
                          ld=Wm + 5 if q == 1 else None) for q in range(npred)]
        if use_rows:
            unscored = torch.ones(G, dtype=torch.bool, device=DEV)
            unscored[self.rows.long()] = False
            for r_ in [self.T] + self.P:
                r_.view[:, unscored] = NAN
        self.n, self.K, self.B, self.npred = n, K, B, npred
        used = [preds[q][..., :K] if self.maps[q] is None else preds[q][..., self.maps[q].long()] for q in range(npred)]
        self.ref = colstats_ref(t[..., :K], used, self.rows)

    def run(self, hip, cols=None, sample=None):
        """The kernel's statistics; `cols`: of that column range scored alone, `sample`: of that sample alone."""
        c0, c1 = cols if cols is not None else (0, self.K)
        bsel = slice(None) if sample is None else slice(sample, sample + 1)
        preds = []
        for P, m in zip(self.P, self.maps):
            preds.append((P.view[bsel, :, c0:c1], None) if m is None else (P.view[bsel], m[c0:c1].contiguous()))
        out = Guarded((self.B if sample is None else 1, self.npred, c1 - c0, 3), torch.float64)
        hip.verify_colstats(self.T.view[bsel, :, c0:c1], preds, self.rows, out.view)
        torch.cuda.synchronize()
        assert out.untouched(), "verify_colstats wrote outside stats"
        return out.view

    def check(self, stats, what):
        n = self.n
        W.within("colstats se/ae", stats[..., :2], self.ref[..., :2], n * E52 * self.ref[..., :2], f"{what}: se, ae")
        W.within("colstats corr", stats[..., 2], self.ref[..., 2], 1e-9, f"{what}: corr")
        const = torch.arange(self.K, device=DEV) % 3 == 2
        assert bool((stats[:, :, const, 2] == 0).all()), f"{what}: corr of a constant column is not exactly 0"


@gpu
@pytest.mark.parametrize("n", NS)
def test_verify_colstats(hip, pool, n):
    """Every K x npred at this n, B alternating between 1 and 3, with and without a row list."""
    i = NS.index(n)
    for iK, K in enumerate(KS):
        for npred in (1, 2, 3, 4):
            B = (1, 3)[(i + iK + npred) % 2]
            for use_rows in (False, True):
                case = ColCase(pool, n, K, npred, B, use_rows, seed=1000 * i + 10 * iK + npred)
                case.check(case.run(hip), f"n={n} K={K} npred={npred} B={B} rows={use_rows}")
    W.report("colstats se/ae", "colstats corr")


@gpu
@pytest.mark.parametrize("n", NS)
def test_verify_colstats_column_and_sample_alone(hip, pool, n):
    """A column's bits do not depend on K, on the other columns or on B."""
    case = ColCase(pool, n, 33, 4, 3, True, seed=77 + n)
    full = case.run(hip)
    case.check(full, f"n={n}")
    for k in (0, 19, 31, 32):
        assert same_bits(case.run(hip, cols=(k, k + 1)), full[:, :, k:k + 1]), f"n={n}: column {k} alone differs"
    assert same_bits(case.run(hip, sample=2), full[2:3]), f"n={n}: sample 2 alone differs"


@gpu
@pytest.mark.parametrize("npred", [1, 2, 3, 4])
def test_verify_colstats_instance(hip, pool, npred):
    case = ColCase(pool, 65, 19, npred, 1, False, seed=5)
    _, names = launched(lambda: case.run(hip))
    assert [str(npred)] in targs(names, "colstats_partial_kernel"), names
    assert [str(npred)] in targs(names, "colstats_combine_kernel"), names


def test_colstats_references_agree():
    """CPU: the two-pass reference and a float64 restatement of the kernel's shifted one-pass formula agree far inside
    the bounds on these columns, so the bounds are left to the kernel."""
    z = deviates(135)
    for n in (1, 7, 65, 129):
        for use_rows in (False, True):
            g = torch.Generator().manual_seed(n)
            rows = None
            if use_rows:
                rows = row_list(n, g)
            t, preds = columns(z[:, :, :n + 5 if use_rows else n], int(rows[0]) if use_rows else 0)
            a, b = colstats_ref(t, preds, rows), colstats_one_pass(t, preds, rows)
            assert bool(((a[..., :2] - b[..., :2]).abs() <= 0.01 * n * E52 * a[..., :2]).all())
            assert float((a[..., 2] - b[..., 2]).abs().max()) <= 1e-11
            assert bool((b[:, :, torch.arange(WMAX) % 3 == 2, 2] == 0).all())


# ------------------------------------------------------------------------------------------------------------------
# verify_accumulate
# ------------------------------------------------------------------------------------------------------------------
def accumulate_ref(stats, jobs, state, masks):
    """verify.hip's accumulate in its documented order, on numpy float64 arrays (state is updated in place)."""
    for off, bstride, ncols, C, so, mo, nrows, B in jobs:
        for b in range(B):
            sb = off + b * bstride
            for ch in range(C):
                for c in range(ch, ncols, C):
                    state[so + 4 + ch] += stats[sb + 3 * c]
                    state[so + 4 + C + ch] += stats[sb + 3 * c + 2]
                    state[so + 4 + 2 * C + ch] += np.float64(nrows)
                    state[so + 4 + 3 * C + ch] += 1.0
            se = ae = cols = np.float64(0.0)
            for c in range(ncols):
                if mo >= 0 and masks[mo + c % C]:
                    continue
                se, ae, cols = se + stats[sb + 3 * c], ae + stats[sb + 3 * c + 1], cols + 1.0
            if cols > 0:
                state[so] += se
                state[so + 1] += ae
                state[so + 3] += cols * np.float64(nrows)
            state[so + 2] += 1.0


@gpu
@pytest.mark.parametrize("C,H", [(1, 1), (1, 3), (19, 2), (64, 1), (65, 3), (130, 2)])
@pytest.mark.parametrize("B", [1, 3])
def test_verify_accumulate(hip, C, H, B):
    """Four jobs on one statistics buffer (all horizons unmasked; the last horizon with some channels excluded; all
    horizons with every channel excluded, the `cols > 0` branch; all horizons partly masked), states and masks at
    different offsets, two calls into the same states."""
    rng = np.random.default_rng(100 * C + 10 * H + B)
    ncols, lead, gap = C * H, 2, 5
    bstride = 3 * ncols + gap
    size = 4 + 4 * C
    so = [3 + j * (size + 3) for j in range(4)]
    some = (rng.random(C) < 0.4).astype(np.uint8)
    some[0] = 1
    masks = np.concatenate([np.zeros(3, np.uint8), some, np.ones(2, np.uint8), np.ones(C, np.uint8), some[::-1]])
    mo = [-1, 3, 3 + C + 2, 3 + 2 * C + 2]
    jobs = [(lead, bstride, ncols, C, so[0], mo[0], 96, B), (lead + 3 * C * (H - 1), bstride, C, C, so[1], mo[1], 40, B),
            (lead, bstride, ncols, C, so[2], mo[2], 96, B), (lead, bstride, ncols, C, so[3], mo[3], 7, B)]
    state = np.full(so[-1] + size + 3, SENT)
    for s in so:
        state[s:s + size] = rng.random(size) * 10
    state_d = torch.from_numpy(state).to(DEV)
    jobs_d = torch.tensor(jobs, dtype=torch.int64, device=DEV)
    masks_d = torch.from_numpy(masks).to(DEV)
    for call in range(2):
        stats = np.full(lead + B * bstride, NAN)
        for b in range(B):
            v = stats[lead + b * bstride:lead + b * bstride + 3 * ncols].reshape(ncols, 3)
            v[:, :2] = rng.random((ncols, 2)) * 1e3
            v[:, 2] = rng.uniform(-1, 1, ncols)
        hip.verify_accumulate(torch.from_numpy(stats).to(DEV), jobs_d, state_d, masks_d)
        accumulate_ref(stats, jobs, state, masks)
        assert same_bits(state_d, torch.from_numpy(state).to(DEV)), f"call {call}: state differs from the float64 loop"
    W.exact("accumulate (bit-equal)")


# ------------------------------------------------------------------------------------------------------------------
# regrid_blend, taper_blend
# ------------------------------------------------------------------------------------------------------------------
def regrid_ref(src, nlat, cell, w, K):
    """float64, left to right, every product rounded on its own, the sum rounded once to float32 (verify.hip)."""
    n00 = cell[:, 0].astype(np.int64) * nlat + cell[:, 1]
    s = src.astype(np.float64)[..., :K]
    acc = s[:, n00] * w[None, :, 0, None]
    for j, d in ((1, 1), (2, nlat), (3, nlat + 1)):
        acc = acc + s[:, n00 + d] * w[None, :, j, None]
    return acc.astype(np.float32)


def blend_ref(m, r, g):
    """float32, one rounding per operation: m r + (1 - m) g."""
    m = m.astype(np.float32)[None, :, None]
    return m * r + (np.float32(1.0) - m) * g


def regrid_case(B, nt, K, nlon=7, nlat=6, seed=0):
    rng = np.random.default_rng(seed)
    cell = np.stack([rng.integers(0, nlon - 1, nt), rng.integers(0, nlat - 1, nt)], 1).astype(np.int32)
    if nt:
        cell[0] = (nlon - 2, nlat - 2)  # reads the last row and the last column of the source
        cell[nt // 2] = (0, 0)
    w = rng.random((nt, 4))
    w /= w.sum(1, keepdims=True) if nt else 1.0
    src = rng.standard_normal((B, nlon * nlat, K + 2)) * 30 + 250
    used = np.zeros(nlon * nlat, bool)
    n00 = cell[:, 0].astype(np.int64) * nlat + cell[:, 1]
    for d in (0, 1, nlat, nlat + 1):
        used[n00 + d] = True
    src[:, ~used] = NAN
    mask = rng.random(nt).astype(np.float32)
    if nt > 2:
        mask[1], mask[2] = 0.0, 1.0
    r = (rng.standard_normal((B, nt, K)) * 30 + 250).astype(np.float32)
    return cell, w, src, mask, r


@gpu
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("mode", ["g", "out", "both"])
@pytest.mark.parametrize("B,nt,K", [(1, 53, 19), (2, 300, 5), (3, 0, 4)])
def test_regrid_blend(hip, f64, mode, B, nt, K):
    cell, w, src, mask, r = regrid_case(B, nt, K, seed=B + nt)
    dt = torch.float64 if f64 else torch.float32
    src = src if f64 else src.astype(np.float32)
    S = Rows.of(torch.from_numpy(src), "pad_nan", NAN, dtype=dt)  # K + 2 columns on wider rows: K is below both
    Rr = Rows.of(torch.from_numpy(r), "colblock", NAN)
    Gg, Oo = Rows(nt, K, "odd_ld", SENT, "out", B=B), Rows(nt, K, "offset", SENT, "out", B=B)
    want_g, want_o = mode in ("g", "both"), mode in ("out", "both")
    hip.regrid_blend(S.view, 6, i32(cell).view(nt, 2), torch.from_numpy(w).to(DEV), K, g3=Gg.view if want_g else None,
                     mask=torch.from_numpy(mask).to(DEV) if want_o else None, r3=Rr.view if want_o else None,
                     out3=Oo.view if want_o else None)
    torch.cuda.synchronize()
    g_ref = regrid_ref(src, 6, cell, w, K)
    assert Gg.untouched(SENT) and Oo.untouched(SENT)
    if want_g:
        assert same_bits(Gg.view, torch.from_numpy(g_ref).to(DEV)), "regrid differs from numpy float64 rounded once"
    else:
        assert bool((Gg.buf == SENT).all())
    if want_o:
        assert same_bits(Oo.view, torch.from_numpy(blend_ref(mask, r, g_ref)).to(DEV)), "blend differs from numpy float32"
    else:
        assert bool((Oo.buf == SENT).all())
    W.exact("regrid / taper blend (bit-equal)")


@gpu
@pytest.mark.parametrize("f64", [False, True])
def test_regrid_keeps_the_sign_of_zero(hip, f64):
    """A target whose four corners hold -0.0: the first product starts the sum, so the value is -0.0, as numpy's and
    scipy's; a sum started from 0.0 would give +0.0 (0.0 + -0.0)."""
    B, nt, K, i = 2, 53, 5, 7
    cell, w, src, _, _ = regrid_case(B, nt, K, seed=3)
    n00 = int(cell[i, 0]) * 6 + int(cell[i, 1])
    src[:, [n00, n00 + 1, n00 + 6, n00 + 7]] = -0.0
    src = src if f64 else src.astype(np.float32)
    g_ref = regrid_ref(src, 6, cell, w, K)
    assert (g_ref[:, i].view(np.uint32) == 0x80000000).all(), "the restatement itself gives -0.0"
    S = Rows.of(torch.from_numpy(src), "pad_nan", NAN, dtype=torch.float64 if f64 else torch.float32)
    Gg = Rows(nt, K, "odd_ld", SENT, "out", B=B)
    hip.regrid_blend(S.view, 6, i32(cell).view(nt, 2), torch.from_numpy(w).to(DEV), K, g3=Gg.view)
    torch.cuda.synchronize()
    assert Gg.untouched(SENT)
    assert same_bits(Gg.view, torch.from_numpy(g_ref).to(DEV)), "regrid differs from numpy float64 rounded once"
    assert (Gg.view[:, i].contiguous().cpu().numpy().view(np.uint32) == 0x80000000).all()


@gpu
@pytest.mark.parametrize("B,nt,K", [(1, 53, 19), (2, 300, 5), (3, 0, 4)])
def test_taper_blend(hip, B, nt, K):
    _, _, _, mask, r = regrid_case(B, nt, K, seed=7)
    g = (np.random.default_rng(8).standard_normal((B, nt, K)) * 30 + 250).astype(np.float32)
    Rr, Gg = Rows.of(torch.from_numpy(r), "colblock", NAN), Rows.of(torch.from_numpy(g), "odd_ld", NAN)
    Oo = Rows(nt, K, "offset", SENT, "out", B=B)
    hip.taper_blend(torch.from_numpy(mask).to(DEV), Rr.view, Gg.view, Oo.view)
    torch.cuda.synchronize()
    assert Oo.untouched(SENT)
    assert same_bits(Oo.view, torch.from_numpy(blend_ref(mask, r, g)).to(DEV))


# ------------------------------------------------------------------------------------------------------------------
# pipeline_sqerr
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("C,G", [(1, 100), (1, 300), (19, 7), (19, 40), (128, 1), (128, 5), (129, 1), (129, 3), (256, 1),
                                 (256, 3)])  # G on both sides of the 256 // C row lanes
@pytest.mark.parametrize("V", [1, 3])
def test_pipeline_sqerr(hip, C, G, V):
    """Variants a padded sample apart, padded truth, station rows with a duplicate, then no stations; horizons 0 and
    H - 1 into the same accumulators, which start from non-zero sums."""
    rng = np.random.default_rng(1000 * C + 10 * G + V)
    H = 3
    p = (rng.standard_normal((V, G, C)) * 3 + 280).astype(np.float32)
    t = (rng.standard_normal((G, C)) * 3 + 280).astype(np.float32)
    P, T = Rows.of(torch.from_numpy(p), "odd_ld", NAN), Rows.of(torch.from_numpy(t), "colblock", NAN)
    stn = rng.integers(0, G, 5).astype(np.int32)
    stn[4] = stn[0]
    a0 = rng.random((2, V, H, C)) * 100
    Ag, As = Guarded((V, H, C), torch.float64, init=torch.from_numpy(a0[0])), \
        Guarded((V, H, C), torch.float64, init=torch.from_numpy(a0[1]))
    sq = (p - t[None]) * (p - t[None])  # float32 difference and square, as numpy rounds them
    assert sq.dtype == np.float32
    ref_g, ref_s = a0[0].copy(), a0[1].copy()
    for h, st in ((0, stn), (H - 1, stn[:0]), (H - 1, stn)):
        hip.pipeline_sqerr(P.view, T.view, i32(st), h, Ag.view, As.view)
        ref_g[:, h] += sq.astype(np.float64).sum(1)
        ref_s[:, h] += sq[:, st.astype(np.int64)].astype(np.float64).sum(1)
    hip.pipeline_sqerr(P.view, T.view, None, 0, Ag.view, None)  # grid sums alone
    ref_g[:, 0] += sq.astype(np.float64).sum(1)
    torch.cuda.synchronize()
    assert Ag.untouched() and As.untouched()
    for A, ref, a, n in ((Ag, ref_g, a0[0], G), (As, ref_s, a0[1], max(G, 5))):
        ref = torch.from_numpy(ref).to(DEV)
        W.within("sqerr", A.view, ref, n * E52 * ref, f"C={C} G={G} V={V}")
        assert same_bits(A.view[:, 1], torch.from_numpy(a[:, 1]).to(DEV)), "horizon 1 was never scored"
    W.report("sqerr")


# ------------------------------------------------------------------------------------------------------------------
# pipeline_roi_phys, pipeline_lapse, pipeline_lapse_geopotential, pipeline_station_obs
# ------------------------------------------------------------------------------------------------------------------
LAPSE = 6.5e-3


def lapse_ref(t, z, elev, f64):
    """pipeline.hip's lapse_t: a weak (Python float) elevation keeps every step float32, a float64 one makes the
    difference and the product float64 and rounds t + delta once."""
    if f64:
        return (t.astype(np.float64) + (z.astype(np.float64) - elev) * LAPSE).astype(np.float32)
    return t + (z - np.float32(elev)) * np.float32(LAPSE)


@gpu
@pytest.mark.parametrize("use_rows", [False, True])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("lapse,f64,tz", [(False, False, (3, 5)), (True, False, (3, 5)), (True, True, (18, 0)),
                                          (True, True, (-1, -1))])
def test_pipeline_roi_phys(hip, use_rows, residual, lapse, f64, tz):
    rng = np.random.default_rng(3)
    N, G, C = 90, 37, 19  # G C = 703, no multiple of 256
    t_idx, z_idx = tz
    elev = 431.7
    pred, xl = rng.standard_normal((N, C + 3)).astype(np.float32), rng.standard_normal((N, C + 1)).astype(np.float32)
    mean, std = (rng.standard_normal(C) * 100).astype(np.float32), (rng.random(C) * 50 + 1).astype(np.float32)
    rows = rng.permutation(np.arange(5, N))[:G].astype(np.int32)
    rows[G - 1] = rows[0]
    src = rows.astype(np.int64) if use_rows else np.arange(11, 11 + G)
    live = np.zeros(N, bool)
    live[src] = True
    pred[~live], xl[~live] = NAN, NAN
    P, X = Rows.of(torch.from_numpy(pred), "pad_nan", NAN), Rows.of(torch.from_numpy(xl), "odd_ld", NAN)
    raw, lap = Guarded((G, C)), Guarded((G, C))
    hip.pipeline_roi_phys(P.view, X.view if residual else None, i32(rows) if use_rows else None, 11, G,
                          torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV), t_idx, z_idx, elev, f64,
                          raw.view, lap.view if lapse else None)
    torch.cuda.synchronize()
    v = pred[src, :C]
    if residual:
        v = xl[src, :C] + v
    ref = v * std + mean
    assert raw.untouched() and lap.untouched()
    assert same_bits(raw.view, torch.from_numpy(ref).to(DEV)), "raw differs from numpy float32"
    if lapse:
        ref_l = ref.copy()
        if z_idx >= 0:
            ref_l[:, t_idx] = lapse_ref(ref[:, t_idx], ref[:, z_idx], elev, f64)
        assert same_bits(lap.view, torch.from_numpy(ref_l).to(DEV)), "lapse copy differs from numpy"
    else:
        assert bool((lap.buf == SENT).all())
    W.exact("pipeline glue (bit-equal)")


@gpu
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("G,S,C", [(37, 3, 19), (1, 1, 2), (300, 2, 5)])
def test_pipeline_lapse(hip, f64, G, S, C):
    rng = np.random.default_rng(G)
    x = (rng.standard_normal((G, S, C)) * 40 + 270).astype(np.float32)
    t_idx, z_idx, elev = 1, 0, 212.25
    got = hip.pipeline_lapse(torch.from_numpy(x).to(DEV), t_idx, z_idx, elev, f64)
    ref = x.copy()
    ref[:, :, t_idx] = lapse_ref(x[:, :, t_idx], x[:, :1, z_idx], elev, f64)
    assert same_bits(got, torch.from_numpy(ref).to(DEV))
    # the geopotential form: t2m + f32(6.5e-3 f32(f32(z / 9.80665) - elev)), every step float32
    out = Guarded((G, S, C))
    hip.pipeline_lapse_geopotential(torch.from_numpy(x).to(DEV), C - 1, z_idx, elev, out=out.view)
    torch.cuda.synchronize()
    ref = x.copy()
    dh = x[:, :1, z_idx] / np.float32(9.80665) - np.float32(elev)
    ref[:, :, C - 1] = x[:, :, C - 1] + np.float32(LAPSE) * dh
    assert out.untouched() and same_bits(out.view, torch.from_numpy(ref).to(DEV))


@gpu
@pytest.mark.parametrize("G,C,S", [(37, 19, 6), (300, 5, 1), (4, 3, 0)])
def test_pipeline_station_obs(hip, G, C, S):
    rng = np.random.default_rng(S)
    t = rng.standard_normal((G, C)).astype(np.float32)
    stn = rng.integers(0, G, S).astype(np.int32)
    if S > 1:
        stn[S - 1] = stn[0]
    T, out = Rows.of(torch.from_numpy(t), "pad_nan", NAN), Guarded((G, C))
    hip.pipeline_station_obs(T.view, i32(stn), out=out.view)
    torch.cuda.synchronize()
    hit = np.zeros(G, bool)
    hit[stn] = True
    assert out.untouched()
    assert torch.equal(torch.isnan(out.view).cpu(), torch.from_numpy(~hit)[:, None].expand(G, C))
    assert same_bits(out.view[torch.from_numpy(hit).to(DEV)], torch.from_numpy(t[hit]).to(DEV))
