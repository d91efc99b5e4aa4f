"""The regional-model glue (csrc/dual_mesh.hip, csrc/roi.hip), the grouped Adam (csrc/optim.hip) and the multi-resolution
window pack (csrc/multires.hip) called through their thin hip.py wrappers or the C entry points, on operands laid out by
tests/helpers/layouts.py (NaN around every input, the sentinel around every output), against restatements written here
from the kernel files' comments.  Nothing here imports dual_mesh.py, roi_residual.py, multires.py or train.py.

Rules:
  segment_wsum      float64 sum in edge order; per element (deg + 4) U (sum_k |w_k act(x_k)| + |addend| + |old|), a SiLU
                    term carrying the 1e-6 |x| + 1e-37 that test_norm_glue allows act_fwd; rows of empty segments bit-equal
                    to what one float32 add of old and addend gives (+0 with neither); LPR asserted by template argument
  cross_update_fwd  pre within (deg + 3) U (|h| + sum |msg| / deg), bit-equal to h without edges; y and the statistics
                    within LNRef's condition-number bounds on the kernel's own pre
  roi_gather_rows   bit-equal to torch indexing; a bad index gives a row of zeros; the neighbours of the column block keep
                    their bits
  roi_compose       bit-equal: pred + (0 + corr) on ROI rows, pred itself (-0.0 included) elsewhere; both instances by name
  adam_step_groups  active parameters bit-equal to gcl_adam_step on the same slice at the same step; a frozen parameter's
                    NaN p / g / m / v, step and bc keep their bits
  window_pack       bit-equal to a numpy restatement, NaN for frames outside the series
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, U, Guarded, Rows, Worst, has, launched, rand, randn, same_bits, targs  # noqa: E402
from ln_ref import LNRef  # noqa: E402

pytestmark = pytest.mark.gpu
W_ = Worst("regional glue kernels")
NUM_CU = 256  # gcl::kNumCU, which sizes the row kernels' grid caps


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV).contiguous()


def csr(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------
# gcl_segment_wsum
# ------------------------------------------------------------------------------------------------------------------
SW_LPR = {4: 8, 32: 8, 36: 16, 64: 16, 68: 32, 128: 32, 252: 32, 256: 64, 260: 64, 516: 64}  # 516: two column trips
SW_LENS = (0, 1, 2, 9, 40, 0, 2, 1, 0, 9, 1)
SW_VARIANTS = (  # B, batch-1 source, SiLU, idx, w, addend, accumulate
    (1, False, False, True, True, False, False),
    (3, True, True, True, True, True, False),
    (3, False, False, False, False, False, True),
    (1, False, True, True, False, True, True),
)


def segment_wsum_check(hip, D, layout, lens, variant, seed, n_src=None, lpr=None):
    B, bcast, silu, with_idx, with_w, with_add, acc = variant
    n, E = len(lens), int(np.sum(lens))
    rowptr = csr(lens)
    if n_src is None:
        n_src = max(E - 3, 1)  # without idx edge k reads row k: the last three are out of range
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n_src, E)
    idx[rng.random(E) < 0.1] = -1
    idx[rng.random(E) < 0.1] = n_src  # neither may contribute, and row n_src holds NaN
    Bs = 1 if bcast else B
    src = randn(Bs, n_src + 3, D, seed=seed) * 2
    src[:, n_src:] = NAN
    S = Rows.of(src, layout, NAN)
    w = randn(E, seed=seed + 1) if with_w else None
    A = Rows.of(randn(B, n, D, seed=seed + 2), layout, NAN) if with_add else None
    old = randn(B, n, D, seed=seed + 3)
    O = Rows.of(old, layout, SENT, role="out") if acc else Rows(n, D, layout, SENT, role="out", B=B)
    _, names = launched(lambda: hip.segment_wsum(S.view[:, :n_src], i32(idx) if with_idx else None, w, i32(rowptr),
                                                 out3=O.view, addend3=A.view if A else None,
                                                 act=hip.ACT_SILU if silu else hip.ACT_NONE, accumulate=acc))
    if lpr is not None:
        assert targs(names, "segment_wsum_kernel") == [[str(lpr)]], names
    assert O.untouched(SENT)
    j = torch.from_numpy(idx if with_idx else np.arange(E)).to(DEV)
    ok = (j >= 0) & (j < n_src)
    x = src.double()[:, j.clamp(0, n_src - 1)].expand(B, E, D)
    ax = Fn.silu(x) if silu else x
    wk = (w.double() if with_w else torch.ones(E, dtype=torch.float64, device=DEV)) * ok
    terms = torch.where(ok[None, :, None], wk[None, :, None] * ax, torch.zeros_like(ax))
    seg = torch.repeat_interleave(torch.arange(n, device=DEV), torch.from_numpy(np.asarray(lens)).to(DEV))
    ref = torch.zeros(B, n, D, dtype=torch.float64, device=DEV).index_add_(1, seg, terms)
    mag = torch.zeros_like(ref).index_add_(1, seg, terms.abs())
    slack = torch.zeros_like(ref)
    if silu:
        slack.index_add_(1, seg, wk.abs()[None, :, None] * (1e-6 * x.abs().nan_to_num() + 1e-37) * ok[None, :, None])
    for t, on in ((A.view if A else None, with_add), (old, acc)):
        if on:
            ref, mag = ref + t.double(), mag + t.double().abs()
    deg = torch.from_numpy(np.asarray(lens, dtype=np.float64)).to(DEV)[None, :, None]
    W_.within("segment_wsum", O.view, ref, (deg + 4) * U * mag + slack, f"D={D} {layout} {variant}")
    empty = torch.from_numpy(np.asarray(lens) == 0).to(DEV)
    e = torch.zeros(B, n, D, device=DEV)
    if with_add:
        e = e + A.view
    if acc:
        e = old + e
    assert same_bits(O.view[:, empty], e[:, empty]), "a row without edges"


@pytest.mark.parametrize("layout", ("pad_nan", "colblock", "tight"))
@pytest.mark.parametrize("D", list(SW_LPR))
def test_segment_wsum_every_lane_count(hip, D, layout):
    for k, variant in enumerate(SW_VARIANTS):
        segment_wsum_check(hip, D, layout, SW_LENS, variant, 100 * D + k, lpr=SW_LPR[D])
    W_.report("segment_wsum")


def test_segment_wsum_rows_past_the_grid(hip):
    """D = 4 (32 rows per block) and 33 rows more than kNumCU * 32 blocks hold: the row loop takes a second trip."""
    n = NUM_CU * 32 * 32 + 33
    segment_wsum_check(hip, 4, "pad_nan", np.ones(n, dtype=np.int64), SW_VARIANTS[0], 7, n_src=1000, lpr=8)
    W_.report("segment_wsum")


# ------------------------------------------------------------------------------------------------------------------
# gcl_cross_update_fwd
# ------------------------------------------------------------------------------------------------------------------
CU_CASES = [(D, 23, B) for D in (4, 36, 132, 252, 256) for B in (1, 3)]
CU_CASES += [(4, NUM_CU * 16 * 4 + 5, 1), (132, NUM_CU * 16 * 2 + 3, 3)]  # five rows more than kNumCU * 16 blocks of four hold


@pytest.mark.parametrize("D,n,B", CU_CASES)
def test_cross_update_fwd(hip, D, n, B):
    lens = np.array([(0, 1, 7)[i % 3] for i in range(n)])
    E = int(lens.sum())
    h, msg = randn(B, n, D, seed=D + n) + 0.5, randn(B, E, D, seed=D + n + 1) * 2
    Hh, M = Rows.of(h, "pad_nan", NAN), Rows.of(msg, "colblock", NAN)
    gm, bt = Guarded((D,), fill=NAN, init=rand(D, seed=3) + 0.5), Guarded((D,), fill=NAN, init=randn(D, seed=4))
    pre, y, stats = Guarded((B, n, D)), Guarded((B, n, D)), Guarded((B * n, 2))
    rowptr = i32(csr(lens))

    def call():
        hip._check(hip.lib().gcl_cross_update_fwd(Hh.ptr, Hh.ld, Hh.bs, M.ptr, M.ld, M.bs, rowptr.data_ptr(),
                                                  gm.view.data_ptr(), bt.view.data_ptr(), 1e-5, pre.view.data_ptr(),
                                                  y.view.data_ptr(), stats.view.data_ptr(), B, n, D, hip._stream()))

    _, names = launched(call)
    assert has(names, "cross_update_fwd_kernel")
    assert pre.untouched() and y.untouched() and stats.untouched()
    seg = torch.repeat_interleave(torch.arange(n, device=DEV), torch.from_numpy(lens).to(DEV))
    deg = torch.from_numpy(lens.astype(np.float64)).to(DEV)[None, :, None]
    inv = torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros_like(deg))
    ssum = torch.zeros(B, n, D, dtype=torch.float64, device=DEV).index_add_(1, seg, msg.double())
    sabs = torch.zeros(B, n, D, dtype=torch.float64, device=DEV).index_add_(1, seg, msg.double().abs())
    W_.within("cross_update pre", pre.view, h.double() + ssum * inv, (deg + 3) * U * (h.double().abs() + sabs * inv),
              f"D={D} n={n} B={B}")
    lone = torch.from_numpy(lens == 0).to(DEV)
    assert same_bits(pre.view[:, lone], h[:, lone]), "a row without edges is not h"
    x = pre.view.reshape(B * n, D)
    ref = LNRef(x, gm.view, bt.view, torch.zeros_like(x))
    ref.check_fwd(y.view.reshape(B * n, D), stats.view, f"D={D} n={n} B={B}")
    W_.report("cross_update pre")


# ------------------------------------------------------------------------------------------------------------------
# gcl_roi_gather_rows
# ------------------------------------------------------------------------------------------------------------------
ROI_GATHER = {  # source widths, Fp, B, n, source rows, map, batch-1 second source
    "krsk_widths": ((38, 256, 19), 316, 3, 41, 60, "rows", False),
    "one_quad_wider": ((38, 256, 19), 320, 1, 41, 60, "rows", True),
    "narrow_with_empty_source": ((1, 0, 2), 4, 3, 9, 20, "rows", False),
    "narrow_one_quad_wider": ((1, 0, 2), 8, 1, 9, 20, "bad", False),
    "one_source": ((38,), 40, 3, 17, 30, "identity", False),
    "two_sources": ((38, 256), 296, 1, 30, 30, "identity", False),
    "bad_rows": ((38, 256, 19), 316, 3, 41, 60, "bad", True),
    "past_the_grid": ((38, 256, 19), 320, 3, 2300, 500, "bad", False),  # 552000 quads, 2048 * 256 = 524288 per trip
}


@pytest.mark.parametrize("name", list(ROI_GATHER))
def test_roi_gather_rows(hip, name):
    widths, Fp, B, n, rows_src, kind, bcast = ROI_GATHER[name]
    rng = np.random.default_rng(len(name))
    srcs, dense = [], []
    for k, wd in enumerate(widths):
        Bk = 1 if bcast and k == 1 else B
        t = randn(Bk, rows_src, max(wd, 1), seed=10 * n + k)[:, :, :wd]
        dense.append(t.expand(B, rows_src, wd))
        srcs.append(Rows.of(t, ("pad_nan", "colblock", "tight")[k], NAN) if wd else None)
    rows = None
    if kind != "identity":
        rows = rng.integers(0, rows_src, n)
        if kind == "bad":
            rows[1], rows[n - 2], rows[n // 2] = -1, rows_src, rows_src + 7
    O = Rows(n, Fp, "colblock", SENT, role="out", B=B)
    _, names = launched(lambda: hip.roi_gather_rows(None if rows is None else i32(rows), rows_src,
                                                    [s.view if s else None for s in srcs], Fp, B, out=O.view))
    assert has(names, "roi_gather_kernel")
    assert O.untouched(SENT)
    r = np.arange(n) if rows is None else rows
    good = torch.from_numpy((r >= 0) & (r < rows_src)).to(DEV)
    rc = torch.from_numpy(np.clip(r, 0, rows_src - 1)).to(DEV)
    want = torch.zeros(B, n, Fp, device=DEV)
    want[:, :, :sum(widths)] = torch.cat([d[:, rc] for d in dense], dim=2)
    want[:, ~good] = 0.0
    assert same_bits(O.view, want)
    W_.exact("roi_gather_rows")


# ------------------------------------------------------------------------------------------------------------------
# gcl_roi_compose
# ------------------------------------------------------------------------------------------------------------------
ROI_COMPOSE = {  # B, G, C, dense pred / out (the vector instance)
    "vec_partial_quad": (1, 7, 5, True),
    "vec_c1": (3, 33, 1, True),
    "vec_c8": (3, 19, 8, True),
    "vec_past_the_grid": (3, 140001, 5, True),  # 525004 quads, the last one partial
    "rows_c5": (3, 7, 5, False),
    "rows_c1": (1, 33, 1, False),
    "rows_c8": (3, 19, 8, False),
    "rows_past_the_grid": (3, 35001, 5, False),  # 525015 elements
}


@pytest.mark.parametrize("name", list(ROI_COMPOSE))
def test_roi_compose(hip, name):
    B, G, C, vec = ROI_COMPOSE[name]
    rng = np.random.default_rng(G + C)
    nroi = max(G // 3, 1)
    roi = rng.permutation(G)[:nroi]
    pos = np.full(G, -1, dtype=np.int32)
    pos[roi] = rng.permutation(nroi)
    pred, corr = randn(B, G, C, seed=G), randn(B, nroi, C + 2, seed=G + 1)
    pred[:, ::2, 0] = -0.0  # on ROI rows and on the others
    pred[:, torch.from_numpy(roi[::2]).to(DEV), 0] = -0.0  # and where the correction is -0.0 too
    at = torch.from_numpy(pos[roi[::2]]).long().to(DEV)
    corr[:, at, 0] = -0.0
    if vec:
        P, O = Guarded((B, G, C), fill=NAN, init=pred), Guarded((B, G, C))
        pv, ov = P.view, O.view
    else:
        P, O = Rows.of(pred, "pad_nan", NAN), Rows(G, C, "colblock", SENT, role="out", B=B)
        pv, ov = P.view, O.view
    Cr = Rows.of(corr, "tight", NAN)
    _, names = launched(lambda: hip.roi_compose(pv, Cr.view, i32(pos), out=ov))
    flag = targs(names, "roi_compose_kernel")
    assert len(flag) == 1 and flag[0][0] in (("true", "(bool)1") if vec else ("false", "(bool)0")), names
    assert O.untouched() if vec else O.untouched(SENT)
    assert same_bits(pv, pred)
    want = pred.clone()
    ri = torch.from_numpy(roi).to(DEV)
    want[:, ri] = pred[:, ri] + (0.0 + corr[:, torch.from_numpy(pos[roi]).long().to(DEV), :C])
    assert same_bits(ov, want)
    keep = torch.from_numpy(pos < 0).to(DEV)
    assert torch.signbit(ov[:, keep, 0][pred[:, keep, 0] == 0]).all(), "-0.0 outside the ROI became +0.0"
    both = (pred[:, ri, 0] == 0) & (corr[:, torch.from_numpy(pos[roi]).long().to(DEV), 0] == 0)
    assert both.any() and not torch.signbit(ov[:, ri, 0][both]).any()
    W_.exact("roi_compose")


# ------------------------------------------------------------------------------------------------------------------
# gcl_adam_step_groups
# ------------------------------------------------------------------------------------------------------------------
def test_adam_step_groups_past_the_grid(hip):
    """2 098 176 floats are 1024 more than 2048 blocks of 256 float4 hold: the grid-stride loop takes a second trip."""
    count = 2048 * 256 * 4 + 1024
    sizes = [1000, 64, 333, 1_000_000, 5, 700_001, 129, 64]
    padded = [(s + 63) // 64 * 64 for s in sizes]
    sizes.append(count - sum(padded))
    padded.append(sizes[-1])
    assert sizes[-1] > 0 and sizes[-1] % 64 == 0
    P = len(sizes)
    active = np.array([1, 0, 1, 1, 1, 0, 1, 1, 1], dtype=np.int32)
    active[3] = 0  # the million-element parameter is frozen: its chunks straddle many blocks
    lr = (1e-3 * (1 + np.arange(P))).astype(np.float32)
    step0 = (3 * np.arange(P) + 1).astype(np.int32)
    starts = np.concatenate([[0], np.cumsum(padded)])
    chunk_param = np.repeat(np.arange(P), np.asarray(padded) // 64).astype(np.int32)
    p, g = randn(count, seed=1), randn(count, seed=2)
    m, v = randn(count, seed=3) * 0.1, rand(count, seed=4) * 0.01
    for k in range(P):
        if not active[k]:
            for t in (p, g, m, v):  # a signalling NaN: any arithmetic on it, even + 0, changes its bits
                t.view(torch.int32)[starts[k]:starts[k + 1]] = 0x7F812345
    b1, b2, eps, wd, gscale = 0.9, 0.999, 1e-8, 0.01, 0.5
    want = []
    for k in range(P):
        sl = slice(int(starts[k]), int(starts[k + 1]))
        pk, mk, vk = p[sl].clone(), m[sl].clone(), v[sl].clone()
        if active[k]:
            hip.adam_step(pk, g[sl].clone(), mk, vk, float(lr[k]), b1, b2, eps, wd, int(step0[k]) + 1, gscale)
        want.append((pk, mk, vk))
    bufs = [Guarded((count,), fill=NAN, init=t) for t in (p, g, m, v)]
    step, bc = Guarded((P,), torch.int32, fill=-7, init=i32(step0)), Guarded((P, 2), init=torch.full((P, 2), 0.75, device=DEV))
    _, names = launched(lambda: hip.adam_step_groups(*(b.view for b in bufs), i32(chunk_param), i32(active),
                                                     torch.from_numpy(lr).to(DEV), step.view, bc.view, b1, b2, eps, wd,
                                                     gscale))
    assert has(names, "adam_groups_kernel") and has(names, "adam_groups_tick_kernel")
    assert step.untouched() and bc.untouched()
    assert all(bool(b.buf[:8].isnan().all()) and bool(b.buf[-8:].isnan().all()) for b in bufs)
    assert same_bits(bufs[1].view, g)
    assert step.view.tolist() == (step0 + active).tolist()
    for k in range(P):
        sl = slice(int(starts[k]), int(starts[k + 1]))
        for got, ref, what in zip((bufs[0], bufs[2], bufs[3]), want[k], "pmv"):
            assert same_bits(got.view[sl], ref), f"parameter {k} ({'active' if active[k] else 'frozen'}): {what}"
        if not active[k]:
            assert bc.view[k].tolist() == [0.75, 0.75]
    # no parameter, or no element, or neither: nothing is launched, nothing changes, no step is counted
    from torch.profiler import ProfilerActivity, profile

    before = [b.buf.clone() for b in bufs + [step, bc]]
    cp, act, lrd = i32(chunk_param), i32(active), torch.from_numpy(lr).to(DEV)
    for cnt, nparams in ((count, 0), (0, P), (0, 0)):
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            hip._check(hip.lib().gcl_adam_step_groups(*(b.view.data_ptr() for b in bufs), cnt, cp.data_ptr(), nparams,
                                                      act.data_ptr(), lrd.data_ptr(), step.view.data_ptr(),
                                                      bc.view.data_ptr(), b1, b2, eps, wd, gscale, hip._stream()))
            torch.cuda.synchronize()
        assert not [e.name for e in prof.events() if "adam_groups" in e.name], (cnt, nparams)
        assert all(same_bits(b.buf, a) for b, a in zip(bufs + [step, bc], before)), (cnt, nparams)
    W_.exact("adam_step_groups")


# ------------------------------------------------------------------------------------------------------------------
# gcl_multires_window_pack
# ------------------------------------------------------------------------------------------------------------------
MR_LON, MR_LAT, MR_CT, MR_C = 37, 21, 4, 3  # 16-point tiles: 3 x 2 of them, the last of each side partial (5 and 5 wide)


def mr_series(T, nlon, nlat, Ct, seed):
    return np.random.default_rng(seed).integers(-40, 41, (T, nlon, nlat, Ct)).astype(np.float16)


def mr_rank():
    """(rank [n_lat * n_lon] lat-major, n_kept): the box lon 5..9 x lat 3..10 (inside the first tile) is removed."""
    keep = np.ones((MR_LAT, MR_LON), dtype=bool)
    keep[3:11, 5:10] = False
    rank = np.where(keep.ravel(), np.cumsum(keep.ravel()) - 1, -1).astype(np.int32)
    return rank, int(keep.sum())


def mr_zscore(x, mean, std):
    return x if mean is None else ((x - mean) / std).astype(np.float32)


def mr_reference(gs, rs, rank, n_kept, n_reg, corner, w, t0, off_g, off_r, mean, std, first, frames, quantize):
    """[B, n_kept + n_reg, frames, C] float32 from multires.hip's comments: a kept global point (lon, lat) goes to row
    rank[lat * n_lon + lon]; merge mode appends the regional grid lat-major; interpolate mode adds the four corners'
    float64 products onto 0.0 in order, rounds to float32 and (quantize) through float16; a frame outside its series is
    NaN; the z-score is float32 arithmetic."""
    B, C = len(t0), MR_C
    out = np.full((B, n_kept + n_reg, frames, C), np.nan, dtype=np.float32)
    la, lo = np.divmod(np.arange(MR_LAT * MR_LON), MR_LON)
    kept = rank >= 0
    for b in range(B):
        for f in range(frames):
            t = t0[b] + off_g + first + f
            if 0 <= t < gs.shape[0]:
                out[b, rank[kept], f] = mr_zscore(gs[t, lo[kept], la[kept], :C].astype(np.float32), mean, std)
                if rs is None:
                    flat = gs[t].reshape(MR_LON * MR_LAT, -1)[:, :C].astype(np.float32).astype(np.float64)
                    acc = np.zeros((n_reg, C))
                    for j in range(4):
                        acc = acc + flat[corner[:, j]] * w[:, j:j + 1]
                    x = acc.astype(np.float32)
                    if quantize:
                        x = x.astype(np.float16).astype(np.float32)
                    out[b, n_kept:, f] = mr_zscore(x, mean, std)
            if rs is not None:
                t = t0[b] + off_r + first + f
                if 0 <= t < rs.shape[0]:
                    rla, rlo = np.divmod(np.arange(n_reg), rs.shape[1])
                    out[b, n_kept:, f] = mr_zscore(rs[t, rlo, rla, :C].astype(np.float32), mean, std)
    return out


@pytest.mark.parametrize("obs,T", [(2, 8), (43, 50)])  # 43 frames of 3 channels halve the tile to 8 points
@pytest.mark.parametrize("mode", ("merge", 63, 64, 65))  # the regional rows: a 5 x 9 grid, or around interp_rows' 64
def test_multires_window_pack(hip, mode, obs, T):
    gs = mr_series(T, MR_LON, MR_LAT, MR_CT, 1)
    rank, n_kept = mr_rank()
    rng = np.random.default_rng(obs)
    if mode == "merge":
        rs, n_reg, corner, w = mr_series(T + 2, 5, 9, MR_C, 2), 45, None, None
    else:
        rs, n_reg = None, mode
        corner = rng.integers(0, MR_LON * MR_LAT, (n_reg, 4)).astype(np.int32)
        a, b = rng.integers(0, 9, n_reg) / 8.0, rng.integers(0, 9, n_reg) / 8.0
        w = np.stack([(1 - a) * (1 - b), (1 - a) * b, a * (1 - b), a * b], axis=1)  # exact binary fractions
    t0 = np.array([1, -1, T - obs - 1], dtype=np.int64)  # the second window starts before the series, the third ends past it
    off_g, off_r = 0, 1
    mean = np.array([0.5, -3.0, 11.0], dtype=np.float32)
    std = np.array([1.7, 0.3, 12.0], dtype=np.float32)
    gd = torch.from_numpy(gs).to(DEV)
    rd = torch.from_numpy(rs).to(DEV) if rs is not None else None
    cd = i32(corner) if corner is not None else None
    wd = torch.from_numpy(w).to(DEV) if w is not None else None
    N = n_kept + n_reg
    for pred in (0, 3):
        for z in (False, True):
            for quantize in (False, True):
                for f16 in (False, True):
                    dt = torch.float16 if f16 else torch.float32
                    X = Guarded((len(t0), N, obs * MR_C), dt)
                    Y = Guarded((len(t0), N, max(pred, 1) * MR_C), dt)
                    m, s = (torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)) if z else (None, None)
                    hip.multires_window_pack(gd, rd, i32(rank), n_kept, n_reg, cd, wd, torch.from_numpy(t0).to(DEV), off_g,
                                             off_r, m, s, MR_C, obs, pred, quantize, out=(X.view, Y.view if pred else None),
                                             out_f16=f16)
                    torch.cuda.synchronize()
                    assert X.untouched() and Y.untouched()
                    what = f"{mode} obs={obs} pred={pred} z={z} quantize={quantize} f16={f16}"
                    for buf, first, frames in ((X, 0, obs), (Y, obs, pred)):
                        if frames == 0:
                            assert (buf.view == SENT).all(), what
                            continue
                        ref = mr_reference(gs, rs, rank, n_kept, n_reg, corner, w, t0, off_g, off_r, mean if z else None,
                                           std if z else None, first, frames, quantize)
                        ref = ref.reshape(len(t0), N, frames * MR_C)
                        ref = torch.from_numpy(ref.astype(np.float16) if f16 else ref).to(DEV)
                        assert ref.isnan().any() and not ref.isnan().all()
                        assert same_bits(buf.view, ref), what
    W_.exact("multires_window_pack")
