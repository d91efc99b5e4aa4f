"""Contract of the kernels of csrc/region_train.hip as include/gcl.h states it: `gcl_region_cache_store` /
`gcl_region_cache_fetch` against torch indexing (bit-equal copies, zero pad columns, zero rows for what lies outside),
`gcl_region_eval_pair` against `hip.ar_advance` (bit-equal step_out and windows) and a restatement of the ROI loss in
extended precision on those float32 outputs.

Bound of the loss: every term is formed in float64 from float32 data and the terms are non-negative, so a fixed-order
sum of at most 3 * 300 * 5 of them keeps a relative error far below 1e-12 - the bar tests/test_eval_step_kernels.py
holds the sums of `gcl_eval_colstats` to."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, Guarded, Rows, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
G, C, OBS, D, HALF_E, M, DM = 300, 5, 2, 11, 7, 19, 6
XF = OBS * C
LD = np.longdouble


def _rows(n_roi, seed):
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(G, generator=g)[:n_roi].to(torch.int32)
    snd = torch.randint(0, M, (HALF_E,), generator=g).to(torch.int32)
    return rows, snd


def _sources(B, P, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(pred=r(B, G, C), lat=r(B, G, D), mesh=r(B, M, DM), X=r(B, G, XF), y=r(B, G, P * C))


def _expected(src, rows, snd, rec):
    """[B, rec.floats] records by torch indexing; a row index outside its source gives zeros."""
    B = src["X"].shape[0]

    def take(t, idx, width):
        n_src = t.shape[1]
        ok = (idx >= 0) & (idx < n_src)
        out = torch.zeros(B, idx.numel(), width)
        out[:, ok, :t.shape[2]] = t[:, idx[ok].long()]
        return out

    roi3 = take(torch.cat([src["X"], src["lat"]], -1), rows, rec.Sp)
    parts = [roi3, take(src["mesh"], snd, rec.Dgp), take(src["pred"], rows, rec.Cp), take(src["y"], rows, rec.Yp)]
    return torch.cat([p.reshape(B, -1) for p in parts], 1), parts


@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n_roi", [1, 37, 257])
def test_store_and_fetch_match_torch_indexing(n_roi, B, P, lib_built):
    from graphcast_lite_amd import hip

    rec = hip.RegionRecord(n_roi, HALF_E, XF, D, DM, C, P)
    assert rec.Sp == 24 and rec.Dgp == 8 and rec.Cp == 8 and rec.Yp == (8 if P == 1 else 12)
    assert rec.nbytes == 4 * rec.floats == 4 * (n_roi * (24 + 8 + rec.Yp) + HALF_E * 8)
    rows, snd = _rows(n_roi, 5 * n_roi + B)
    if n_roi > 3:
        rows[3] = G  # outside the grid: a zero row in roi3, pred and y
        snd[2] = -1
    src = _sources(B, P, 100 + n_roi + 7 * B + P)
    want, parts = _expected(src, rows, snd, rec)
    if n_roi > 3:
        assert bool((parts[0][:, 3] == 0).all()) and bool((parts[1][:, 2] == 0).all())
    # every source padded, strided or offset, NaN around it: a read of the padding poisons the record
    layouts = {"pred": "offset", "lat": "pad_nan", "mesh": "odd_ld", "X": "tight", "y": "contig"}
    lay = {k: Rows.of(v.to(DEV), layouts[k], NAN) for k, v in src.items()}
    n_slots = 6
    cache = Guarded((n_slots, rec.floats))
    cache.view.fill_(SENT)
    slots = {1: [3], 3: [4, -1, 2]}[B]  # out of order; the slot of sample 1 lies outside the cache: skipped
    hip.region_cache_store(rec, cache.view, torch.tensor(slots, device=DEV), lay["pred"].view, lay["lat"].view,
                           lay["mesh"].view, lay["X"].view, lay["y"].view, rows.to(DEV), snd.to(DEV))
    got = cache.view.cpu()
    assert cache.untouched()
    written = [s for s in slots if 0 <= s < n_slots]
    for b, s in enumerate(slots):
        if 0 <= s < n_slots:
            assert torch.equal(got[s], want[b]), (b, s)
    for s in range(n_slots):
        if s not in written:
            assert bool((got[s] == SENT).all()), s
    # pad columns are exactly zero (+0.0)
    roi3 = got[written[0], :n_roi * rec.Sp].view(n_roi, rec.Sp)
    assert same_bits(roi3[:, XF + D:], torch.zeros(n_roi, rec.Sp - XF - D))
    # fetch: repeated, out-of-order slots and two outside the cache
    fslots = [written[-1], written[0], written[-1], n_slots, 0, -3]
    Bf = len(fslots)
    dst = [Guarded(tuple(t.shape)) for t in rec.parts(Bf, DEV)]
    out = hip.region_cache_fetch(rec, cache.view, torch.tensor(fslots, device=DEV), out=[d.view for d in dst])
    for k, (d, o) in enumerate(zip(dst, out)):
        assert d.untouched()
        lo, size = rec.offsets[k], rec.sizes[k]
        for b, s in enumerate(fslots):
            ref = got[s, lo:lo + size] if 0 <= s < n_slots else torch.zeros(size)
            assert same_bits(o[b].cpu().reshape(-1), ref), (k, b, s)
    # a destination left out is not written, the others are the same
    only = hip.region_cache_fetch(rec, cache.view, torch.tensor(fslots, device=DEV),
                                  out=[dst[0].view, None, None, torch.empty_like(dst[3].view)])
    assert only[1] is None and torch.equal(only[3], dst[3].view)


def _pair_case(B, n_roi, P, step, kinds_on, seed):
    g = torch.Generator().manual_seed(seed)
    wins = [torch.randn(B, G, XF, generator=g) for _ in range(2)]
    deltas = [Rows.of(0.2 * torch.randn(B, G, C, generator=g).to(DEV), lay, NAN) for lay in ("pad_nan", "offset")]
    Y = torch.randn(B, G, P * C, generator=g).to(DEV)
    kinds = None
    if kinds_on:
        kinds = torch.zeros(C, dtype=torch.int32)
        kinds[1], kinds[3] = 1, 2  # one static, one forcing channel
        kinds = kinds.to(DEV)
    rows = torch.randperm(G, generator=g)[:n_roi].to(torch.int32).to(DEV)
    return [w.to(DEV) for w in wins], deltas, Y[:, :, step * C:(step + 1) * C], kinds, rows


def _ref_loss(out, y, rows):
    o, t = out.cpu().numpy().astype(LD), y.cpu().numpy().astype(LD)
    idx = rows.cpu().numpy() if rows is not None else np.arange(o.shape[1])
    return float(((o[:, idx] - t[:, idx]) ** 2).mean())


@pytest.mark.parametrize("nq", [1, 2])
@pytest.mark.parametrize("residual", [True, False])
@pytest.mark.parametrize("B,n_roi,P,kinds_on", [(1, 1, 1, False), (3, 37, 2, True), (3, 257, 2, True), (1, 257, 1, False)])
def test_eval_pair_matches_ar_advance_and_the_restated_loss(B, n_roi, P, kinds_on, residual, nq, lib_built):
    from graphcast_lite_amd import hip

    wins, deltas, y_step, kinds, rows = _pair_case(B, n_roi, P, P - 1, kinds_on, 31 * n_roi + B + nq)
    want_out, want_win = [], []
    for q in range(nq):
        o = torch.empty(B, G, C, device=DEV)
        want_win.append(hip.ar_advance(wins[q].view(B, G, OBS, C), deltas[q].view, y_step, kinds, o, 0, residual))
        want_out.append(o)
    new = [Guarded((B, G, OBS, C)) for _ in range(nq)]
    outs = [Rows(G, C, "pad_nan", SENT, role="out", B=B) for _ in range(nq)]
    acc0, weight = 0.5, 0.5
    accs = []
    for run in range(2):
        acc = Guarded((nq,), dtype=torch.float64, init=torch.full((nq,), acc0, dtype=torch.float64))
        preds = [(deltas[q].view, wins[q], new[q].view, outs[q].view) for q in range(nq)]
        hip.region_eval_pair(preds, y_step, kinds, residual, rows, weight, acc.view, OBS)
        assert acc.untouched()
        accs.append(acc.view.clone())
    assert same_bits(accs[0], accs[1])  # two runs, the same bits
    for q in range(nq):
        assert torch.equal(outs[q].view, want_out[q]) and outs[q].untouched(SENT)
        assert torch.equal(new[q].view, want_win[q]) and new[q].untouched()
        want = acc0 + weight * _ref_loss(want_out[q], y_step, rows)
        got = float(accs[0][q])
        print(f"B={B} n={n_roi} q={q}: loss state {got!r}, restated {want!r}")
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (q, got, want)
    # no window and no output: the same sums, nothing else written
    acc = torch.full((nq,), acc0, dtype=torch.float64, device=DEV)
    hip.region_eval_pair([(deltas[q].view, wins[q], None, None) for q in range(nq)], y_step, kinds, residual, rows, weight,
                         acc, OBS)
    assert same_bits(acc, accs[0])


@pytest.mark.parametrize("nq", [1, 2])
def test_eval_pair_on_compact_rows(nq, lib_built):
    """`rows` NULL: the inputs are the ROI rows themselves (the cached mode), the window a column block of wider rows."""
    from graphcast_lite_amd import hip

    B, n = 3, 37
    g = torch.Generator().manual_seed(9 + nq)
    roi3 = torch.randn(B, n, 24, generator=g).to(DEV)  # [X | latent | pad]: the window is its first obs * C columns
    deltas = [Rows.of(torch.randn(B, n, C, generator=g).to(DEV), "pad_nan", NAN) for _ in range(nq)]
    y = Rows.of(torch.randn(B, n, C, generator=g).to(DEV), "pad_zero", 0.0)
    acc = torch.zeros(nq, dtype=torch.float64, device=DEV)
    hip.region_eval_pair([(d.view, roi3, None, None) for d in deltas], y.view, None, True, None, 1.0, acc, OBS)
    for q in range(nq):
        out = roi3[..., XF - C:XF] + deltas[q].view
        want = _ref_loss(out, y.view, None)
        assert abs(float(acc[q]) - want) <= 1e-12 * max(1.0, abs(want))


def test_wrappers_reject_what_the_kernels_cannot_address(lib_built):
    from graphcast_lite_amd import hip

    rec = hip.RegionRecord(37, HALF_E, XF, D, DM, C, 1)
    cache = torch.zeros(4, rec.floats, device=DEV)
    slots = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        hip.region_cache_fetch(rec, cache[:, :-4], slots)
    with pytest.raises(ValueError):
        hip.region_cache_fetch(rec, cache, slots, out=rec.parts(3, DEV))
    with pytest.raises(AssertionError):
        hip.region_cache_fetch(rec, cache, slots.to(torch.int32))
    d = torch.zeros(2, G, C, device=DEV)
    w = torch.zeros(2, G, XF, device=DEV)
    with pytest.raises(ValueError):
        hip.region_eval_pair([(d, w, None, None)], d, None, True, None, 1.0, torch.zeros(2, dtype=torch.float64, device=DEV),
                             OBS)
    with pytest.raises(ValueError):
        hip.region_eval_pair([(d, w[..., :C], None, None)], d, None, True, None, 1.0,
                             torch.zeros(1, dtype=torch.float64, device=DEV), OBS)
