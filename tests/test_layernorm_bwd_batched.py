"""The mapped + skip LayerNorm backward that serves four trips of a lane group together (the default) against the
single-trip kernel (GCL_LN_BWD_BATCH=0).

Rows keep their (block, lane group, trip) places and every lane adds its terms in the same order, so dx of the present
rows, dgamma, dbeta and the column sums are compared with torch.equal.  Both are also held to the float64 restatement
and the bounds of tests/test_norm_glue.py.  At F = 64 and F = 48 a block serves 16 rows per trip and the grid is capped
at 1024 blocks, so a sweep is 16384 rows: only a row count above 4 * 16384 reaches the batched body at all."""
import pytest
import torch

from test_norm_glue import DEV, EPS, LNRef, ln_inputs, rand, randn, within

pytestmark = pytest.mark.gpu
NAN = float("nan")
N_PER = 130
SWEEP = 1024 * 16  # rows of one trip of the whole grid
# B * 130 rows: below one sweep (every row is the ragged tail); 4 sweeps + 114 rows (one batch, one partial tail trip);
# 5 sweeps + 110 rows (one batch, then a whole and a partial single trip)
SIZES = {"below_sweep": 3, "four_trips": 505, "five_trips": 631}


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def make_map(kind, B, seed):
    """(keep [rows of the kernel's sample] bool, samples of the kernel, rows per sample).  The per-node maps repeat over
    the B samples of 130 rows; the two that drop rows by their place in the whole row space hand the kernel ONE sample
    of B * 130 rows."""
    gen = torch.Generator().manual_seed(seed)
    rows = B * N_PER
    if kind == "half":
        return torch.rand(N_PER, generator=gen) < 0.5, B, N_PER
    if kind == "none_dropped":
        return torch.ones(N_PER, dtype=torch.bool), B, N_PER
    keep = torch.ones(rows, dtype=torch.bool)
    if kind == "whole_sample":
        s = B // 2
        keep[s * N_PER:(s + 1) * N_PER] = False
    elif kind == "whole_trips":
        # trips 1 and 2 of every lane group (all of them inside the first batch), and the last whole trip
        keep[SWEEP:3 * SWEEP] = False
        last = (rows // SWEEP - 1) * SWEEP
        keep[last:last + SWEEP] = False
    else:
        raise ValueError(kind)
    return keep, 1, rows


CASES = [(F, size, kind) for F in (64, 48) for size in SIZES for kind in ("half", "whole_trips", "whole_sample", "none_dropped")
         if not (kind == "whole_trips" and size == "below_sweep")]  # below one sweep there is no whole trip to drop


@pytest.mark.parametrize("F,size,kind", CASES)
def test_batched_equals_single_trip(hip, monkeypatch, F, size, kind):
    B = SIZES[size]
    rows = B * N_PER
    keep, Bk, n = make_map(kind, B, seed=F + B)
    nk, head = int(keep.sum()), 3
    pos = torch.full((n,), -1, dtype=torch.int32)
    pos[keep] = (head + torch.randperm(nk, generator=torch.Generator().manual_seed(7))).to(torch.int32)
    pos_d, keep_d = pos.to(DEV), keep.to(DEV)
    rows_of = pos[keep].long().to(DEV)
    present = keep_d.repeat(Bk) if Bk > 1 else keep_d  # [rows]

    x = ln_inputs(rows, F, seed=F + 1)
    gm, bt = rand(F, seed=5) + 0.5, randn(F, seed=6)
    _, stats = hip.layernorm_fwd(x, gm, bt, EPS)
    Fsrc = F + 4
    src3 = randn(Bk, head + nk + 2, Fsrc, seed=F + 2)
    src3[:, :, F:] = NAN  # the padding of dy's source rows
    dyd = torch.zeros(Bk, n, F, device=DEV)
    dyd[:, keep_d] = src3[:, rows_of, :F]
    ref = LNRef(x, gm, bt, dyd.view(rows, F))

    def bwd(batch, fill):
        if batch:
            monkeypatch.delenv("GCL_LN_BWD_BATCH", raising=False)
        else:
            monkeypatch.setenv("GCL_LN_BWD_BATCH", "0")
        xs, st = x.clone(), stats.clone()
        xs[~present] = fill
        st[~present] = fill
        dg, db, cs = (torch.full((F,), -7.25, device=DEV) for _ in range(3))
        dx = hip.layernorm_bwd(None, xs, gm, st, dg, db, False, colsum_dx=cs, dy_map=(src3, pos_d), skip=True)
        return dx, dg, db, cs

    dx0, dg0, db0, cs0 = bwd(False, 0.0)
    for fill in (0.0, NAN):
        dx1, dg1, db1, cs1 = bwd(True, fill)
        assert torch.equal(dx1[present], dx0[present]), "dx of the present rows"
        assert torch.equal(dg1, dg0) and torch.equal(db1, db0) and torch.equal(cs1, cs0)
        assert bool(torch.isfinite(dg1).all() and torch.isfinite(db1).all() and torch.isfinite(cs1).all())
    # absent rows of dx are not written: filled with NaN beforehand they stay NaN.  (hip.layernorm_bwd allocates dx, so
    # the raw call is made here with a buffer of this test's own.)
    dxn = torch.full((rows, F), NAN, device=DEV)
    dg2, db2, cs2 = (torch.zeros(F, device=DEV) for _ in range(3))
    L = hip.lib()
    ws = hip.workspace(L.gcl_layernorm_bwd_ws_bytes(rows, F), DEV)
    monkeypatch.delenv("GCL_LN_BWD_BATCH", raising=False)
    hip._check(L.gcl_layernorm_bwd_map_skip(src3.data_ptr(), src3.stride(1), src3.stride(0), pos_d.data_ptr(), n, x.data_ptr(), F,
                                            gm.data_ptr(), stats.data_ptr(), dxn.data_ptr(), F, dg2.data_ptr(), db2.data_ptr(),
                                            cs2.data_ptr(), 0, rows, F, ws.data_ptr(), ws.numel(), hip._stream()))
    assert bool(torch.isnan(dxn[~present]).all()), "an absent row of dx was written"
    assert torch.equal(dxn[present], dx0[present]) and torch.equal(dg2, dg0) and torch.equal(cs2, cs0)

    # float64 and the bounds of the mapped kernel's own test
    within(dx1[present], ref.dx[present], ref.tol_dx[present], "batched dx vs float64")
    within(dg1, ref.dg, ref.tol_dg, "batched dgamma vs float64")
    within(db1, ref.db, ref.tol_db, "batched dbeta vs float64")
    within(cs1, ref.dx.sum(0), ref.tol_cs, "batched colsum(dx) vs float64")
