"""LayerNorm, GraphNorm and the column sums (csrc/norm.hip, csrc/graphnorm.hip), the glue every training step runs
(csrc/misc.hip: loss, AR step backward and advance, row padding and copies, the device-counter Adam) and the elementwise
activations (csrc/interaction.hip) against float64 restatements, on every dispatch variant: each lane count of the row
kernels, vector and scalar row access, padded, odd-strided and misaligned rows, row counts past the grid caps (so that
every grid-stride loop takes a second trip) and index walks that wrap.

Error bounds follow what fp32 arithmetic can promise, in units of the fp32 roundoff U: per row (or sample) they grow
with the condition |mean| / std of the normalisation, and every reduction is held to a multiple of the sum of |terms|.
A kernel that drops, repeats or misplaces a single term is far outside them."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

from oracle import pyg_ops as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, U, Rows, input_fill, rand, randn, within  # noqa: E402
from ln_ref import EPS, LNRef  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def lpr_for(F):
    lanes = (F + 3) // 4
    return 4 if lanes <= 4 else 8 if lanes <= 8 else 16 if lanes <= 16 else 32 if lanes <= 32 else 64


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm (mode="node")
# ------------------------------------------------------------------------------------------------------------------
def ln_inputs(rows, F, seed):
    """Random rows, with every 5th row (from row 1) at |mean| = 1e3 std and every 5th (from row 3) nearly constant
    (std 1e-4, far below sqrt(eps))."""
    x = randn(rows, F, seed=seed) * 1.5 + 0.3
    r = torch.arange(rows, device=DEV)
    far, flat = r % 5 == 1, r % 5 == 3
    sign = torch.where(r[far] % 2 == 0, 1.0, -1.0)
    x[far] = 1e3 * sign[:, None] + randn(int(far.sum()), F, seed=seed + 1)
    x[flat] = 0.5 + 1e-4 * randn(int(flat.sum()), F, seed=seed + 2)
    return x


def ln_fwd(hip, X, gm, bt, Y, stats, rows, F):
    hip._check(hip.lib().gcl_layernorm_fwd(X.ptr, X.ld, gm.data_ptr(), bt.data_ptr(), EPS, Y.ptr,
                                           Y.ld, stats.data_ptr(), rows, F, hip._stream()))


def ln_bwd(hip, DY, X, gm, stats, DX, dg, db, cs, acc, rows, F):
    L = hip.lib()
    ws = hip.workspace(L.gcl_layernorm_bwd_ws_bytes(rows, F), DEV)
    hip._check(L.gcl_layernorm_bwd_cs(DY.ptr, DY.ld, X.ptr, X.ld, gm.data_ptr(), stats.data_ptr(),
                                      DX.ptr, DX.ld, dg.data_ptr(), db.data_ptr(),
                                      None if cs is None else cs.data_ptr(), acc, rows, F, ws.data_ptr(), ws.numel(),
                                      hip._stream()))


LN_FS = (3, 12, 19, 32, 33, 64, 96, 128, 129, 200, 256)  # every LPR (4, 8, 16, 32, 64), both sides of F % 4
LN_LAYOUTS = ("contig", "pad_1e3", "pad_nan", "odd_ld", "offset", "mixed")
LN_CASES = [(F, lay, n) for F in LN_FS for lay in LN_LAYOUTS for n in ("7", "rpb+1", "past_caps")
            if n != "past_caps" or lay in ("contig", "pad_nan", "mixed")]


@pytest.mark.parametrize("F,layout,nrows", LN_CASES)
def test_layernorm_every_variant(hip, F, layout, nrows):
    """gcl_layernorm_fwd / gcl_layernorm_bwd_cs against float64 (autograd for the backward) on every lane count, every
    row layout and row counts of 7, one block plus one row, and past the 8192-block forward cap (which is also past the
    1024-block backward cap): the grid-stride loops of both directions take a second trip.  Padding of x and dy is
    ignored whatever it holds; columns of y and dx past F, and the padding of their buffers, are left as they were."""
    rpb = 4 * 64 // lpr_for(F)
    rows = {"7": 7, "rpb+1": rpb + 1, "past_caps": 8192 * rpb + rpb // 2 + 3}[nrows]
    x = ln_inputs(rows, F, seed=F)
    dy = randn(rows, F, seed=F + 100)
    gm, bt = rand(F, seed=3) + 0.5, randn(F, seed=4)
    ref = LNRef(x, gm, bt, dy)
    fill = input_fill(layout)
    X, DY = Rows.of(x, layout, fill), Rows.of(dy, layout, fill)
    Y, DX = Rows(rows, F, layout, SENT, "out"), Rows(rows, F, layout, SENT, "out")
    stats = torch.full((rows, 2), SENT, device=DEV)
    ln_fwd(hip, X, gm, bt, Y, stats, rows, F)
    ref.check_fwd(Y.view, stats, "forward")
    assert Y.untouched(SENT), "the forward wrote outside y[:, :F]"

    dg, db, cs = (torch.full((F,), SENT, device=DEV) for _ in range(3))
    ln_bwd(hip, DY, X, gm, stats, DX, dg, db, cs, 0, rows, F)
    ref.check_bwd(DX.view, dg, db, cs, "backward")
    assert DX.untouched(SENT), "the backward wrote outside dx[:, :F]"

    # the two accumulate bits act independently (the kernels are deterministic: a second identical call adds the
    # identical sums, so accumulation doubles them exactly)
    dx1, dg1, db1, cs1 = DX.view.clone(), dg.clone(), db.clone(), cs.clone()
    cs.fill_(5.0)
    ln_bwd(hip, DY, X, gm, stats, DX, dg, db, cs, hip.ACC_DW, rows, F)
    assert torch.equal(dg, 2 * dg1) and torch.equal(db, 2 * db1), "GCL_ACC_DW did not add into dgamma / dbeta"
    assert torch.equal(cs, cs1), "column sums accumulated without GCL_ACC_COLSUM"
    assert torch.equal(DX.view, dx1)
    dg.fill_(-3.0)
    db.fill_(-3.0)
    ln_bwd(hip, DY, X, gm, stats, DX, dg, db, cs, hip.ACC_COLSUM, rows, F)
    assert torch.equal(dg, dg1) and torch.equal(db, db1), "dgamma / dbeta accumulated without GCL_ACC_DW"
    assert torch.equal(cs, 2 * cs1), "GCL_ACC_COLSUM did not add into the column sums"

    # without column sums: the other instantiation
    DX2 = Rows(rows, F, layout, SENT, "out")
    dg2, db2 = torch.full((F,), SENT, device=DEV), torch.full((F,), SENT, device=DEV)
    ln_bwd(hip, DY, X, gm, stats, DX2, dg2, db2, None, 0, rows, F)
    ref.check_bwd(DX2.view, dg2, db2, None, "backward without column sums")
    assert DX2.untouched(SENT)


@pytest.mark.parametrize("F,Fsrc", [(19, 20), (64, 68), (200, 203)])
def test_layernorm_row_map(hip, F, Fsrc):
    """gcl_layernorm_fwd_map and the mapped backward (dy read through a row map, zero for pos = -1) with n_per = 777,
    which does not divide the backward's row step, and B * n_per past 1024 blocks of rows: the incremental (sample,
    row) walk of the backward wraps.  dy's source rows are padded with NaN.  Against the dense kernels on the gathered /
    zero-filled gradient, and against float64."""
    rpb = 4 * 64 // lpr_for(F)
    n = 777
    B = 1024 * rpb // n + 2
    rows = B * n
    gen = torch.Generator().manual_seed(F)
    keep = torch.rand(n, generator=gen) < 0.6
    nk, head = int(keep.sum()), 5
    m = head + nk + 3
    pos = torch.full((n,), -1, dtype=torch.int32)
    pos[keep] = (head + torch.randperm(nk, generator=gen)).to(torch.int32)
    pos_d, keep_d = pos.to(DEV), keep.to(DEV)
    rows_of = pos[keep].long().to(DEV)

    x = ln_inputs(rows, F, seed=F + 1)
    gm, bt = rand(F, seed=5) + 0.5, randn(F, seed=6)
    out3 = torch.full((B, m, Fsrc), SENT, device=DEV)
    st = hip.layernorm_fwd_map(x, gm, bt, EPS, out3, pos_d)
    y_d, st_d = hip.layernorm_fwd(x, gm, bt, EPS)
    y3 = y_d.view(B, n, F)
    got = out3[:, rows_of, :F]
    written = torch.zeros(B, m, Fsrc, dtype=torch.bool, device=DEV)
    written[:, rows_of, :F] = True
    assert bool((out3[~written] == SENT).all()), "the mapped forward wrote outside the mapped rows / first F columns"

    src3 = randn(B, m, Fsrc, seed=F + 2)
    src3[:, :, F:] = NAN
    dyd = torch.zeros(B, n, F, device=DEV)
    dyd[:, keep_d] = src3[:, rows_of, :F]
    dyd = dyd.view(rows, F)
    ref = LNRef(x, gm, bt, dyd)
    ref.check_fwd(y_d, st_d, "dense forward")
    within(st[:, 0], ref.mean, 32 * U * ref.mabs, "mapped forward: mean")
    within(st[:, 1], ref.rstd, ref.tol_rstd, "mapped forward: rstd")
    tol_y = ref.tol_y.view(B, n, 1)[:, keep_d]
    within(got, ref.y.view(B, n, F)[:, keep_d], tol_y, "mapped forward vs float64")
    # the two instantiations round the mean into the deviations differently (see LNRef): equal within both bounds
    within(got, y3[:, keep_d], 2 * tol_y, "mapped forward vs dense")

    dg, db, cs = (torch.full((F,), SENT, device=DEV) for _ in range(3))
    dx = hip.layernorm_bwd(None, x, gm, st, dg, db, False, colsum_dx=cs, dy_map=(src3, pos_d))
    dgd, dbd, csd = (torch.full((F,), SENT, device=DEV) for _ in range(3))
    dxd = hip.layernorm_bwd(dyd, x, gm, st, dgd, dbd, False, colsum_dx=csd)
    ref.check_bwd(dx, dg, db, cs, "mapped backward")
    within(dx, dxd, ref.tol_dx, "mapped backward vs dense")
    within(dg, dgd, ref.tol_dg, "mapped dgamma vs dense")
    within(db, dbd, ref.tol_db, "mapped dbeta vs dense")
    within(cs, csd, 1e-5 * dxd.double().abs().sum(0), "mapped column sums vs dense")


# ------------------------------------------------------------------------------------------------------------------
# Column sums
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 19, 129, 256])
@pytest.mark.parametrize("nrows", ["0", "1", "past_cap"])
@pytest.mark.parametrize("layout", ["contig", "pad_nan", "odd_ld"])
def test_colsum_every_variant(hip, F, nrows, layout):
    """gcl_colsum against a float64 sum: no rows, one row, and past the 1024-block cap with the four-rows-in-flight
    loop and the one-row tail both running; padded rows (NaN) and odd strides.  No rows with accumulate leaves the
    output as it was, without accumulate writes zeros; one row without accumulate is that row, exactly."""
    rpb = 4 * 64 // lpr_for(F)
    rows = {"0": 0, "1": 1, "past_cap": 5 * 1024 * rpb + 17}[nrows]
    x = randn(max(rows, 1), F, seed=F)[:rows] + 0.25
    X = Rows.of(x, layout, NAN)
    L = hip.lib()
    ws = hip.workspace(L.gcl_colsum_ws_bytes(rows, F), DEV)
    start = randn(F, seed=7)
    out = start.clone()
    hip._check(L.gcl_colsum(X.ptr, X.ld, rows, F, out.data_ptr(), 1, ws.data_ptr(), ws.numel(), hip._stream()))
    xd = x.double()
    within(out, start.double() + xd.sum(0), 1e-5 * (xd.abs().sum(0) + start.double().abs()), "accumulated column sums")
    if rows == 0:
        assert torch.equal(out, start), "no rows with accumulate changed the output"
    out2 = torch.full((F,), SENT, device=DEV)
    hip._check(L.gcl_colsum(X.ptr, X.ld, rows, F, out2.data_ptr(), 0, ws.data_ptr(), ws.numel(), hip._stream()))
    within(out2, xd.sum(0), 1e-5 * xd.abs().sum(0), "column sums")
    if rows <= 1:
        assert torch.equal(out2, x.sum(0) if rows else torch.zeros(F, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# GraphNorm (PyG LayerNorm mode="graph")
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [4, 19, 200, 256])
@pytest.mark.parametrize("layout", ["contig", "odd_ld"])
def test_graphnorm_every_variant(hip, F, layout):
    """gcl_graphnorm_fwd / _bwd against oracle.pyg_ops.pyg_layer_norm(.., "graph") in float64: the 16-byte path
    (contiguous, F % 4 == 0; F = 200 takes the scalar apply of the backward, 256 % (F / 4) != 0) and the scalar path
    (F = 19, odd strides), several partial chunks per sample and several backward blocks, one sample at a 1e3 offset
    and one with std = eps / 10 (eps is added to the std, not under the square root)."""
    B = 3
    n = max(-(-7 * 16384 // (2 * F)), 700)  # >= 3.5 chunks of 16K elements per sample, >= 3 backward blocks of 256 rows
    x = randn(B, n, F, seed=F) * 2 + 0.5
    x[1] = 1e3 + randn(n, F, seed=F + 1)
    x[2] = 1e-6 * randn(n, F, seed=F + 2)
    dy = randn(B, n, F, seed=F + 3)
    gm, bt = rand(F, seed=8) + 0.5, randn(F, seed=9)
    x64 = x.double().requires_grad_()
    g64, b64 = gm.double().requires_grad_(), bt.double().requires_grad_()
    y64 = P.pyg_layer_norm(x64, g64, b64, "graph")
    y64.backward(dy.double())
    y64 = y64.detach()

    def strided(t):
        X = Rows.of(t.reshape(B * n, F), layout, NAN)
        return X.view.view(B, n, F) if layout == "contig" else X.buf[:B * n * X.ld].view(B, n, X.ld)[:, :, :F]

    xs, dys = strided(x), strided(dy)
    assert torch.equal(xs, x) and torch.equal(dys, dy)
    y, stats = hip.graphnorm_fwd(xs, gm, bt)
    dg, db = torch.full((F,), SENT, device=DEV), torch.full((F,), SENT, device=DEV)
    dx = hip.graphnorm_bwd(dys, xs, gm, stats, dg, db, False)

    xd = x.double()
    mean = xd.mean(dim=(1, 2))
    std = xd.var(dim=(1, 2), unbiased=False).sqrt()
    rinv = 1.0 / (std + EPS)
    kappa = mean.abs() * rinv
    xhat = (xd - mean[:, None, None]) * rinv[:, None, None]
    hmax = xhat.abs().amax(dim=(1, 2))
    within(stats[:, 0], mean, 4 * U * (mean.abs() + std), "graph mean")
    within(stats[:, 1], rinv, 8 * U * rinv, "graph 1 / (std + eps)")
    tol_y = 32 * U * (kappa + 1 + hmax) * gm.abs().max() + 2 * U * bt.abs().max()
    within(y, y64, tol_y[:, None, None], "graph norm y")
    ady = dy.double().abs()
    q = (ady * gm.double()).amax(dim=(1, 2))
    tol_dx = 32 * U * (kappa + 4) * (1 + hmax) * rinv * q
    within(dx, x64.grad, tol_dx[:, None, None], "graph norm dx")
    tol_dg = 1e-5 * (ady * xhat.abs()).sum(dim=(0, 1)) + 32 * U * (ady * (kappa + 1)[:, None, None]).sum(dim=(0, 1))
    within(dg, g64.grad, tol_dg, "graph norm dgamma")
    within(db, b64.grad, 1e-5 * ady.sum(dim=(0, 1)), "graph norm dbeta")
    dg1, db1 = dg.clone(), db.clone()
    hip.graphnorm_bwd(dys, xs, gm, stats, dg, db, True)
    assert torch.equal(dg, 2 * dg1) and torch.equal(db, 2 * db1), "accumulate did not add into dgamma / dbeta"


# ------------------------------------------------------------------------------------------------------------------
# Training-step glue
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_x", [False, True])
@pytest.mark.parametrize("with_node_w", [False, True])
@pytest.mark.parametrize("with_chan_w", [False, True])
def test_wmse_fwd_bwd(hip, with_x, with_node_w, with_chan_w):
    """gcl_wmse_fwd_bwd (src/train.py:203-213): out = x_last + delta (or delta), loss = sum(w (out - y)^2) * inv_wsum,
    dd = 2 w (out - y) * inv_wsum * grad_scale, over B * G * C past 1024 blocks of 256 (every thread's (b, g, c) walk
    takes a second trip), x_last and y row-strided views, chained through loss_prev.  Loss and dd within 1e-6 of
    float64; the state is the fp32 delta + x_last, bit for bit."""
    B, G, C = 3, 4001, 33
    delta = randn(B, G, C, seed=1)
    xbuf, ybuf = randn(B, G, C + 5, seed=2), randn(B, G, C + 3, seed=3)
    x_last = xbuf[:, :, 2:2 + C] if with_x else None
    y = ybuf[:, :, :C]
    node_w = rand(G, seed=4) + 0.1 if with_node_w else None
    chan_w = rand(C, seed=5) + 0.5 if with_chan_w else None
    w64 = torch.ones(B, G, C, dtype=torch.float64, device=DEV)
    if with_chan_w:
        w64 = w64 * chan_w.double()
    if with_node_w:
        w64 = w64 * node_w.double()[:, None]
    w = w64.float().double()  # the kernel forms the weight in fp32
    inv = f32(1.0 / float(w64.sum()))  # the kernel takes it as fp32
    gs = 0.5
    o64 = delta.double() + (x_last.double() if with_x else 0.0)
    d64 = o64 - y.double()
    l64 = float((w * d64 * d64).sum()) * inv
    dd64 = 2 * w * d64 * inv * gs

    loss, dd, st = hip.wmse_fwd_bwd(delta, x_last, y, node_w, chan_w, inv, gs, want_grad=True, want_state=True)
    assert abs(loss.item() - l64) <= 1e-6 * l64, (loss.item(), l64)
    within(dd, dd64, 1e-6 * 2 * w * inv * gs * (o64.abs() + y.double().abs()), "dd")
    assert torch.equal(st, delta + x_last if with_x else delta), "state is not the fp32 delta + x_last"

    # chained: loss_prev + this loss; without gradient and state outputs
    loss2, dd2, st2 = hip.wmse_fwd_bwd(delta, x_last, y, node_w, chan_w, inv, gs, want_grad=False, loss_prev=loss)
    assert dd2 is None and st2 is None
    assert abs(loss2.item() - (loss.item() + l64)) <= 1e-6 * 2 * l64, (loss2.item(), loss.item() + l64)


CHAN_KINDS = [0, 1, 2, 0, 2, 1, 0]


def ar_step_ref(delta, state, y_step, kinds, has_y, residual, dd, g_loss, g_new):
    """float64 autograd of one AR training step: pred = x_last + delta (residual) or delta; the loss enters with
    d loss / d pred = dd; new_state = shift(state) with last slot pred, x_last for static channels, y for forcing ones."""
    d64, s64 = delta.double().requires_grad_(), state.double().requires_grad_()
    x_last = s64[:, :, -1]
    pred = x_last + d64 if residual else d64
    gl = 1.0 if g_loss is None else g_loss.double()
    total = gl * (dd.double() * pred).sum()
    k = kinds.long()
    last = torch.where(k == 1, x_last, pred)
    if has_y:
        last = torch.where(k == 2, y_step.double(), last)
    new_state = torch.cat([s64[:, :, 1:], last.unsqueeze(2)], dim=2)
    if g_new is not None:
        total = total + (g_new.double() * new_state).sum()
    total.backward()
    return d64.grad, (torch.zeros_like(s64) if s64.grad is None else s64.grad)  # (state unused: zero gradient)


AR_CASES = [(obs, res, hy, "small") for obs in (1, 3) for res in (False, True) for hy in (False, True)] + [(3, True, True, "past_cap")]


@pytest.mark.parametrize("obs,residual,has_y,size", AR_CASES)
def test_ar_step_bwd(hip, obs, residual, has_y, size):
    """gcl_ar_step_bwd against float64 autograd of the step forward (prediction, weighted loss, window shift with the
    static / forcing overwrite) for every channel kind, with g_new and g_loss each given and absent; the large case
    runs past 8192 blocks of 256 elements (every thread's walk takes a second trip)."""
    B, C = 2, len(CHAN_KINDS)
    G = 301 if size == "small" else 8192 * 256 // (obs * C) // B + 1001
    delta, state = randn(B, G, C, seed=1), randn(B, G, obs, C, seed=2)
    y_step, dd = randn(B, G, C, seed=3), randn(B, G, C, seed=4)
    g_new_full = randn(B, G, obs, C, seed=5)
    g_loss_t = torch.tensor(0.75, device=DEV)
    for kinds in (torch.tensor(CHAN_KINDS, dtype=torch.int32, device=DEV), None):
        kk = kinds if kinds is not None else torch.zeros(C, dtype=torch.int32, device=DEV)
        for g_new in (g_new_full, None):
            for g_loss in (g_loss_t, None):
                want_dd, want_ds = ar_step_ref(delta, state, y_step, kk, has_y, residual, dd, g_loss, g_new)
                d_delta, d_state = hip.ar_step_bwd(dd, g_loss, g_new, kinds, has_y, residual, obs, want_state=True)
                scale = dd.abs().amax() + 2 * g_new_full.abs().amax()
                what = f"kinds={'mixed' if kinds is not None else None} g_new={g_new is not None} g_loss={g_loss is not None}"
                within(d_delta, want_dd, 4 * U * scale, f"{what}: d_delta")
                within(d_state, want_ds, 4 * U * scale, f"{what}: d_state")
                d_delta2, none = hip.ar_step_bwd(dd, g_loss, g_new, kinds, has_y, residual, obs, want_state=False)
                assert none is None and torch.equal(d_delta2, d_delta)


@pytest.mark.parametrize("obs", [1, 3])
@pytest.mark.parametrize("residual", [False, True])
def test_ar_advance_into_wider_row(hip, obs, residual):
    """gcl_ar_advance with the step written at column out_off of a wider output row, delta and y_step row-strided:
    bit-exact to the float32 step (one add at most), every other column of the output untouched."""
    B, G, C = 2, 523, len(CHAN_KINDS)
    kinds = torch.tensor(CHAN_KINDS, dtype=torch.int32, device=DEV)
    state = randn(B, G, obs, C, seed=1)
    delta = randn(B, G, C + 4, seed=2)[:, :, 1:1 + C]
    y_step = randn(B, G, C + 2, seed=3)[:, :, :C]
    ow, off = 3 * C + 5, C + 2
    out = torch.full((B, G, ow), SENT, device=DEV)
    new = hip.ar_advance(state, delta, y_step, kinds, out, off, residual)
    want = (state[:, :, -1] + delta) if residual else delta.clone()
    k = kinds.long()
    want = torch.where(k == 1, state[:, :, -1], want)
    want = torch.where(k == 2, y_step, want)
    assert torch.equal(out[:, :, off:off + C], want)
    assert bool((out[:, :, :off] == SENT).all()) and bool((out[:, :, off + C:] == SENT).all())
    assert torch.equal(new, torch.cat([state[:, :, 1:], want.unsqueeze(2)], dim=2))


def strided3(B, rows, F, ld, bs, off, fill):
    """A [B, rows, F] view with row stride ld and batch stride bs, `off` floats into a buffer that holds `fill`;
    returns (buffer, view, its base pointer, mask of the view's elements in the buffer)."""
    buf = torch.full((off + B * bs + 4,), fill, device=DEV)
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
    torch.as_strided(inside, (B, rows, F), (bs, ld, 1), off).fill_(True)
    return buf, torch.as_strided(buf, (B, rows, F), (bs, ld, 1), off), buf.data_ptr() + 4 * off, inside


COPY_CASES = {  # F, source (ld, batch stride - rows * ld, base offset), destination (the same)
    "vector": (64, (68, 8, 0), (72, 4, 0)),
    "F%4": (33, (36, 4, 0), (40, 0, 0)),
    "odd_ld": (64, (65, 3, 0), (68, 4, 0)),
    "misaligned": (64, (68, 8, 1), (72, 4, 0)),
}


@pytest.mark.parametrize("case", sorted(COPY_CASES))
@pytest.mark.parametrize("nrows", ["0", "small", "past_cap"])
def test_copy_rows_bit_exact(hip, case, nrows):
    """gcl_copy_rows on its 16-byte and element variants (F % 4, odd strides, misaligned base): bit-exact, nothing
    written outside dst[:, :rows, :F]; no rows; and past 8192 blocks of 256 items (grid-stride loop)."""
    F, (lds, es, os_), (ldd, ed, od) = COPY_CASES[case]
    B = 2
    per = F // 4 if case == "vector" else F
    rows = {"0": 0, "small": 37, "past_cap": 8192 * 256 // (B * per) + 999}[nrows]
    bss, bsd = rows * lds + es, rows * ldd + ed
    _, src, src_p, _ = strided3(B, rows, F, lds, bss, os_, NAN)
    src.copy_(randn(B, rows, F, seed=F))
    dst_buf, dst, dst_p, inside = strided3(B, rows, F, ldd, bsd, od, SENT)
    hip._check(hip.lib().gcl_copy_rows(src_p, lds, bss, dst_p, ldd, bsd, B, rows, F, hip._stream()))
    assert torch.equal(dst, src)
    assert bool((dst_buf[~inside] == SENT).all()), "copy_rows wrote outside the destination rows"


@pytest.mark.parametrize("case", ["strided", "odd_ld", "misaligned", "no_rows", "no_cols", "past_cap"])
def test_pad_rows_bit_exact(hip, case):
    """gcl_pad_rows: dst[b, i, c] = src[b, i, c] for i < rows_src, c < F_src, else 0 - bit-exact, over row-strided,
    odd-strided and misaligned sources (padding NaN), rows_src = 0, F_src = 0, and past 8192 blocks of 256 elements."""
    B = 2
    rows_src, F_src, rows_dst, F_dst, lds, off = {
        "strided": (301, 33, 340, 36, 40, 0), "odd_ld": (301, 19, 305, 20, 21, 0), "misaligned": (300, 64, 300, 68, 68, 1),
        "no_rows": (0, 33, 50, 36, 36, 0), "no_cols": (40, 0, 50, 36, 36, 0), "past_cap": (32001, 33, 33001, 36, 37, 1)}[case]
    bss = rows_src * lds + 3
    _, src, src_p, _ = strided3(B, rows_src, F_src, lds, bss, off, NAN)
    src.copy_(randn(B, rows_src, F_src, seed=3))
    dst = torch.full((B, rows_dst, F_dst), SENT, device=DEV)
    hip._check(hip.lib().gcl_pad_rows(src_p, lds, bss, rows_src, F_src, dst.data_ptr(), F_dst, rows_dst * F_dst,
                                      rows_dst, F_dst, B, hip._stream()))
    want = torch.zeros(B, rows_dst, F_dst, device=DEV)
    want[:, :rows_src, :F_src] = src
    assert torch.equal(dst, want)


def f32(v):
    """v rounded to fp32: what the library receives for a float argument."""
    return float(torch.tensor(v, dtype=torch.float32))


def test_adam_step_dev_matches_torch_adam(hip):
    """gcl_adam_step_dev: 20 steps on the device step counter, with weight decay and grad_scale, against
    torch.optim.Adam in float64 (with the same fp32 hyper-parameters); the counter and the bias corrections it leaves
    behind.  The parameter count runs past 1024 blocks of 256 (grid-stride loop)."""
    count, steps = 1024 * 256 + 3001, 20
    lr, b1, b2, eps, wd, gs = f32(3e-3), f32(0.9), f32(0.999), f32(1e-8), f32(0.01), 0.5
    p = randn(count, seed=1)
    m, v = torch.zeros(count, device=DEV), torch.zeros(count, device=DEV)
    step_dev, bc_dev = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    p64 = p.double().clone().requires_grad_()
    opt = torch.optim.Adam([p64], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for t in range(steps):
        g = randn(count, seed=100 + t)
        g[::97] *= 1e-3  # a few small gradients
        hip.adam_step_dev(p, g, m, v, lr, b1, b2, eps, wd, step_dev, bc_dev, gs)
        p64.grad = g.double() * gs
        opt.step()
    st = opt.state[p64]
    assert int(step_dev.item()) == steps
    assert torch.equal(bc_dev.cpu(), torch.tensor([1 - b1 ** steps, math.sqrt(1 - b2 ** steps)], dtype=torch.float32))
    within(m, st["exp_avg"], 64 * U * st["exp_avg"].abs().amax(), "m")
    within(v, st["exp_avg_sq"], 64 * U * st["exp_avg_sq"].abs().amax(), "v")
    # per step p rounds once (U |p|), and the update (at most ~3 lr) carries the rounding of m, v and the bias
    # corrections, which builds up over the steps in m and v
    within(p, p64.detach(), steps * (2 * U * p64.detach().abs() + 64 * U * 3 * lr), "p")


@pytest.mark.parametrize("act", [1, 2])
def test_act_past_slope_cap(hip, act):
    """gcl_act_fwd / gcl_act_bwd (PReLU, SiLU) over more elements than 2048 blocks of 256 float4 (the slope-partial cap:
    the backward's grid-stride loop takes a second trip) against float64; the PReLU slope gradient within a bound
    proportional to the sum of |terms|."""
    count = 2048 * 256 * 4 + 400004
    x, dy = randn(count, seed=1) * 3, randn(count, seed=2)
    a = torch.tensor([0.3], device=DEV)
    x64 = x.double().requires_grad_()
    a64 = a.double().requires_grad_()
    y64 = Fn.prelu(x64, a64) if act == 1 else Fn.silu(x64)
    y64.backward(dy.double())
    ad = a if act == 1 else None
    y = hip.act_fwd(x, act, ad)
    within(y, y64.detach(), 1e-6 * x.double().abs() + 1e-37, "act forward")
    ds = torch.full((1,), 0.125, device=DEV) if act == 1 else None
    dx = hip.act_bwd(x, dy, act, ad, ds)
    within(dx, x64.grad, 1e-6 * (1 + x.double().abs()) * dy.double().abs(), "act backward")
    if act == 1:
        terms = (dy.double() * x.double())[x <= 0].abs().sum()
        assert abs(ds.item() - (0.125 + a64.grad.item())) <= 4 * U * float(terms) + U * 0.125, (ds.item(), a64.grad.item())
