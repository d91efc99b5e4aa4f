"""The dense transforms (csrc/linear.hip, csrc/linear_x3.hip, csrc/gemm_tile.h) through the C ABI on padded, strided,
offset and column-block rows: gcl_dense_fwd / gcl_linear_fwd, gcl_dense_bwd_dx, gcl_dense_bwd_dw and gcl_linear_bwd_all.

Every operand is a view inside a buffer the test owns (tests/helpers/layouts.py).  Around an input the buffer holds
NaN, around an output a sentinel.  Each case
  - names the kernel and the template instance the launch code must pick for its shape and layout, and checks with the
    profiler that this one ran (the module asserts on import that its cases reach every instance listed in
    _required() at its end);
  - holds every output element to |got - ref| <= (K + 3) U sum_k |a_k b_k| of a float64 restatement (K: contraction
    length; the classical bound of an fp32 sum in any order, + 3 for the three dropped piece products of the
    split-operand kernels, csrc/x3.h, at most 2^-25 relative each) plus U |bias| and U |addend|;
  - runs the same call on a twin whose padding holds zeros instead of NaN and asserts BIT-equal results ("padding is
    ignored": include/gcl.h) - pad_nan against pad_zero, a column block with NaN against zero neighbours, and so on
    for every layout;
  - asserts that nothing outside the output views changed;
  - or, for a layout the entry point refuses, asserts GCL_EINVAL, a message and an untouched output.
Rows are 1, 63, 129, 257 (either side of the 64- and 128-row tiles) and one count per persistent kernel past
cap * tile rows, so that its grid-stride loop takes a second trip."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, U, Geom, Rows, launched, randn, same_bits, targs, within  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1
NUM_CU, LDS_BYTES = 256, 160 * 1024  # csrc/common.h
LAYOUTS = ("contig", "pad_nan", "tight", "colblock", "odd_ld", "offset", "mixed")
ROWS = (1, 63, 129, 257)


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture
def x3_off(monkeypatch):
    monkeypatch.setenv("GCL_X3", "0")


def lay(t, layout, fill, role="in"):
    return Rows.of(t, layout, fill, role)


def out_like(rows, F, layout, role="out"):
    return Rows(rows, F, layout, SENT, role)


def act64(x, act, a):
    return x if act == 0 else torch.where(x > 0, x, a * x) if act == 1 else x * torch.sigmoid(x)


def dact64(x, act, a):
    if act == 0:
        return torch.ones_like(x)
    if act == 1:
        return torch.where(x > 0, torch.ones_like(x), a * torch.ones_like(x))
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


# ------------------------------------------------------------------------------------------------------------------
# What the launch code must pick (csrc/linear.hip: gcl_dense_fwd, gcl_dense_bwd_dx, dw_block, bwd_all_impl)
# ------------------------------------------------------------------------------------------------------------------
def _ns(N):
    ns = (N + 31) // 32
    return 4 if ns == 3 else 8 if ns > 4 else ns


def _panel(K, N, vec, trans, w_ok):
    """panel_fits(): does the resident-panel kernel take this contraction?"""
    tile_ok = vec and w_ok and K % 4 == 0 and N % 4 == 0
    if tile_ok and (K > 128 or (N >= 128 and (K >= 128 or trans))):
        return False
    if K > 256 or N > 256 or (not vec and K > 128):
        return False
    return (_ns(N) * 32 + 64) * ((K + 3) // 4 * 4 + 2) * 4 + 64 <= LDS_BYTES


def _mfma(K, N, epi, vec):
    return ("linear_mfma_kernel", [str(_ns(N)), str(epi), str(64 if K <= 64 else 128 if K <= 128 else 256),
                                   "true" if vec else "false"])


def _tile(rows, K, N, epi, trans, x_ok, w_ok):
    """launch_gemm(): the 128 x 128 tile contraction, or the refusal of rows it cannot read 16 bytes at a time."""
    if not (K % 4 == 0 and x_ok and w_ok and (not trans or N % 4 == 0)):
        return EINVAL
    mi = 1 if -(-rows // 128) * -(-N // 128) < 3 * 2 * NUM_CU else 2
    if mi == 2 and not trans:
        return ("gemm_tile_x3_kernel", [str(epi)])
    return ("gemm_tile_kernel", [str(epi), "true" if trans else "false", str(mi)])


def expect_fwd(rows, Fin, Fout, X, Y, ldw, addend, act, x3=True):
    w_ok = ldw % 4 == 0
    vec = Fin % 4 == 0 and X.aligned()
    if not addend and ldw == Fin:
        if x3 and Fin <= 64 and 4 <= Fout <= 64 and Fout % 4 == 0 and X.aligned() and Y.aligned():
            return ("linear_x3_fwd_kernel", ["1" if Fout <= 32 else "2", "true" if act == 2 else "false",
                                             "2" if Fin <= 32 else "4"])
        if _panel(Fin, Fout, vec, False, w_ok):
            return _mfma(Fin, Fout, 0, vec)
    return _tile(rows, Fin, Fout, 0, False, X.aligned(), w_ok)


def expect_dx(rows, Fin, Fout, DY, ldw, addend):
    """The contraction runs over Fout; its "weights" are W^T."""
    w_ok = ldw % 4 == 0
    vec = Fout % 4 == 0 and DY.aligned()
    if not addend and ldw == Fin and _panel(Fout, Fin, vec, True, w_ok):
        return _mfma(Fout, Fin, 1, vec)
    if Fout % 4 == 0 and rows >= 4096:  # W is transposed into the workspace first: 16-byte rows of Fout floats
        return _tile(rows, Fout, Fin, 1, False, DY.aligned(), True)
    return _tile(rows, Fout, Fin, 1, True, DY.aligned(), w_ok)


def expect_dw(Fin, Fout, DY, X):
    nct = (Fin + 127) // 128
    no = (min(Fout, 256) + 31) // 32
    return ("dw_mfma_kernel", [str(no if no <= 2 else 4 if no <= 4 else 8), str(4 if nct > 1 else (Fin + 31) // 32),
                               "true" if DY.aligned() and X.aligned() else "false"])


def expect_all(rows, Fin, Fout, DY, X, DX, x3=True):
    fused = (Fout <= 64 and Fin <= 96 and Fin % 4 == 0 and DY.ld >= (Fout + 3) // 4 * 4 and DY.aligned() and X.aligned())
    if not fused:
        return None  # the three separate kernels
    no, nc = (Fout + 31) // 32, (Fin + 31) // 32
    if nc == 2 and x3 and DX.aligned():
        return ("linear_x3_bwd_kernel", [str(no)])
    if nc == 2:
        return ("linear_bwd_fused64_kernel", [str(no)])
    return ("linear_bwd_fused_kernel", [str(no), str(nc)])


def ran(names, want, what):
    kern, args = want
    got = targs(names, kern)
    print(f"ran: {kern}<{', '.join(args)}>  [{what}]")
    assert args in got, f"{what}: expected {kern}<{', '.join(args)}>, launched {names}"


def refused(hip, rc, OUT, what):
    assert rc == EINVAL, f"{what}: expected GCL_EINVAL, got {rc}"
    assert hip.lib().gcl_last_error(), f"{what}: refusal without a message"
    torch.cuda.synchronize()
    assert bool((OUT.buf == SENT).all()), f"{what}: a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------------------
# Forward
# ------------------------------------------------------------------------------------------------------------------
class Fwd:
    """One forward problem and its float64 answer; run(layout, fill) calls the library on that layout."""

    def __init__(self, hip, rows, Fin, Fout, act, wblock=False, addend=False, bias=True, seed=0):
        self.hip, self.rows, self.Fin, self.Fout, self.act = hip, rows, Fin, Fout, act
        self.x = randn(rows, Fin, seed=seed + 1)
        self.W = randn(Fout, Fin, seed=seed + 2) * 0.3
        self.b = randn(Fout, seed=seed + 3) if bias else None
        self.add = randn(rows, Fout, seed=seed + 4) if addend else None
        self.a = torch.tensor([0.25], device=DEV)
        self.wblock = wblock
        ax = act64(self.x.double(), act, 0.25)
        self.ref = ax @ self.W.double().t()
        self.tol = (Fin + 3) * U * (ax.abs() @ self.W.double().abs().t())
        if bias:
            self.ref = self.ref + self.b.double()
            self.tol = self.tol + U * self.b.double().abs()
        if addend:
            self.ref = self.ref + self.add.double()
            self.tol = self.tol + U * self.add.double().abs()

    def run(self, layout, fill, linear_entry=False):
        h, L = self.hip, self.hip.lib()
        X, Y = lay(self.x, layout, fill), out_like(self.rows, self.Fout, layout)
        Wl = lay(self.W, "colblock" if self.wblock else "contig", fill)
        A = lay(self.add, layout, fill) if self.add is not None else None
        sl = self.a.data_ptr() if self.act == 1 else None
        bp = self.b.data_ptr() if self.b is not None else None
        if linear_entry:
            rc = L.gcl_linear_fwd(X.ptr, X.ld, sl, Wl.ptr, bp, Y.ptr, Y.ld, self.rows, self.Fin, self.Fout, h._stream())
        else:
            rc = L.gcl_dense_fwd(X.ptr, X.ld, self.act, sl, Wl.ptr, Wl.ld, bp, A.ptr if A else None, A.ld if A else 0,
                                 Y.ptr, Y.ld, self.rows, self.Fin, self.Fout, h._stream())
        return rc, X, Y, Wl


def check_fwd(hip, rows, Fin, Fout, act, layout, x3=True, **kw):
    p = Fwd(hip, rows, Fin, Fout, act, seed=Fin + Fout, **kw)
    what = f"fwd rows={rows} {Fin}->{Fout} act={act} {layout} {kw}"
    (rc, X, Y, Wl), names = launched(lambda: p.run(layout, NAN))
    want = expect_fwd(rows, Fin, Fout, X, Y, Wl.ld, p.add is not None, act, x3)
    if want == EINVAL:
        return refused(hip, rc, Y, what)
    hip._check(rc)
    ran(names, want, what)
    assert Y.untouched(SENT), f"{what}: wrote outside y[:, :Fout]"
    rc0, _, Y0, _ = p.run(layout, 0.0)
    hip._check(rc0)
    assert same_bits(Y.view, Y0.view), f"{what}: NaN padding and zero padding give different results"
    within(Y.view, p.ref, p.tol, what)


FWD_SHAPES = [  # Fin, Fout: see EXPECTED for what each reaches
    (12, 32), (19, 32), (19, 64), (48, 32), (33, 64), (48, 64), (64, 33), (64, 19), (66, 48), (96, 66), (48, 96),
    (12, 132), (132, 33), (128, 64), (128, 132), (260, 132), (132, 260)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout", FWD_SHAPES)
def test_dense_fwd_layouts(hip, Fin, Fout, layout):
    """gcl_dense_fwd on every layout; all four row counts on the contiguous and the NaN-padded rows.  The activation
    cycles with the row count, so every kernel family sees none, PReLU and SiLU."""
    for i, rows in enumerate(ROWS if layout in ("contig", "pad_nan", "tight") else (129,)):
        check_fwd(hip, rows, Fin, Fout, (i + Fin + len(layout)) % 3, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout,kw", [
    (64, 64, dict(wblock=True)), (128, 132, dict(wblock=True)), (19, 32, dict(wblock=True)),
    (64, 48, dict(addend=True)), (132, 132, dict(addend=True, wblock=True)), (33, 64, dict(bias=False)),
    (64, 33, dict(bias=False))])
def test_dense_fwd_weight_block_and_addend(hip, Fin, Fout, kw, layout):
    """The weight as a column block of a wider matrix (ldw > Fin, NaN beside it) and the epilogue addend: both run the
    tile kernel, which refuses rows it cannot read 16 bytes at a time (Fin % 4 != 0, odd strides, a misaligned base);
    and the kernels without a bias."""
    check_fwd(hip, 129, Fin, Fout, (Fin + len(layout)) % 3, layout, **kw)


@pytest.mark.parametrize("layout", ["contig", "pad_nan", "tight", "offset"])
@pytest.mark.parametrize("Fin,Fout", [(19, 32), (33, 64), (64, 33), (48, 96)])
def test_dense_fwd_with_x3_off(hip, x3_off, Fin, Fout, layout):
    """GCL_X3=0: the fp32 MFMA panel kernel on the shapes the split-operand kernel takes by default."""
    check_fwd(hip, 129, Fin, Fout, (Fin + len(layout)) % 3, layout, x3=False)


def test_linear_fwd_entry_is_dense_fwd(hip):
    """gcl_linear_fwd (PReLU when in_slope is given) is gcl_dense_fwd with ldw = Fin: same bits."""
    for act in (0, 1):
        p = Fwd(hip, 129, 19, 32, act)
        rc, _, Y, _ = p.run("tight", NAN, linear_entry=True)
        hip._check(rc)
        rc, _, Y2, _ = p.run("tight", NAN)
        hip._check(rc)
        assert same_bits(Y.view, Y2.view) and Y.untouched(SENT)
        within(Y.view, p.ref, p.tol, f"gcl_linear_fwd act={act}")


# second trip of each persistent grid: cap * tile + tile + 1 rows (caps from the launch code)
FWD_LONG = [
    (48, 64, 2 * NUM_CU * 128 + 129, True),   # linear_x3_fwd_kernel: 2 blocks per CU, 128-row tiles
    (64, 33, 3 * NUM_CU * 128 + 129, True),   # linear_mfma_kernel<2, 0, 64>: kNumCU * bpc blocks, bpc = 3
    (128, 132, 3 * NUM_CU * 64 + 65, True),   # gemm_tile_kernel, 64-row tiles, 3 blocks per CU, two column tiles
    (12, 260, 512 * 128 + 1, True),           # gemm_tile_x3_kernel: 128-row tiles once there are 1536 of them
]


@pytest.mark.parametrize("layout", ["contig", "pad_nan"])
@pytest.mark.parametrize("Fin,Fout,rows,x3", FWD_LONG)
def test_dense_fwd_second_trip(hip, Fin, Fout, rows, x3, layout):
    check_fwd(hip, rows, Fin, Fout, 1, layout, x3=x3)


# ------------------------------------------------------------------------------------------------------------------
# dX
# ------------------------------------------------------------------------------------------------------------------
def slope_ok(got, ref, what):
    assert abs(got - ref) <= 1e-4 * max(1.0, abs(ref)), f"{what}: slope gradient {got!r}, float64 {ref!r}"


class Dx:
    def __init__(self, hip, rows, Fin, Fout, act, wblock=False, addend=False, seed=0):
        self.hip, self.rows, self.Fin, self.Fout, self.act, self.wblock = hip, rows, Fin, Fout, act, wblock
        self.dy = randn(rows, Fout, seed=seed + 1)
        self.W = randn(Fout, Fin, seed=seed + 2) * 0.3
        self.z = randn(rows, Fin, seed=seed + 3)
        self.add = randn(rows, Fin, seed=seed + 4) if addend else None
        self.a = torch.tensor([0.25], device=DEV)
        g = self.dy.double() @ self.W.double()
        d = dact64(self.z.double(), act, 0.25)
        self.ref = g * d
        self.tol = (Fout + 3) * U * (self.dy.double().abs() @ self.W.double().abs()) * d.abs()
        if act == 2:
            # SiLU' = s (1 + z (1 - s)), s = sigmoid(z), is formed in fp32 and its bracket cancels near z = -1.28, where
            # the bound above (relative to |SiLU'|) vanishes: the three roundings inside the bracket are each within
            # U (1 + |z|), and s (expf, one addition, one division: 3 U relative) enters it twice - an ABSOLUTE error
            # of at most 6 U s (1 + |z|) on the factor that multiplies dy W
            zd = self.z.double()
            self.tol = self.tol + g.abs() * 6 * U * torch.sigmoid(zd) * (1 + zd.abs())
        if addend:
            self.ref = self.ref + self.add.double()
            self.tol = self.tol + U * self.add.double().abs()
        zd = self.z.double()
        self.dslope = float((g * zd)[zd <= 0].sum()) if act == 1 else 0.0

    def run(self, layout, fill):
        h, L = self.hip, self.hip.lib()
        DY, DX = lay(self.dy, layout, fill), out_like(self.rows, self.Fin, layout)
        Z = lay(self.z, layout, fill) if self.act else None
        Wl = lay(self.W, "colblock" if self.wblock else "contig", fill)
        A = lay(self.add, layout, fill) if self.add is not None else None
        ds = torch.full((1,), 0.125, device=DEV)
        ws = h.workspace(L.gcl_linear_bwd_ws_bytes(self.rows, self.Fin, self.Fout), DEV)
        rc = L.gcl_dense_bwd_dx(DY.ptr, DY.ld, Wl.ptr, Wl.ld, Z.ptr if Z else None, Z.ld if Z else 0, self.act,
                                self.a.data_ptr() if self.act == 1 else None, ds.data_ptr() if self.act == 1 else None,
                                A.ptr if A else None, A.ld if A else 0, DX.ptr, DX.ld, self.rows, self.Fin, self.Fout,
                                ws.data_ptr(), ws.numel(), h._stream())
        return rc, DY, DX, Wl, ds


def check_dx(hip, rows, Fin, Fout, act, layout, **kw):
    p = Dx(hip, rows, Fin, Fout, act, seed=Fin + 2 * Fout, **kw)
    what = f"dx rows={rows} Fin={Fin} Fout={Fout} act={act} {layout} {kw}"
    (rc, DY, DX, Wl, ds), names = launched(lambda: p.run(layout, NAN))
    want = expect_dx(rows, Fin, Fout, DY, Wl.ld, p.add is not None)
    if want == EINVAL:
        return refused(hip, rc, DX, what)
    hip._check(rc)
    ran(names, want, what)
    if rows >= 4096 and Fout % 4 == 0 and want[0].startswith("gemm_tile"):
        assert any("transpose_kernel" in n for n in names), names
    assert DX.untouched(SENT), f"{what}: wrote outside dx[:, :Fin]"
    rc0, _, DX0, _, ds0 = p.run(layout, 0.0)
    hip._check(rc0)
    assert same_bits(DX.view, DX0.view) and same_bits(ds, ds0), f"{what}: NaN padding and zero padding differ"
    within(DX.view, p.ref, p.tol, what)
    if act == 1:
        slope_ok(ds.item(), 0.125 + p.dslope, what)


DX_SHAPES = [  # Fin, Fout
    (64, 33), (33, 64), (48, 64), (19, 32), (96, 33), (64, 96), (33, 132), (96, 128), (66, 96), (132, 12), (64, 132),
    (132, 64), (260, 132), (128, 260)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout", DX_SHAPES)
def test_dense_bwd_dx_layouts(hip, Fin, Fout, layout):
    for i, rows in enumerate(ROWS if layout in ("contig", "pad_nan", "tight") else (129,)):
        check_dx(hip, rows, Fin, Fout, (i + Fout + len(layout)) % 3, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout,kw", [
    (64, 64, dict(wblock=True)), (132, 128, dict(wblock=True)), (32, 19, dict(wblock=True)),
    (48, 64, dict(addend=True)), (132, 132, dict(addend=True, wblock=True))])
def test_dense_bwd_dx_weight_block_and_addend(hip, Fin, Fout, kw, layout):
    check_dx(hip, 129, Fin, Fout, (Fout + len(layout)) % 3, layout, **kw)


DX_LONG = [
    (64, 33, 3 * NUM_CU * 128 + 129),   # linear_mfma_kernel<2, 1, 64>: second trip
    (132, 64, 4096),                    # the smallest row count that transposes W into the workspace
    (132, 64, 3 * NUM_CU * 64 + 65),    # ... and the second trip of gemm_tile_kernel behind it (two column tiles)
    (260, 12, 512 * 128 + 1),           # ... and gemm_tile_x3_kernel behind it
]


@pytest.mark.parametrize("layout", ["contig", "pad_nan"])
@pytest.mark.parametrize("Fin,Fout,rows", DX_LONG)
def test_dense_bwd_dx_second_trip_and_workspace_transpose(hip, Fin, Fout, rows, layout):
    check_dx(hip, rows, Fin, Fout, 1, layout)


# ------------------------------------------------------------------------------------------------------------------
# dW, db
# ------------------------------------------------------------------------------------------------------------------
class Dw:
    def __init__(self, hip, rows, Fin, Fout, act, dwblock=False, seed=0):
        self.hip, self.rows, self.Fin, self.Fout, self.act, self.dwblock = hip, rows, Fin, Fout, act, dwblock
        self.dy = randn(rows, Fout, seed=seed + 1)
        self.x = randn(rows, Fin, seed=seed + 2)
        self.a = torch.tensor([0.25], device=DEV)
        ax = act64(self.x.double(), act, 0.25)
        self.ref = self.dy.double().t() @ ax
        self.tol = (rows + 3) * U * (self.dy.double().abs().t() @ ax.abs())
        self.ref_db = self.dy.double().sum(0)
        self.tol_db = (rows + 3) * U * self.dy.double().abs().sum(0)

    def run(self, layout, fill, DW=None, db=None, acc=0):
        h, L = self.hip, self.hip.lib()
        DY, X = lay(self.dy, layout, fill), lay(self.x, layout, fill)
        if DW is None:
            DW = Rows(self.Fout, self.Fin, "colblock" if self.dwblock else "contig", SENT, "out")
            db = torch.full((self.Fout,), SENT, device=DEV)
        ws = h.workspace(L.gcl_linear_bwd_ws_bytes(self.rows, self.Fin, self.Fout), DEV)
        rc = L.gcl_dense_bwd_dw(DY.ptr, DY.ld, X.ptr, X.ld, self.act, self.a.data_ptr() if self.act == 1 else None,
                                DW.ptr, DW.ld, db.data_ptr(), self.rows, self.Fin, self.Fout, acc, ws.data_ptr(),
                                ws.numel(), h._stream())
        return rc, DY, X, DW, db


def check_dw(hip, rows, Fin, Fout, act, layout, **kw):
    p = Dw(hip, rows, Fin, Fout, act, seed=3 * Fin + Fout, **kw)
    what = f"dw rows={rows} Fin={Fin} Fout={Fout} act={act} {layout} {kw}"
    (rc, DY, X, DW, db), names = launched(lambda: p.run(layout, NAN))
    hip._check(rc)
    ran(names, expect_dw(Fin, Fout, DY, X), what)
    assert DW.untouched(SENT), f"{what}: wrote outside dW[:, :Fin]"
    rc0, _, _, DW0, db0 = p.run(layout, 0.0)
    hip._check(rc0)
    assert same_bits(DW.view, DW0.view) and same_bits(db, db0), f"{what}: NaN padding and zero padding differ"
    within(DW.view, p.ref, p.tol, what + ": dW")
    within(db, p.ref_db, p.tol_db, what + ": db")
    # accumulate: the kernels are deterministic, so a second identical call adds the identical sums
    dw1, db1 = DW.view.clone(), db.clone()
    hip._check(p.run(layout, NAN, DW, db, acc=1)[0])
    assert torch.equal(DW.view, 2 * dw1) and torch.equal(db, 2 * db1), f"{what}: accumulate did not add"
    assert DW.untouched(SENT)


DW_SHAPES = [  # Fin, Fout
    (12, 19), (19, 32), (33, 64), (64, 33), (96, 66), (48, 132), (128, 48), (132, 64), (260, 12), (66, 260)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout", DW_SHAPES)
def test_dense_bwd_dw_layouts(hip, Fin, Fout, layout):
    """gcl_dense_bwd_dw: 16-byte and element loads, one to three 128-column input chunks (Fin = 132, 260), more than
    256 outputs (Fout = 260: two launches); rows = 257 gives a block more than one 64-row step."""
    for i, rows in enumerate(ROWS if layout in ("contig", "pad_nan", "tight") else (129,)):
        check_dw(hip, rows, Fin, Fout, (i + Fin + len(layout)) % 3, layout)


@pytest.mark.parametrize("layout", ["contig", "pad_nan", "odd_ld"])
@pytest.mark.parametrize("Fin,Fout", [(19, 32), (64, 64), (132, 33)])
def test_dense_bwd_dw_into_column_block(hip, Fin, Fout, layout):
    """dW as a column block of a wider gradient (lddw > Fin): the columns beside it stay as they were."""
    check_dw(hip, 129, Fin, Fout, 1, layout, dwblock=True)


@pytest.mark.parametrize("layout", ["contig", "pad_nan"])
def test_dense_bwd_dw_past_block_cap(hip, layout):
    """More rows than 512 blocks of two 64-row steps: every block walks a longer range."""
    check_dw(hip, 512 * 128 + 129, 64, 64, 1, layout)


# ------------------------------------------------------------------------------------------------------------------
# The whole backward in one call
# ------------------------------------------------------------------------------------------------------------------
class All:
    def __init__(self, hip, rows, Fin, Fout, prelu, seed=0):
        self.hip, self.rows, self.Fin, self.Fout, self.prelu = hip, rows, Fin, Fout, prelu
        self.dy, self.x = randn(rows, Fout, seed=seed + 1), randn(rows, Fin, seed=seed + 2)
        self.W = randn(Fout, Fin, seed=seed + 3) * 0.3
        self.a = torch.tensor([0.25], device=DEV)
        act = 1 if prelu else 0
        xd, dyd, Wd = self.x.double(), self.dy.double(), self.W.double()
        ax, d = act64(xd, act, 0.25), dact64(xd, act, 0.25)
        g = dyd @ Wd
        self.dx, self.tol_dx = g * d, (Fout + 3) * U * (dyd.abs() @ Wd.abs()) * d.abs()
        self.dW, self.tol_dW = dyd.t() @ ax, (rows + 3) * U * (dyd.abs().t() @ ax.abs())
        self.db, self.tol_db = dyd.sum(0), (rows + 3) * U * dyd.abs().sum(0)
        # the kernel sums its own dx: every term carries that element's bound, the sum its own rounding
        self.cs, self.tol_cs = self.dx.sum(0), (rows + 3) * U * self.dx.abs().sum(0) + self.tol_dx.sum(0)
        self.dslope = float((g * xd)[xd <= 0].sum()) if prelu else 0.0

    def run(self, layout, fill_x, bits=0, pre=SENT, with_db=True, with_cs=True):
        """dy's padding is zero where Fout % 4 != 0 (the documented exception of gcl_linear_bwd_all: it must be finite),
        else NaN like everything else."""
        h, L = self.hip, self.hip.lib()
        fill_dy = 0.0 if self.Fout % 4 else fill_x
        DY, X = lay(self.dy, layout, fill_dy), lay(self.x, layout, fill_x)
        DX = out_like(self.rows, self.Fin, layout)
        dW = torch.full((self.Fout, self.Fin), pre, device=DEV)
        db, cs = torch.full((self.Fout,), pre, device=DEV), torch.full((self.Fin,), pre, device=DEV)
        ds = torch.full((1,), 0.125, device=DEV)
        ws = h.workspace(L.gcl_linear_bwd_all_ws_bytes(self.rows, self.Fin, self.Fout), DEV)
        rc = L.gcl_linear_bwd_all(DY.ptr, DY.ld, self.W.data_ptr(), X.ptr, X.ld, self.a.data_ptr() if self.prelu else None,
                                  ds.data_ptr() if self.prelu else None, DX.ptr, DX.ld, dW.data_ptr(),
                                  db.data_ptr() if with_db else None, cs.data_ptr() if with_cs else None, self.rows,
                                  self.Fin, self.Fout, bits, ws.data_ptr(), ws.numel(), h._stream())
        return rc, DY, X, DX, dW, db, cs, ds


def check_all(hip, rows, Fin, Fout, prelu, layout, x3=True, bit_sets=(5, 2)):
    p = All(hip, rows, Fin, Fout, prelu, seed=5 * Fin + Fout)
    what = f"bwd_all rows={rows} Fin={Fin} Fout={Fout} prelu={prelu} {layout}"
    (rc, DY, X, DX, dW, db, cs, ds), names = launched(lambda: p.run(layout, NAN))
    hip._check(rc)
    want = expect_all(rows, Fin, Fout, DY, X, DX, x3)
    if want is None:
        ran(names, expect_dw(Fin, Fout, DY, X), what + " (separate kernels)")
        ran(names, expect_dx(rows, Fin, Fout, DY, Fin, False), what + " (separate kernels)")
        assert any("colsum_kernel" in n for n in names) and not any("fused" in n or "x3_bwd" in n for n in names), names
    else:
        ran(names, want, what)
    assert DX.untouched(SENT), f"{what}: wrote outside dx[:, :Fin]"
    rc0, _, _, DX0, dW0, db0, cs0, ds0 = p.run(layout, 0.0)
    hip._check(rc0)
    for a, b, name in ((DX.view, DX0.view, "dx"), (dW, dW0, "dW"), (db, db0, "db"), (cs, cs0, "colsum"), (ds, ds0, "d_slope")):
        assert same_bits(a, b), f"{what}: {name} differs between NaN padding and zero padding"
    within(DX.view, p.dx, p.tol_dx, what + ": dx")
    within(dW, p.dW, p.tol_dW, what + ": dW")
    within(db, p.db, p.tol_db, what + ": db")
    within(cs, p.cs, p.tol_cs, what + ": colsum_dx vs float64")
    if prelu:
        slope_ok(ds.item(), 0.125 + p.dslope, what)
    # one accumulate bit per destination: a set bit adds into 3.0, a clear bit overwrites it
    for bits in bit_sets:
        rc, _, _, DXb, dWb, dbb, csb, _ = p.run(layout, NAN, bits=bits, pre=3.0)
        hip._check(rc)
        assert same_bits(DXb.view, DX.view)
        for t, ref, tol, bit, name in ((dWb, p.dW, p.tol_dW, 1, "dW"), (dbb, p.db, p.tol_db, 2, "db"),
                                       (csb, p.cs, p.tol_cs, 4, "colsum_dx")):
            add = 3.0 if bits & bit else 0.0
            within(t, ref + add, tol + U * (ref.abs() + add), f"{what}: {name} with accumulate = {bits}")
    # without db and colsum_dx: nothing is written through the absent pointers' neighbours
    rc, _, _, DXn, dWn, dbn, csn, _ = p.run(layout, NAN, with_db=False, with_cs=False)
    hip._check(rc)
    assert same_bits(DXn.view, DX.view)
    within(dWn, p.dW, p.tol_dW, what + ": dW without db and colsum_dx")  # (the final pass may sum in another order)
    assert bool((dbn == SENT).all()) and bool((csn == SENT).all())


ALL_SHAPES = [  # Fin, Fout
    (12, 19), (32, 64), (48, 33), (64, 64), (64, 19), (36, 32), (96, 48), (96, 33), (72, 19), (19, 32), (128, 64),
    (64, 96)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("Fin,Fout", ALL_SHAPES)
def test_linear_bwd_all_layouts(hip, Fin, Fout, layout):
    """gcl_linear_bwd_all: the split-operand fused kernel (Fin 33..64 on 16-byte rows, dx included), the 64-row fused
    kernel behind it (dx on scalar rows: "mixed"), the 128-row fused kernel (Fin <= 32 or 65..96), and the three
    separate kernels where fused_ok says no (scalar rows of dy or x, Fin % 4 != 0, Fin > 96, Fout > 64)."""
    for i, rows in enumerate(ROWS if layout in ("contig", "pad_nan", "tight") else (129,)):
        check_all(hip, rows, Fin, Fout, (i + Fin // 4 + len(layout)) % 2 == 0, layout)


@pytest.mark.parametrize("layout", ["contig", "pad_nan", "tight", "colblock"])
@pytest.mark.parametrize("Fin,Fout", [(64, 64), (48, 33), (36, 19)])
def test_linear_bwd_all_fused64_with_x3_off(hip, x3_off, Fin, Fout, layout):
    check_all(hip, 257, Fin, Fout, True, layout, x3=False)


@pytest.mark.parametrize("Fin,Fout,layout", [(64, 64, "pad_nan"), (96, 48, "pad_nan"), (64, 33, "tight"), (128, 64, "contig")])
def test_linear_bwd_all_every_accumulate_mask(hip, Fin, Fout, layout):
    check_all(hip, 129, Fin, Fout, True, layout, bit_sets=tuple(range(1, 8)))


ALL_LONG = [
    (64, 64, 2 * NUM_CU * 64 + 65, True),    # linear_x3_bwd_kernel: 2 blocks per CU, 64-row tiles
    (64, 33, 3 * NUM_CU * 64 + 65, False),   # linear_bwd_fused64_kernel: 3 blocks per CU
    (96, 48, NUM_CU * 128 + 129, True),      # linear_bwd_fused_kernel: one block per CU, 128-row tiles
]


@pytest.mark.parametrize("layout", ["contig", "pad_nan"])
@pytest.mark.parametrize("Fin,Fout,rows,x3", ALL_LONG)
def test_linear_bwd_all_second_trip(hip, monkeypatch, Fin, Fout, rows, x3, layout):
    if not x3:
        monkeypatch.setenv("GCL_X3", "0")
    check_all(hip, rows, Fin, Fout, True, "tight" if layout == "pad_nan" and Fout % 4 else layout, x3=x3, bit_sets=(7,))


# ------------------------------------------------------------------------------------------------------------------
# The cases above reach every instance they are there for (checked on import, GPU or not)
# ------------------------------------------------------------------------------------------------------------------
def _reached():
    seen = set()

    def add(w):
        if w not in (None, EINVAL):
            seen.add((w[0],) + tuple(w[1]))
        else:
            seen.add(w)

    row_sets = lambda lay_: ROWS if lay_ in ("contig", "pad_nan", "tight") else (129,)  # noqa: E731
    g = Geom
    for Fin, Fout in FWD_SHAPES:
        for lay_ in LAYOUTS:
            for i, rows in enumerate(row_sets(lay_)):
                add(expect_fwd(rows, Fin, Fout, g(Fin, lay_), g(Fout, lay_, "out"), Fin, False, (i + Fin + len(lay_)) % 3))
    for Fin, Fout, rows, _ in FWD_LONG:
        add(expect_fwd(rows, Fin, Fout, g(Fin, "contig"), g(Fout, "contig", "out"), Fin, False, 1))
    add(expect_fwd(129, 64, 64, g(64, "contig"), g(64, "contig", "out"), 76, False, 0))
    for Fin, Fout in DX_SHAPES:
        for lay_ in LAYOUTS:
            add(expect_dx(129, Fin, Fout, g(Fout, lay_), Fin, False))
    for Fin, Fout, rows in DX_LONG:
        add(expect_dx(rows, Fin, Fout, g(Fout, "contig"), Fin, False))
    for Fin, Fout in DW_SHAPES:
        for lay_ in LAYOUTS:
            add(expect_dw(Fin, Fout, g(Fout, lay_), g(Fin, lay_)))
    for Fin, Fout in ALL_SHAPES:
        for lay_ in LAYOUTS:
            add(expect_all(129, Fin, Fout, g(Fout, lay_), g(Fin, lay_), g(Fin, lay_, "out")))
    add(expect_all(129, 64, 64, g(64, "contig"), g(64, "contig"), g(64, "contig", "out"), x3=False))
    return seen


def _required():
    req = {None, EINVAL}  # the three-kernel fallback of gcl_linear_bwd_all; a refusal
    req |= {("linear_x3_fwd_kernel", ns, silu, nks) for ns in "12" for nks in "24" for silu in ("false", "true")}
    req |= {("linear_mfma_kernel", ns, "0", "64", v) for ns in "1248" for v in ("true", "false")}
    req |= {("linear_mfma_kernel", "2", epi, kt, "true") for epi in "01" for kt in ("64", "128", "256")}
    req |= {("linear_mfma_kernel", "2", epi, "128", "false") for epi in "01"}
    req |= {("linear_mfma_kernel", ns, "1", "64", "false") for ns in "124"}
    req |= {("gemm_tile_kernel", epi, tr, "1") for epi, tr in (("0", "false"), ("1", "true"), ("1", "false"))}
    req |= {("gemm_tile_x3_kernel", "0"), ("gemm_tile_x3_kernel", "1")}
    req |= {("dw_mfma_kernel", no, nc, v) for no, nc in (("1", "1"), ("2", "2"), ("4", "3"), ("2", "4"), ("8", "3"))
            for v in ("true", "false")}
    req |= {("linear_x3_bwd_kernel", "1"), ("linear_x3_bwd_kernel", "2"), ("linear_bwd_fused64_kernel", "2")}
    req |= {("linear_bwd_fused_kernel", no, nc) for no, nc in (("1", "1"), ("2", "1"), ("1", "3"), ("2", "3"))}
    return req


_missing = _required() - _reached()
assert not _missing, f"no case of this module reaches {sorted(map(str, _missing))}"
