"""What VALUES the hot-path kernels carry, beside where they read and write (the layout files): non-finite data, and
data far from order one.

A. Containment.  Every operation runs twice on the same operands, clean and with ONE element replaced by NaN (by +inf
   where said).  The poisoned run must be finite exactly where a float64 restatement of the operation is finite, and
   BIT-equal to the clean run there (tests/helpers/poison.py::contained); at least half of all output elements stay
   finite in the reference, and the sentinels around the outputs stay.  A mask done by multiplying with zero, a row
   table that reads a row nobody asked for, a tile that mixes the rows of two samples: each passes the layout files and
   fails here.  The poisoned rows are row 0, the middle of a 64-row tile, the last row and, with a batch, the first
   row of sample 1.
B. Power-of-two scale covariance.  A kernel that is linear in an operand must scale its output by exactly 2^k when the
   operand (and the additive terms) are scaled by 2^k, k = -48, -24, 24, 48, bit for bit, while everything stays a
   normal fp32 number: the arithmetic of csrc/x3.h (exact pieces, exact piece products, fp32 sums) and of an fp32 FMA
   chain implies it.  The data are sign * [0.5, 2), so that the smallest piece product at 2^-48 x 2^-48 is 2^-121.
C. The band of the split-operand path (csrc/x3.h, include/gcl.h): a CPU restatement of the split pins
   where x = hi + mid + lo holds exactly; on the GPU every split-operand kernel is held to the float64-arbitrated
   comparison with an fp32 GEMM at the inner edges of the band, and gives finite results for finite operands anywhere
   below 2^127 whose result is inside fp32's range.

Every case names the kernel that ran (torch profiler) and prints it as `ran: ...`.  The tolerances are the project's:
same_bits, `within` with the U-based bounds of test_dense_layouts.py, and the fp32 arbitration of
test_hip_ops.py::test_x3_linear_fwd_is_as_accurate_as_fp32."""
import copy
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as Fn

from oracle import pyg_ops as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, Rows, has, launched, same_bits, targs  # noqa: E402
from poison import (INF, SCALES, as_accurate_as_fp32, contained, covariant, full_significands, poison_rows,  # noqa: E402
                    poisoned, split3, split_is_exact)
from test_dense_layouts import All, Dw, Dx, Fwd, act64, expect_all, expect_dw, expect_dx, expect_fwd, ran  # noqa: E402
from test_sparse_layouts import edges_of, graphs, rnd  # noqa: E402, F401  (graphs: the module-scoped fixture)

gpu = pytest.mark.gpu
ROWS = 129  # two 64-row tiles and a ragged tail of one row
B = 3
A = 0.25  # the PReLU slope of the dense test classes


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def cpu64(t):
    return t.detach().double().cpu()


def col_of(r, F):
    return (7 * r + 3) % F


# ------------------------------------------------------------------------------------------------------------------
# C.1 The split on the CPU
# ------------------------------------------------------------------------------------------------------------------
def test_split_is_exact_inside_the_band_and_not_outside():
    """csrc/x3.h::split2 restated with torch.bfloat16: hi + mid + lo == x for 2^-110 <= |x| < 2^127 and for 0 (24-bit
    significands with the lowest bit set: the worst case), because the last piece lives on bf16's subnormal grid of
    2^-133 = 2^(-110 - 23).  Not at 2^-111 (the lowest bit, 2^-134, is lost), and not at the largest finite fp32, whose
    hi piece rounds to inf and whose other pieces are -inf and NaN."""
    for e in list(range(-110, -100)) + list(range(-100, 127, 9)) + [126]:
        x = full_significands(e, seed=e + 200)
        assert bool(split_is_exact(x).all()), f"the split loses bits at 2^{e}"
    edge = torch.tensor([0.0, -0.0, 2.0 ** -110, -(2.0 ** -110) * (2 - 2.0 ** -23), 2.0 ** 127 - 2.0 ** 103, -(2.0 ** 126)])
    assert bool(split_is_exact(edge).all())
    below = full_significands(-111, seed=1)
    assert not bool(split_is_exact(below).any()), "2^-111 with the lowest bit set cannot be three bf16 pieces"
    res = (below.double() - sum(p.double() for p in split3(below))).abs()
    assert float(res.max()) == 2.0 ** -134, "the residue at 2^-111 is the lost bit (4.6e-41)"
    top = torch.tensor([torch.finfo(torch.float32).max])
    hi, mid, lo = split3(top)
    assert math.isinf(float(hi)) and not math.isfinite(float(mid)) and math.isnan(float(lo))
    assert not bool(split_is_exact(top).any())


# ------------------------------------------------------------------------------------------------------------------
# A. Dense forward
# ------------------------------------------------------------------------------------------------------------------
FWD_FAMILIES = [  # Fin, Fout, GCL_X3 on
    (48, 64, True), (19, 32, True),      # linear_x3_fwd_kernel
    (66, 48, True), (64, 33, True),      # linear_mfma_kernel
    (128, 132, True), (260, 132, True),  # gemm_tile_kernel
    (48, 64, False), (19, 32, False),    # GCL_X3=0: linear_mfma_kernel on the split-operand kernel's shapes
]


def fwd_ref(p):
    return act64(cpu64(p.x), p.act, A) @ cpu64(p.W).t() + cpu64(p.b)


def fwd_run(hip, p, linear_entry=False):
    rc, X, Y, Wl = p.run("pad_nan", NAN, linear_entry=linear_entry)
    hip._check(rc)
    torch.cuda.synchronize()
    assert Y.untouched(SENT), "wrote outside y[:, :Fout]"
    return X, Y, Wl


@gpu
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("Fin,Fout,x3", FWD_FAMILIES)
def test_dense_fwd_contains_a_poisoned_element(hip, monkeypatch, Fin, Fout, x3, act):
    """gcl_dense_fwd (and gcl_linear_fwd where it is the same call): NaN in x reaches one row of y, +inf in x too, NaN in
    the bias one column, NaN in one row of W one column."""
    if not x3:
        monkeypatch.setenv("GCL_X3", "0")
    p = Fwd(hip, ROWS, Fin, Fout, act, seed=Fin + Fout)
    what = f"fwd {Fin}->{Fout} act={act} x3={x3}"
    (X, Y, Wl), names = launched(lambda: fwd_run(hip, p))
    ran(names, expect_fwd(ROWS, Fin, Fout, X, Y, Wl.ld, False, act, x3), what)
    clean = Y.view.clone()
    x0, W0, b0 = p.x, p.W, p.b
    mid = poison_rows(ROWS)[1]
    cases = [("x", (r, col_of(r, Fin)), NAN) for r in poison_rows(ROWS)]
    cases += [("x", (mid, Fin - 1), INF), ("b", (Fout // 2,), NAN), ("W", (Fout - 1, Fin // 2), NAN)]
    for name, idx, val in cases:
        p.x, p.W, p.b = x0, W0, b0
        setattr(p, name, poisoned(getattr(p, name), idx, val))
        _, Yp, _ = fwd_run(hip, p)
        contained(clean, Yp.view, fwd_ref(p), f"{what}: {val} in {name}{list(idx)}")
    if act < 2 and Fin in (48, 19):  # gcl_linear_fwd: PReLU when a slope is given
        _, Yl, _ = fwd_run(hip, p, linear_entry=True)
        contained(clean, Yl.view, fwd_ref(p), f"{what}: gcl_linear_fwd, NaN in W")


# ------------------------------------------------------------------------------------------------------------------
# A. Dense backward
# ------------------------------------------------------------------------------------------------------------------
def bwd_ref(x, W, dy, act):
    """float64 autograd on the CPU of y = act(x) W^T: dx, dW, db, column sums of dx, slope gradient."""
    x64, W64 = cpu64(x).requires_grad_(), cpu64(W).requires_grad_()
    a = torch.tensor([A], dtype=torch.float64, requires_grad=True)
    ax = x64 if act == 0 else Fn.prelu(x64, a) if act == 1 else Fn.silu(x64)
    (ax @ W64.t()).backward(cpu64(dy))
    ds = a.grad if act == 1 else torch.zeros(1, dtype=torch.float64)
    return {"dx": x64.grad, "dW": W64.grad, "db": cpu64(dy).sum(0), "cs": x64.grad.sum(0), "ds": 0.125 + ds}


def negative_at(x, idx):
    """x with a negative value at idx: PReLU' is the slope there with the clean value and with NaN (NaN > 0 is false),
    so the reference leaves dx finite at a poisoned x and it must keep the clean run's bits."""
    x = x.clone()
    x[idx] = -x[idx].abs() - 0.5
    return x


ALL_CASES = [  # Fin, Fout, prelu, GCL_X3 on, with colsum_dx -> the kernel
    (64, 64, True, True, True, ("linear_x3_bwd_kernel", ["2"])),
    (48, 33, False, True, True, ("linear_x3_bwd_kernel", ["2"])),
    (64, 64, True, True, False, ("linear_x3_bwd_lean_kernel", ["2", "true", "true", "false", "false"])),
    (48, 33, False, True, False, ("linear_x3_bwd_lean_kernel", ["2", "false", "true", "false", "true"])),
    (64, 64, True, False, True, ("linear_bwd_fused64_kernel", ["2"])),
    (96, 48, True, True, True, ("linear_bwd_fused_kernel", ["2", "3"])),
    (32, 64, False, True, True, ("linear_bwd_fused_kernel", ["2", "1"])),
    (128, 64, True, True, True, None),  # the three separate kernels
]


def all_run(hip, p, with_cs):
    rc, DY, X, DX, dW, db, cs, ds = p.run("tight", NAN, with_cs=with_cs)
    hip._check(rc)
    torch.cuda.synchronize()
    assert DX.untouched(SENT), "wrote outside dx[:, :Fin]"
    assert with_cs or bool((cs == SENT).all())
    outs = {"dx": DX.view, "dW": dW, "db": db, "cs": cs, "ds": ds}
    keys = ["dx", "dW", "db"] + (["cs"] if with_cs else []) + (["ds"] if p.prelu else [])
    return (DY, X, DX), keys, [outs[k] for k in keys]


@gpu
@pytest.mark.parametrize("Fin,Fout,prelu,x3,with_cs,want", ALL_CASES)
def test_linear_bwd_all_contains_a_poisoned_element(hip, monkeypatch, Fin, Fout, prelu, x3, with_cs, want):
    """gcl_linear_bwd_all on each of its kernels: NaN in dy[r, o] reaches row r of dx, row o of dW, db[o] and what the
    reference says of the column sums and the slope gradient; NaN in x[r, c] reaches column c of dW and the slope
    gradient, and dx only through the activation's derivative."""
    if not x3:
        monkeypatch.setenv("GCL_X3", "0")
    p = All(hip, ROWS, Fin, Fout, prelu, seed=5 * Fin + Fout)
    mid = poison_rows(ROWS)[1]
    xi = (mid, col_of(mid, Fin))
    p.x = negative_at(p.x, xi)
    what = f"bwd_all {Fin}->{Fout} prelu={prelu} x3={x3} colsum={with_cs}"
    ((DY, X, DX), keys, clean), names = launched(lambda: all_run(hip, p, with_cs))
    if want is None:
        assert expect_all(ROWS, Fin, Fout, DY, X, DX, x3) is None
        ran(names, expect_dw(Fin, Fout, DY, X), what + " (separate kernels)")
        ran(names, expect_dx(ROWS, Fin, Fout, DY, Fin, False), what + " (separate kernels)")
        assert not any("fused" in n or "x3_bwd" in n for n in names), names
    else:
        ran(names, want, what)
    clean = [t.clone() for t in clean]
    dy0, x0 = p.dy, p.x
    for name, idx in [("dy", (r, col_of(r, Fout))) for r in poison_rows(ROWS)] + [("x", xi)]:
        p.dy, p.x = dy0, x0
        setattr(p, name, poisoned(getattr(p, name), idx))
        _, _, got = all_run(hip, p, with_cs)
        ref = bwd_ref(p.x, p.W, p.dy, 1 if prelu else 0)
        contained(clean, got, [ref[k] for k in keys], f"{what}: NaN in {name}{list(idx)} {keys}")


@gpu
def test_deferred_reduction_contains_a_poisoned_element(hip):
    """The same through gcl_linear_bwd_all_deferred + gcl_reduce_jobs: 65 blocks of partial records, summed later."""
    rows, Fin, Fout = 64 * 64 + 1, 64, 64
    p = All(hip, rows, Fin, Fout, True, seed=11)
    mid = poison_rows(rows)[1]
    xi = (mid, col_of(mid, Fin))
    p.x = negative_at(p.x, xi)

    def run():
        dW, db, cs = (torch.full(s, SENT, device=DEV) for s in ((Fout, Fin), (Fout,), (Fin,)))
        ds = torch.full((1,), 0.125, device=DEV)
        hip.defer_begin()
        try:
            dx = hip.linear_bwd_all(p.dy, p.W, p.x, p.a, ds, dW, db, cs, False)
            assert bool((dW == SENT).all()), "the deferred call reduced on the spot"
            hip.defer_flush()
        finally:
            hip.defer_flush(drop=True)
        torch.cuda.synchronize()
        return [dx, dW, db, cs, ds]

    clean, names = launched(run)
    ran(names, ("linear_x3_bwd_kernel", ["2"]), "deferred bwd_all")
    assert has(names, "reduce_jobs_kernel"), names
    print("ran: reduce_jobs_kernel  [deferred bwd_all]")
    dy0, x0 = p.dy, p.x
    for name, idx in [("dy", (r, col_of(r, Fout))) for r in poison_rows(rows)] + [("x", xi)]:
        p.dy, p.x = dy0, x0
        setattr(p, name, poisoned(getattr(p, name), idx))
        ref = bwd_ref(p.x, p.W, p.dy, 1)
        contained(clean, run(), [ref[k] for k in ("dx", "dW", "db", "cs", "ds")], f"deferred: NaN in {name}{list(idx)}")


@gpu
@pytest.mark.parametrize("Fin,Fout,act", [(64, 33, 1), (64, 33, 2), (260, 132, 1), (260, 132, 2)])
def test_dense_bwd_dx_contains_a_poisoned_element(hip, Fin, Fout, act):
    """gcl_dense_bwd_dx on the panel kernel and on the tile kernel (W^T): NaN in dy[r, o] reaches row r of dx; NaN in z
    reaches what the activation's derivative carries (SiLU: that element; PReLU: nothing of dx, the slope gradient)."""
    p = Dx(hip, ROWS, Fin, Fout, act, seed=Fin + 2 * Fout)
    mid = poison_rows(ROWS)[1]
    zi = (mid, col_of(mid, Fin))
    p.z = negative_at(p.z, zi)
    what = f"dx {Fin}<-{Fout} act={act}"

    def run():
        rc, DY, DX, Wl, ds = p.run("pad_nan", NAN)
        hip._check(rc)
        torch.cuda.synchronize()
        assert DX.untouched(SENT)
        return DY, Wl, [DX.view] + ([ds] if act == 1 else [])

    (DY, Wl, clean), names = launched(run)
    ran(names, expect_dx(ROWS, Fin, Fout, DY, Wl.ld, False), what)
    clean = [t.clone() for t in clean]
    dy0, z0 = p.dy, p.z
    for name, idx in [("dy", (r, col_of(r, Fout))) for r in poison_rows(ROWS)] + [("z", zi)]:
        p.dy, p.z = dy0, z0
        setattr(p, name, poisoned(getattr(p, name), idx))
        ref = bwd_ref(p.z, p.W, p.dy, act)
        contained(clean, run()[2], [ref["dx"]] + ([ref["ds"]] if act == 1 else []), f"{what}: NaN in {name}{list(idx)}")


@gpu
@pytest.mark.parametrize("Fin,Fout,act", [(33, 64, 0), (33, 64, 2), (132, 64, 1)])
def test_dense_bwd_dw_contains_a_poisoned_element(hip, Fin, Fout, act):
    """gcl_dense_bwd_dw: NaN in dy[r, o] reaches row o of dW and db[o]; NaN in x[r, c] column c of dW."""
    p = Dw(hip, ROWS, Fin, Fout, act, seed=3 * Fin + Fout)
    what = f"dw {Fin}x{Fout} act={act}"

    def run():
        rc, DY, X, DW, db = p.run("pad_nan", NAN)
        hip._check(rc)
        torch.cuda.synchronize()
        assert DW.untouched(SENT)
        return DY, X, [DW.view, db]

    (DY, X, clean), names = launched(run)
    ran(names, expect_dw(Fin, Fout, DY, X), what)
    clean = [t.clone() for t in clean]
    dy0, x0 = p.dy, p.x
    mid = poison_rows(ROWS)[1]
    for name, idx in [("dy", (r, col_of(r, Fout))) for r in poison_rows(ROWS)] + [("x", (mid, col_of(mid, Fin)))]:
        p.dy, p.x = dy0, x0
        setattr(p, name, poisoned(getattr(p, name), idx))
        ref = bwd_ref(p.x, torch.zeros(Fout, Fin), p.dy, act)
        contained(clean, run()[2], [ref["dW"], ref["db"]], f"{what}: NaN in {name}{list(idx)}")


# ------------------------------------------------------------------------------------------------------------------
# A. gcl_mlp_fwd_chain
# ------------------------------------------------------------------------------------------------------------------
EPS = 1e-5


def chain_params(widths, seed):
    g = torch.Generator().manual_seed(seed)
    n = len(widths) - 1
    Ws = [(torch.randn(widths[k + 1], widths[k], generator=g) * 0.3).to(DEV) for k in range(n)]
    bs = [torch.randn(widths[k + 1], generator=g).to(DEV) for k in range(n)]
    slopes = [torch.tensor([0.25 - 0.125 * k], device=DEV) for k in range(n - 1)]
    gamma = (1 + 0.1 * torch.randn(widths[-1], generator=g)).to(DEV)
    beta = (0.1 * torch.randn(widths[-1], generator=g)).to(DEV)
    return Ws, bs, slopes, gamma, beta


def chain_ref(x, Ws, bs, slopes, ln):
    """[z_0, .., (y, stats)] in float64 on the CPU."""
    out, cur = [], cpu64(x)
    for k, (W, b) in enumerate(zip(Ws, bs)):
        if k:
            cur = torch.where(cur > 0, cur, cpu64(slopes[k - 1]) * cur)
        cur = cur @ cpu64(W).t() + cpu64(b)
        out.append(cur)
    if ln is not None:
        mean, var = cur.mean(1), cur.var(1, unbiased=False)
        rstd = 1 / torch.sqrt(var + EPS)
        out += [(cur - mean[:, None]) * rstd[:, None] * cpu64(ln[0]) + cpu64(ln[1]), torch.stack([mean, rstd], 1)]
    return out


def chain_run(hip, x, Ws, bs, slopes, ln):
    got = hip.mlp_fwd_chain(x, Ws, bs, slopes, ln=ln)
    assert got is not None, "the chained kernel must take this run"
    zs, y, stats = got
    if ln is not None and y is None:  # three layers: the LayerNorm is a launch of its own
        y, stats = hip.layernorm_fwd(zs[-1], ln[0], ln[1], EPS)
    torch.cuda.synchronize()
    return list(zs) + ([y, stats] if ln is not None else [])


CHAINS = [((64, 64, 64, 64), False), ((64, 64, 64, 64), True), ((48, 48, 64), True), ((64, 48, 36), False)]


@gpu
@pytest.mark.parametrize("widths,has_ln", CHAINS)
def test_mlp_chain_contains_a_poisoned_row(hip, widths, has_ln):
    """mlp_x3_chain_kernel: a NaN in one input row stays that row of every z_k, of y and of the LayerNorm statistics
    (rows pass from layer to layer in LDS; 129 rows are one full 128-row tile and one row of the next)."""
    Ws, bs, slopes, gamma, beta = chain_params(widths, seed=sum(widths))
    ln = (gamma, beta, EPS) if has_ln else None
    x = torch.randn(ROWS, widths[0], generator=torch.Generator().manual_seed(9)).to(DEV)
    what = f"chain {widths} ln={has_ln}"
    clean, names = launched(lambda: chain_run(hip, x, Ws, bs, slopes, ln))
    L = len(widths) - 1
    ran(names, ("mlp_x3_chain_kernel", [str(L), "true" if has_ln and L == 2 else "false"]), what)
    for r in poison_rows(ROWS):
        xp = poisoned(x, (r, col_of(r, widths[0])))
        contained(clean, chain_run(hip, xp, Ws, bs, slopes, ln), chain_ref(xp, Ws, bs, slopes, ln), f"{what}: NaN in x[{r}]")


# ------------------------------------------------------------------------------------------------------------------
# B. Scale covariance of the dense kernels and of the chain
# ------------------------------------------------------------------------------------------------------------------
def unit_range(*shape, seed):
    """sign * [0.5, 2): no element is small enough for a piece product to leave the normal range at 2^-48 x 2^-48."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.5 + 1.5 * torch.rand(*shape, generator=g)
    return (mag * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).to(DEV)


def fwd_scaled(hip, p, x, W, b, kx, kw):
    p.x, p.W, p.b = x * 2.0 ** kx, W * 2.0 ** kw, b * 2.0 ** (kx + kw)
    rc, X, Y, Wl = p.run("pad_nan", NAN)
    hip._check(rc)
    torch.cuda.synchronize()
    return X, Y, Wl


FWD_COVARIANT = FWD_FAMILIES + [(12, 260, True)]  # the last one: gemm_tile_x3_kernel, at its smallest row count
X3_TILE_ROWS = 511 * 128 + 1  # 512 row tiles x 3 column tiles = 1536 = 3 * 2 * 256 tiles: launch_gemm's threshold


@gpu
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("Fin,Fout,x3", FWD_COVARIANT)
def test_dense_fwd_is_scale_covariant(hip, monkeypatch, Fin, Fout, x3, act):
    """y(2^k x, W, 2^k b) = 2^k y(x, W, b), the same for W, and for x and W together at 2^-48 and 2^48, bit for bit."""
    if not x3:
        monkeypatch.setenv("GCL_X3", "0")
    rows = X3_TILE_ROWS if Fout == 260 else ROWS
    p = Fwd(hip, rows, Fin, Fout, act, seed=1)
    x, W, b = unit_range(rows, Fin, seed=Fin), unit_range(Fout, Fin, seed=Fout) / 4, unit_range(Fout, seed=3)
    what = f"fwd {Fin}->{Fout} act={act} x3={x3}"
    (X, Y, Wl), names = launched(lambda: fwd_scaled(hip, p, x, W, b, 0, 0))
    want = expect_fwd(rows, Fin, Fout, X, Y, Wl.ld, False, act, x3)
    assert Fout != 260 or want[0] == "gemm_tile_x3_kernel"
    assert Fout != 260 or expect_fwd(rows - 128, Fin, Fout, X, Y, Wl.ld, False, act, x3)[0] == "gemm_tile_kernel"
    ran(names, want, what)
    base = Y.view.clone()
    for kx, kw in [(k, 0) for k in SCALES] + [(0, k) for k in SCALES] + [(-48, -48), (48, 48)]:
        _, Ys, _ = fwd_scaled(hip, p, x, W, b, kx, kw)
        covariant(base, Ys.view, kx + kw, f"{what}: x * 2^{kx}, W * 2^{kw}")


@gpu
@pytest.mark.parametrize("Fin,Fout,prelu,x3,with_cs,want", ALL_CASES)
def test_linear_bwd_all_is_scale_covariant(hip, monkeypatch, Fin, Fout, prelu, x3, with_cs, want):
    """dy scales dx, dW, db and the column sums; W scales dx and the column sums and leaves dW alone; x (PReLU is
    homogeneous) scales dW and leaves dx alone.  (The slope gradient is added into a destination that does not scale.)"""
    if not x3:
        monkeypatch.setenv("GCL_X3", "0")
    p = All(hip, ROWS, Fin, Fout, prelu, seed=2)
    dy, x, W = unit_range(ROWS, Fout, seed=Fout + 1), unit_range(ROWS, Fin, seed=Fin + 2), unit_range(Fout, Fin, seed=5) / 4
    what = f"bwd_all {Fin}->{Fout} prelu={prelu} x3={x3} colsum={with_cs}"

    def run(kdy, kx, kw):
        p.dy, p.x, p.W = dy * 2.0 ** kdy, x * 2.0 ** kx, W * 2.0 ** kw
        _, keys, outs = all_run(hip, p, with_cs)
        return {k: t.clone() for k, t in zip(keys, outs) if k != "ds"}

    base, names = launched(lambda: run(0, 0, 0))
    if want is not None:
        ran(names, want, what)
    else:
        print(f"ran: dw_mfma_kernel + the dx kernel + colsum_kernel  [{what}]")
        assert has(names, "dw_mfma_kernel") and has(names, "colsum_kernel"), names
    combos = [(k, 0, 0) for k in SCALES] + [(0, k, 0) for k in SCALES] + [(0, 0, k) for k in SCALES]
    combos += [(-48, -48, 0), (48, 48, 0), (-48, 0, -48), (48, 0, 48)]
    for kdy, kx, kw in combos:
        got = run(kdy, kx, kw)
        exps = {"dx": kdy + kw, "dW": kdy + kx, "db": kdy, "cs": kdy + kw}
        for key, t in got.items():
            covariant(base[key], t, exps[key], f"{what}: dy * 2^{kdy}, x * 2^{kx}, W * 2^{kw}: {key}")


@gpu
@pytest.mark.parametrize("Fin,Fout,act", [(64, 33, 1), (260, 132, 0)])
def test_dense_bwd_dx_and_dw_are_scale_covariant(hip, Fin, Fout, act):
    """gcl_dense_bwd_dx (panel and tile kernel) and gcl_dense_bwd_dw on their own."""
    px, pw = Dx(hip, ROWS, Fin, Fout, act, seed=1), Dw(hip, ROWS, Fin, Fout, act, seed=1)
    dy, x, W = unit_range(ROWS, Fout, seed=Fout + 1), unit_range(ROWS, Fin, seed=Fin + 2), unit_range(Fout, Fin, seed=5) / 4
    px.z = pw.x = x

    def run(kdy, kw):
        px.dy, px.W, pw.dy = dy * 2.0 ** kdy, W * 2.0 ** kw, dy * 2.0 ** kdy
        rc, DY, DX, Wl, _ = px.run("pad_nan", NAN)
        hip._check(rc)
        rc, DY2, X2, DW, db = pw.run("pad_nan", NAN)
        hip._check(rc)
        torch.cuda.synchronize()
        return (DY, Wl, X2), [DX.view.clone(), DW.view.clone(), db.clone()]

    ((DY, Wl, X2), base), names = launched(lambda: run(0, 0))
    ran(names, expect_dx(ROWS, Fin, Fout, DY, Wl.ld, False), "dx")
    ran(names, expect_dw(Fin, Fout, DY, X2), "dw")
    for kdy, kw in [(k, 0) for k in SCALES] + [(0, k) for k in SCALES] + [(-48, -48), (48, 48)]:
        got = run(kdy, kw)[1]
        for t0, t, e, key in zip(base, got, (kdy + kw, kdy, kdy), ("dx", "dW", "db")):
            covariant(t0, t, e, f"{Fin}<-{Fout} act={act}: dy * 2^{kdy}, W * 2^{kw}: {key}")


@gpu
@pytest.mark.parametrize("widths", [(64, 64, 64, 64), (64, 48, 36)])
def test_mlp_chain_is_scale_covariant(hip, widths):
    """The chain without LayerNorm is linear in x with every bias scaled along (PReLU is homogeneous), and in each W_k
    with the biases from layer k on scaled along."""
    n = len(widths) - 1
    x = unit_range(ROWS, widths[0], seed=1)
    Ws = [unit_range(widths[k + 1], widths[k], seed=10 + k) / 8 for k in range(n)]
    bs = [unit_range(widths[k + 1], seed=20 + k) for k in range(n)]
    slopes = [torch.tensor([0.25 / (k + 1)], device=DEV) for k in range(n - 1)]
    what = f"chain {widths}"

    def run(kx, kw, layer=0):
        Wk = [W * 2.0 ** (kw if k == layer else 0) for k, W in enumerate(Ws)]
        bk = [b * 2.0 ** (kx + (kw if k >= layer else 0)) for k, b in enumerate(bs)]
        return chain_run(hip, x * 2.0 ** kx, Wk, bk, slopes, None)

    base, names = launched(lambda: run(0, 0))
    ran(names, ("mlp_x3_chain_kernel", [str(n), "false"]), what)
    for k in SCALES:
        covariant(base, run(k, 0), k, f"{what}: x * 2^{k}")
        for layer in range(n):
            got = run(0, k, layer)
            for j, (t0, t) in enumerate(zip(base, got)):
                covariant(t0, t, k if j >= layer else 0, f"{what}: W_{layer} * 2^{k}: z_{j}")
    for k in (-48, 48):
        covariant(base, run(k, k), 2 * k, f"{what}: x * 2^{k} and W_0 * 2^{k}")


# ------------------------------------------------------------------------------------------------------------------
# A. LayerNorm and GraphNorm
# ------------------------------------------------------------------------------------------------------------------
def ln_ref(x, gm, bt, dy):
    """float64 autograd of the node LayerNorm: y, (mean, rstd), dx, dgamma, dbeta, column sums of dx."""
    x64, g64, b64 = cpu64(x).requires_grad_(), cpu64(gm).requires_grad_(), cpu64(bt).requires_grad_()
    y = Fn.layer_norm(x64, (x.shape[1],), g64, b64, EPS)
    y.backward(cpu64(dy))
    xd = x64.detach()
    stats = torch.stack([xd.mean(1), 1 / torch.sqrt(xd.var(1, unbiased=False) + EPS)], 1)
    return [y.detach(), stats], [x64.grad, g64.grad, b64.grad, x64.grad.sum(0)]


def ln_operands(rows, F):
    g = torch.Generator().manual_seed(F)
    x = (torch.randn(rows, F, generator=g) * 1.5 + 0.3).to(DEV)
    dy = torch.randn(rows, F, generator=g).to(DEV)
    return x, dy, (torch.rand(F, generator=g) + 0.5).to(DEV), torch.randn(F, generator=g).to(DEV)


@gpu
@pytest.mark.parametrize("F", [64, 33])
def test_layernorm_contains_a_poisoned_row(hip, F):
    """gcl_layernorm_fwd / gcl_layernorm_bwd_cs (16-byte rows and scalar rows): NaN in x[r] reaches row r of y, of the
    statistics and of dx, and dgamma and the column sums of dx; NaN in dy[r, c] reaches row r of dx, dgamma[c], dbeta[c]
    and the column sums."""
    x, dy, gm, bt = ln_operands(ROWS, F)

    def run(x, dy):
        y, stats = hip.layernorm_fwd(x, gm, bt, EPS)
        dg, db, cs = (torch.full((F,), SENT, device=DEV) for _ in range(3))
        dx = hip.layernorm_bwd(dy, x, gm, stats, dg, db, False, colsum_dx=cs)
        torch.cuda.synchronize()
        return [y, stats, dx, dg, db, cs]

    clean, names = launched(lambda: run(x, dy))
    assert has(names, "ln_fwd_kernel") and has(names, "ln_bwd_kernel"), names
    print(f"ran: ln_fwd_kernel<{', '.join(targs(names, 'ln_fwd_kernel')[0])}> + ln_bwd_kernel  [layernorm F={F}]")
    for r in poison_rows(ROWS):
        for name in ("x", "dy"):
            xp, dyp = (poisoned(x, (r, col_of(r, F))), dy) if name == "x" else (x, poisoned(dy, (r, col_of(r, F))))
            fwd, bwd = ln_ref(xp, gm, bt, dyp)
            contained(clean, run(xp, dyp), fwd + bwd, f"layernorm F={F}: NaN in {name}[{r}]")


@gpu
@pytest.mark.parametrize("skip", [False, True])
def test_mapped_layernorm_contains_a_poisoned_row(hip, skip):
    """gcl_layernorm_fwd_map / _bwd_map and the _skip forms, B = 3 samples of 43 rows (a 64-row tile spans two samples),
    the output rows placed through a map that drops every third row.  NaN in a kept row of x reaches that row; in the
    _skip forms NaN in a DROPPED row reaches nothing at all (its statistics and its dx are not written: not compared)."""
    n, F, m = 43, 64, 40
    rows = B * n
    x, _, gm, bt = ln_operands(rows, F)
    keep = torch.arange(n) % 3 != 1
    pos = torch.full((n,), -1, dtype=torch.int32)
    pos[keep] = (2 + torch.randperm(int(keep.sum()), generator=torch.Generator().manual_seed(1))).to(torch.int32)
    pos_d, rlist = pos.to(DEV), torch.nonzero(keep).flatten().to(torch.int32).to(DEV)
    kept_rows = keep.repeat(B)
    src3 = torch.randn(B, m, F + 4, generator=torch.Generator().manual_seed(2)).to(DEV)
    dyd = torch.zeros(B, n, F, device=DEV)
    dyd[:, keep.to(DEV)] = src3[:, pos[keep].long().to(DEV), :F]

    def run(x):
        out3 = torch.full((B, m, F + 4), SENT, device=DEV)
        if skip:
            st = hip.layernorm_fwd_map_skip(x, gm, bt, EPS, out3, pos_d, rlist)
        else:
            st = hip.layernorm_fwd_map(x, gm, bt, EPS, out3, pos_d)
        dg, db, cs = (torch.full((F,), SENT, device=DEV) for _ in range(3))
        dx = hip.layernorm_bwd(None, x, gm, st, dg, db, False, colsum_dx=cs, dy_map=(src3, pos_d), skip=skip)
        torch.cuda.synchronize()
        written = torch.zeros(B, m, F + 4, dtype=torch.bool, device=DEV)
        written[:, pos[keep].long().to(DEV), :F] = True
        assert bool((out3[~written] == SENT).all()), "the mapped forward wrote outside the mapped rows"
        y = out3[:, pos[keep].long().to(DEV), :F]
        if skip:  # the dropped rows' statistics and dx are not written
            return [y, st[kept_rows.to(DEV)], dx[kept_rows.to(DEV)], dg, db, cs]
        return [y, st, dx, dg, db, cs]

    def ref(x):
        if skip:  # the dropped rows do not exist: whatever they hold, the result is that of zeros there
            x = x.clone()
            x[(~kept_rows).to(DEV)] = 0.0
        (y, st), (dx, dg, db, cs) = ln_ref(x, gm, bt, dyd.view(rows, F))
        y = y.view(B, n, F)[:, keep]
        if skip:
            return [y, st[kept_rows], dx[kept_rows], dg, db, dx[kept_rows].sum(0)]
        return [y, st, dx, dg, db, cs]

    clean, names = launched(lambda: run(x))
    assert has(names, "ln_fwd_kernel") and has(names, "ln_bwd_kernel"), names
    print(f"ran: ln_fwd_kernel<{', '.join(targs(names, 'ln_fwd_kernel')[0])}> + ln_bwd_kernel<"
          f"{', '.join(targs(names, 'ln_bwd_kernel')[0])}>  [mapped layernorm skip={skip}]")
    kept_i, dropped_i = [i for i in range(n) if keep[i]], [i for i in range(n) if not keep[i]]
    cases = [(0, kept_i[0]), (1, kept_i[0]), (1, kept_i[len(kept_i) // 2]), (B - 1, kept_i[-1])]
    if skip:
        cases += [(1, dropped_i[0]), (B - 1, dropped_i[-1])]
    for b, i in cases:
        xp = poisoned(x, (b * n + i, col_of(i, F)))
        want = ref(xp)
        if skip and not keep[i]:
            assert all(bool(torch.isfinite(t).all()) for t in want)
        contained(clean, run(xp), want, f"mapped layernorm skip={skip}: NaN in x[{b}, {i}] (kept: {bool(keep[i])})")


@gpu
def test_graphnorm_contains_a_poisoned_sample(hip):
    """gcl_graphnorm_fwd / _bwd: NaN in one element of x reaches that sample's y, statistics and dx (and dgamma, a sum
    over all samples); NaN in dy reaches that sample's dx and one element of dgamma and dbeta."""
    n, F = 43, 64
    g = torch.Generator().manual_seed(3)
    x, dy = (torch.randn(B, n, F, generator=g) * 2 + 0.5).to(DEV), torch.randn(B, n, F, generator=g).to(DEV)
    gm, bt = (torch.rand(F, generator=g) + 0.5).to(DEV), torch.randn(F, generator=g).to(DEV)

    def run(x, dy):
        y, stats = hip.graphnorm_fwd(x, gm, bt)
        dg, db = torch.full((F,), SENT, device=DEV), torch.full((F,), SENT, device=DEV)
        dx = hip.graphnorm_bwd(dy, x, gm, stats, dg, db, False)
        torch.cuda.synchronize()
        return [y, stats, dx, dg, db]

    def ref(x, dy):
        x64, g64, b64 = cpu64(x).requires_grad_(), cpu64(gm).requires_grad_(), cpu64(bt).requires_grad_()
        y = P.pyg_layer_norm(x64, g64, b64, "graph")
        y.backward(cpu64(dy))
        xd = x64.detach()
        stats = torch.stack([xd.mean(dim=(1, 2)), 1 / (xd.var(dim=(1, 2), unbiased=False).sqrt() + EPS)], 1)
        return [y.detach(), stats, x64.grad, g64.grad, b64.grad]

    clean, names = launched(lambda: run(x, dy))
    for k in ("gn_partial_kernel", "gn_fwd_apply_kernel", "gn_bwd_apply_kernel"):
        assert has(names, k), names
    print("ran: gn_partial_kernel + gn_finalize_kernel + gn_fwd_apply_kernel + gn_bwd_apply_kernel  [graphnorm]")
    for b, i in [(0, 0), (1, 0), (1, n // 2), (B - 1, n - 1)]:
        for name in ("x", "dy"):
            idx = (b, i, col_of(i, F))
            xp, dyp = (poisoned(x, idx), dy) if name == "x" else (x, poisoned(dy, idx))
            contained(clean, run(xp, dyp), ref(xp, dyp), f"graphnorm: NaN in {name}{list(idx)}")


# ------------------------------------------------------------------------------------------------------------------
# A / B. gcl_aggregate and its forms
# ------------------------------------------------------------------------------------------------------------------
def poison_nodes(e2, n):
    """Row 0; a row all of whose readers sit in another 64-row tile (if the graph has one); a sender of a heavy row
    (more than 64 in-edges; if the graph has one)."""
    out = {"row 0": 0}
    src_tile, dst_tile = e2[0] // 64, e2[1] // 64
    near = torch.zeros(n, dtype=torch.bool)
    near[e2[0][src_tile == dst_tile]] = True
    read = torch.zeros(n, dtype=torch.bool)
    read[e2[0]] = True
    far = torch.nonzero(read & ~near).flatten()
    if far.numel():
        out["read from another tile only"] = int(far[far.numel() // 2])
    deg = torch.bincount(e2[1], minlength=n)
    heavy = torch.nonzero(deg > 64).flatten()
    if heavy.numel():
        senders = e2[0][e2[1] == heavy[0]]
        cand = senders[((senders - heavy[0]).abs() > 8) & (senders != 0)].sort().values  # not a ring neighbour, not row 0
        out["sender of a heavy row"] = int(cand[cand.numel() // 2])
    return out


def agg_kernels(names):
    ks = sorted({n.split("(")[0].replace("void ", "").replace("gcl::", "") for n in names if "agg_" in n})
    assert ks, f"no aggregation kernel ran: {names}"
    return ks


AGG_GRAPHS = [("heavy_ring", "gcn"), ("degree", "mean"), ("mesh23_tiled", "gcn")]


@gpu
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("halo", ["1", "0"])
@pytest.mark.parametrize("gname,kind", AGG_GRAPHS)
def test_aggregate_contains_a_poisoned_row(hip, graphs, monkeypatch, gname, kind, halo, transpose):
    """gcl_aggregate, both directions, with and without the source-tile kernel: NaN (and +inf) in one row of one sample
    reaches exactly the rows that read it - not the rows whose padded or skipped records point at row 0, not the other
    rows of a heavy row's block, not the other samples."""
    monkeypatch.setenv("GCL_AGG_HALO", halo)
    n, ei = graphs[gname]
    k = hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN
    G = hip.Graph(ei, n, k)
    e2, w = edges_of(k, n, ei, hip)
    spots = poison_nodes(e2, n)
    assert gname != "heavy_ring" or "sender of a heavy row" in spots
    assert gname != "degree" or len(spots) == 3, spots
    if transpose:
        e2 = e2.flip(0)
    F = 64
    h, bias = rnd(B, n, F, seed=F + n), rnd(F, seed=3)
    L, bd = hip.lib(), bias.to(DEV)
    what = f"aggregate {gname} {kind} transpose={transpose} GCL_AGG_HALO={halo}"

    def run(h):
        H_, Y = Rows.of(h.to(DEV), "pad_nan", NAN), Rows(n, F, "pad_nan", SENT, "out", B=B)
        hip._check(L.gcl_aggregate(G.handle, int(transpose), H_.ptr, H_.ld, H_.bs, bd.data_ptr(), Y.ptr, Y.ld, Y.bs, B, F,
                                   hip._stream()))
        torch.cuda.synchronize()
        assert Y.untouched(SENT), f"{what}: wrote outside y"
        return Y.view.clone()

    clean, names = launched(lambda: run(h))
    ks = agg_kernels(names)
    if gname == "mesh23_tiled":
        assert has(names, "agg_halo_loop_kernel") == (halo == "1"), names
    print(f"ran: {' + '.join(ks)}  [{what}]")
    for label, s in spots.items():
        for val in (NAN, INF) if s == 0 else (NAN,):
            hp = poisoned(h, (1, s, col_of(s, F)), val)
            ref = P._propagate_sum(hp.double(), e2, w, n) + bias.double()
            contained(clean, run(hp), ref, f"{what}: {val} in h[1, {s}] ({label})")


@gpu
@pytest.mark.parametrize("transpose", [False, True])
def test_aggregate_forms_contain_a_poisoned_row(hip, graphs, transpose):
    """gcl_aggregate_present (NaN in an ABSENT row reaches nothing), gcl_aggregate_split and gcl_aggregate_head on the
    ring with a heavy row."""
    n, ei = graphs["heavy_ring"]
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    e2, w = edges_of(hip.GRAPH_GCN, n, ei, hip)
    spots = poison_nodes(e2, n)
    s_heavy = spots["sender of a heavy row"]
    if transpose:
        e2 = e2.flip(0)
    F, head = 64, 300
    h = rnd(B, n, F, seed=7)
    absent = torch.arange(n) % 5 == 2
    absent[s_heavy] = True
    absent[0] = False
    present = torch.where(absent, -1, 1).to(torch.int32).to(DEV)

    def ref(h, zero_rows=None):
        h64 = h.double().clone()
        if zero_rows is not None:
            h64[:, zero_rows] = 0.0
        return P._propagate_sum(h64, e2, w, n)

    forms = {
        "present": (lambda h: hip.aggregate_present(G, h.to(DEV), present, None, transpose), lambda h: ref(h, absent),
                    [0, s_heavy, int(torch.nonzero(absent)[3])]),
        "split": (lambda h: hip.aggregate_split(G, h[:, :head].contiguous().to(DEV), h[:, head:].contiguous().to(DEV), transpose),
                  ref, [0, head - 1, head, s_heavy]),
        "head": (lambda h: hip.aggregate_head(G, h[:, :head].contiguous().to(DEV), transpose),
                 lambda h: ref(h, torch.arange(n) >= head), [0, head - 1, n - 1]),
    }
    for form, (run, ref_of, rows) in forms.items():
        clean, names = launched(lambda: run(h))
        torch.cuda.synchronize()
        print(f"ran: {' + '.join(agg_kernels(names))}  [aggregate_{form} transpose={transpose}]")
        for s in rows:
            hp = poisoned(h, (1, s, col_of(s, F)))
            want = ref_of(hp)
            if (form == "present" and bool(absent[s])) or (form == "head" and s >= head):
                assert bool(torch.isfinite(want).all()), "a row that is not read reaches nothing"
            got = run(hp)
            torch.cuda.synchronize()
            contained(clean, got, want, f"aggregate_{form} transpose={transpose}: NaN in h[1, {s}]")


@gpu
def test_aggregate_compact_contains_a_poisoned_row(hip, graphs):
    """gcl_aggregate_compact (the transposed source-tile kernel with a store map): the poisoned row's readers are
    non-finite wherever the map sends them, in place or into the compact destination."""
    n, ei = graphs["mesh23_tiled"]
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    e2, w = edges_of(hip.GRAPH_GCN, n, ei, hip)
    e2 = e2.flip(0)
    F = 64
    h = rnd(B, n, F, seed=81)
    assert hip.aggregate_compact_ok(G, h.to(DEV), transpose=True), "the source-tile kernel does not take this graph"
    rows = torch.nonzero(torch.rand(n, generator=torch.Generator().manual_seed(82)) < 0.3).flatten()
    rows = rows[torch.randperm(rows.numel(), generator=torch.Generator().manual_seed(83))]
    smap = torch.full((n,), -1, dtype=torch.int32)
    smap[rows] = torch.arange(rows.numel(), dtype=torch.int32)
    compact = smap >= 0

    def run(h):
        out = torch.full((B, n, F), SENT, device=DEV)
        big = torch.full((B, rows.numel() + 3, F), SENT, device=DEV)
        outc = big[:, 1: 1 + rows.numel()]
        hip.aggregate_compact(G, h.to(DEV), smap.to(DEV), outc, transpose=True, out=out)
        torch.cuda.synchronize()
        assert bool((out[:, compact.to(DEV)] == SENT).all()) and bool((big[:, 0] == SENT).all()) \
            and bool((big[:, 1 + rows.numel():] == SENT).all()), "written outside the rows the map names"
        return [out[:, (~compact).to(DEV)], outc.clone()]

    clean, names = launched(lambda: run(h))
    print(f"ran: {' + '.join(agg_kernels(names))}  [aggregate_compact]")
    for s in sorted(set(poison_nodes(e2, n).values()) | {n - 1, 95}):
        hp = poisoned(h, (1, s, col_of(s, F)))
        ref = P._propagate_sum(hp.double(), e2, w, n)
        contained(clean, run(hp), [ref[:, ~compact], ref[:, rows]], f"aggregate_compact: NaN in h[1, {s}]")


@gpu
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("gname,kind,halo", [("heavy_ring", "gcn", "1"), ("mesh23_tiled", "gcn", "1"), ("mesh23_tiled", "gcn", "0"),
                                             ("degree", "mean", "1")])
def test_aggregate_is_scale_covariant(hip, graphs, monkeypatch, gname, kind, halo, transpose):
    """y(2^k h, 2^k bias) = 2^k y(h, bias), bit for bit (the edge weights stay as the graph holds them)."""
    monkeypatch.setenv("GCL_AGG_HALO", halo)
    n, ei = graphs[gname]
    G = hip.Graph(ei, n, hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN)
    F = 64
    h, bias = unit_range(B, n, F, seed=n), unit_range(F, seed=4)
    what = f"aggregate {gname} {kind} transpose={transpose} GCL_AGG_HALO={halo}"
    base, names = launched(lambda: hip.aggregate(G, h, bias, transpose))
    torch.cuda.synchronize()
    print(f"ran: {' + '.join(agg_kernels(names))}  [{what}]")
    for k in SCALES:
        covariant(base, hip.aggregate(G, h * 2.0 ** k, bias * 2.0 ** k, transpose), k, f"{what}: h * 2^{k}")


# ------------------------------------------------------------------------------------------------------------------
# A / B. gcl_gcn_layer_fwd and its forms
# ------------------------------------------------------------------------------------------------------------------
def gcn_ref(x, W, bias, act, e2, w, n):
    return P._propagate_sum(act64(x.double(), act, A) @ W.double().t(), e2, w, n) + bias.double()


GCN_CASES = [  # graph, kind, Fin, Fout, act, GCL_GCN_HALO -> the kernel
    ("mesh23_tiled", "gcn", 64, 64, 1, "1", "gcn_halo_fwd_kernel"), ("mesh23_tiled", "gcn", 64, 64, 1, "0", "gcn_fwd_kernel"),
    ("mesh23_tiled", "gcn", 48, 33, 0, "1", "gcn_halo_fwd_kernel"), ("degree64", "mean", 64, 33, 0, "1", "gcn_fwd_kernel"),
    ("mesh12", "gcn", 12, 33, 2, "1", "gcn_fwd_kernel")]


@gpu
@pytest.mark.parametrize("gname,kind,Fin,Fout,act,halo,kern", GCN_CASES)
def test_gcn_layer_contains_a_poisoned_row(hip, graphs, monkeypatch, gname, kind, Fin, Fout, act, halo, kern):
    """gcl_gcn_layer_fwd and gcl_gcn_layer_fwd_rows (the source-tile layer on split operands and the per-edge layer):
    NaN (+inf) in one row of x of one sample reaches exactly the rows that read it."""
    monkeypatch.setenv("GCL_GCN_HALO", halo)
    n, ei = graphs[gname]
    k = hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN
    G = hip.Graph(ei, n, k)
    e2, w = edges_of(k, n, ei, hip)
    Fs = (Fout + 3) // 4 * 4
    x, W, bias = rnd(B, n, Fin, seed=Fin + Fout), rnd(Fout, Fin, seed=2, scale=0.3), rnd(Fout, seed=3)
    L, Wd, bd, a = hip.lib(), W.to(DEV), bias.to(DEV), torch.tensor([A], device=DEV)
    what = f"gcn_layer {gname} {kind} {Fin}->{Fout} act={act} GCL_GCN_HALO={halo}"

    def run(x, rows_out=None):
        X, Y = Rows.of(x.to(DEV), "pad_nan", NAN), Rows(n, Fs, "pad_nan", SENT, "out", B=B)
        sl = a.data_ptr() if act == 1 else None
        if rows_out is None:
            rc = L.gcl_gcn_layer_fwd(G.handle, X.ptr, X.ld, X.bs, act, sl, Wd.data_ptr(), bd.data_ptr(), Y.ptr, Y.ld, Y.bs,
                                     B, Fin, Fout, Fs, hip._stream())
        else:
            rc = L.gcl_gcn_layer_fwd_rows(G.handle, X.ptr, X.ld, X.bs, act, sl, Wd.data_ptr(), bd.data_ptr(), Y.ptr, Y.ld,
                                          Y.bs, B, Fin, Fout, Fs, rows_out, hip._stream())
        hip._check(rc)
        torch.cuda.synchronize()
        r = n if rows_out is None else rows_out
        if r < n:
            torch.as_strided(Y.inside, (B, n - r, Fs), (Y.bs, Y.ld, 1), Y.view.storage_offset() + r * Y.ld).fill_(False)
        assert Y.untouched(SENT), f"{what}: wrote outside y[:, :rows_out, :Fout_store]"
        return Y.view[:, :r, :Fout].clone()

    clean, names = launched(lambda: run(x))
    assert has(names, kern + "<"), f"{what}: {names}"
    print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [{what}]")
    clean70, names70 = launched(lambda: run(x, 70))
    print(f"ran: {'gcn_halo_fwd_kernel' if has(names70, 'gcn_halo_fwd_kernel') else 'gcn_fwd_kernel'}  [{what} rows_out=70]")
    spots = poison_nodes(e2, n)
    spots.update({"mid-tile": 95, "last": n - 1})
    for label, s in spots.items():
        for val in (NAN, INF) if s == 0 else (NAN,):
            xp = poisoned(x, (1, s, col_of(s, Fin)), val)
            ref = gcn_ref(xp, W, bias, act, e2, w, n)
            contained(clean, run(xp), ref, f"{what}: {val} in x[1, {s}] ({label})")
            contained(clean70, run(xp, 70), ref[:, :70], f"{what} rows_out=70: {val} in x[1, {s}] ({label})", min_finite=0.5)


@gpu
def test_gcn_layer_tab_and_split_contain_a_poisoned_row(hip, graphs, monkeypatch):
    """gcl_gcn_layer_fwd_tab (input rows through a row table: a sample's own row or a batch-invariant flat row, which every
    sample reads) and gcl_gcn_layer_fwd_split (two-part destination)."""
    n, ei = graphs["mesh23_tiled"]
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    e2, w = edges_of(hip.GRAPH_GCN, n, ei, hip)
    Fin = Fout = 64
    W, bias = rnd(Fout, Fin, seed=2, scale=0.3), rnd(Fout, seed=3)
    Wd, bd, a = W.to(DEV), bias.to(DEV), torch.tensor([A], device=DEV)
    # the row table
    ne = n // 3 + 17
    gen = torch.Generator().manual_seed(5)
    x = rnd(B, ne, Fin, seed=1)
    own = torch.rand(n, generator=gen) < 0.5
    tab = torch.where(own, torch.randint(0, ne, (n,), generator=gen), -torch.randint(0, B * ne, (n,), generator=gen) - 1).to(torch.int32)

    def lat_of(x):
        return torch.where(own[None, :, None], x[:, tab.clamp(min=0).long()], x.reshape(B * ne, Fin)[(-tab.long() - 1).clamp(min=0)][None])

    assert hip.gcn_layer_tab_ok(G, x.to(DEV), Fout)

    def run_tab(x):
        y = hip.gcn_layer_fwd_tab(G, x.to(DEV), tab.to(DEV), 1, a, Wd, bd)
        torch.cuda.synchronize()
        return y

    clean, names = launched(lambda: run_tab(x))
    assert has(names, "gcn_halo_fwd_kernel"), names
    print(f"ran: gcn_halo_fwd_kernel<{', '.join(targs(names, 'gcn_halo_fwd_kernel')[0])}>  [gcn_layer_fwd_tab]")
    used_own = sorted(set(tab[own].tolist()))
    used_flat = sorted(set((-tab[~own].long() - 1).tolist()))
    for b, r in [(1, used_own[0]), (1, used_own[len(used_own) // 2]), divmod(used_flat[len(used_flat) // 2], ne), (B - 1, ne - 1)]:
        xp = poisoned(x, (b, r, col_of(r, Fin)))
        contained(clean, run_tab(xp), gcn_ref(lat_of(xp), W, bias, 1, e2, w, n), f"gcn_layer_fwd_tab: NaN in x[{b}, {r}]")
    # the two-part destination (head % 32 == 0; only the per-edge layer has it: GCL_GCN_HALO=0)
    monkeypatch.setenv("GCL_GCN_HALO", "0")
    n, ei = graphs["mesh12"]
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    e2, w = edges_of(hip.GRAPH_GCN, n, ei, hip)
    head = 96
    x = rnd(B, n, Fin, seed=4)

    def run_split(x):
        ya, yb = torch.full((B, head, Fout), SENT, device=DEV), torch.full((B, n - head, Fout), SENT, device=DEV)
        xd = x.to(DEV)
        assert hip.gcn_layer_split_ok(G, xd, Fout, ya, yb), "the split form does not take this layer"
        hip.gcn_layer_fwd_split(G, xd, 1, a, Wd, bd, ya, yb)
        torch.cuda.synchronize()
        return [ya, yb]

    clean, names = launched(lambda: run_split(x))
    kern = "gcn_halo_fwd_kernel" if has(names, "gcn_halo_fwd_kernel") else "gcn_fwd_kernel"
    print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [gcn_layer_fwd_split]")
    for s in (0, head - 1, head, n - 1):
        xp = poisoned(x, (1, s, col_of(s, Fin)))
        ref = gcn_ref(xp, W, bias, 1, e2, w, n)
        contained(clean, run_split(xp), [ref[:, :head], ref[:, head:]], f"gcn_layer_fwd_split: NaN in x[1, {s}]")


@gpu
@pytest.mark.parametrize("gname,kind,Fin,Fout,act,halo,kern", GCN_CASES[:4])
def test_gcn_layer_is_scale_covariant(hip, graphs, monkeypatch, gname, kind, Fin, Fout, act, halo, kern):
    """The layer is linear in x (activation none or PReLU) and in W, with the bias scaled along."""
    monkeypatch.setenv("GCL_GCN_HALO", halo)
    n, ei = graphs[gname]
    G = hip.Graph(ei, n, hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN)
    x, W, bias = unit_range(B, n, Fin, seed=n), unit_range(Fout, Fin, seed=6) / 4, unit_range(Fout, seed=7)
    a = torch.tensor([A], device=DEV)
    what = f"gcn_layer {gname} {kind} {Fin}->{Fout} act={act} GCL_GCN_HALO={halo}"

    def run(kx, kw):
        y = hip.gcn_layer_fwd(G, x * 2.0 ** kx, act, a if act == 1 else None, W * 2.0 ** kw, bias * 2.0 ** (kx + kw))
        torch.cuda.synchronize()
        return y.clone()

    base, names = launched(lambda: run(0, 0))
    assert has(names, kern + "<"), f"{what}: {names}"
    print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [{what}]")
    for kx, kw in [(k, 0) for k in SCALES] + [(0, k) for k in SCALES] + [(-48, -48), (48, 48)]:
        covariant(base, run(kx, kw), kx + kw, f"{what}: x * 2^{kx}, W * 2^{kw}")


# ------------------------------------------------------------------------------------------------------------------
# A. gcl_gat_fwd / gcl_gat_bwd
# ------------------------------------------------------------------------------------------------------------------
def gat_ref(p, ei, h):
    """float64 autograd of oracle.pyg_ops.gat_conv on h (identity weight): y, the per-node score terms, alpha in PyG edge
    order, dh and the parameter gradients."""
    Hh, C = p.H, p.C
    x = h.double().requires_grad_()
    as64, ad64 = p.a_s.double().view(1, Hh, C).requires_grad_(), p.a_d.double().view(1, Hh, C).requires_grad_()
    b64 = p.b.double().requires_grad_()
    y, _, alpha = P.gat_conv(x, ei, torch.eye(Hh * C, dtype=torch.float64), as64, ad64, b64, Hh)
    y.backward(p.dy.double())
    h4 = h.double().view(h.shape[0], p.n, Hh, C)
    s_src, s_dst = (h4 * p.a_s.double().view(Hh, C)).sum(-1), (h4 * p.a_d.double().view(Hh, C)).sum(-1)
    return [y.detach(), s_src, s_dst, alpha.detach(), x.grad, as64.grad.reshape(-1), ad64.grad.reshape(-1), b64.grad]


@gpu
@pytest.mark.parametrize("gname,H,C,tiles_off", [("mesh23_tiled", 1, 64, False), ("mesh23_tiled", 1, 64, True), ("mesh12", 4, 64, False),
                                                ("mesh12", 1, 12, False)])
def test_gat_contains_a_poisoned_row(hip, graphs, monkeypatch, gname, H, C, tiles_off):
    """gcl_gat_fwd / gcl_gat_bwd, the source-tile and the per-edge kernels, one and four heads: NaN in one row of h of one
    sample; the reach of y, alpha, dh and the parameter gradients is that of oracle.pyg_ops.gat_conv in float64."""
    from test_sparse_layouts import Gat

    n, ei = graphs[gname]
    if tiles_off:
        monkeypatch.setenv("GCL_GAT_HALO", "0")
    p = Gat(hip, n, ei, H, C, seed=H * C)
    what = f"gat {gname} H={H} C={C}{' GCL_GAT_HALO=0' if tiles_off else ''}"
    h0 = p.h

    def run(h):
        p.dev[0] = h.to(DEV)
        rc, Hh, Y, s_src, s_dst, alpha = p.fwd("pad_nan", "pad_nan", NAN)
        hip._check(rc)
        rc, DH, d_as, d_ad, d_b = p.bwd("pad_nan", "pad_nan", NAN, (s_src, s_dst, alpha))
        hip._check(rc)
        torch.cuda.synchronize()
        assert Y.untouched(SENT) and DH.untouched(SENT), f"{what}: wrote outside y or dh"
        al = torch.stack([hip.gat_alpha_edge_order(p.G, alpha[i], H) for i in range(B)])
        return [Y.view.clone(), s_src, s_dst, al, DH.view.clone(), d_as, d_ad, d_b]

    clean, names = launched(lambda: run(h0))
    staged = has(names, "gat_halo_fwd_kernel")
    assert staged == (gname == "mesh23_tiled" and not tiles_off) and staged != has(names, "gat_fwd_kernel"), names
    bwd = "gat_halo_bwd_dst_kernel + gat_halo_bwd_src_kernel" if has(names, "gat_halo_bwd_dst_kernel") else \
        "gat_bwd_dst_kernel + gat_bwd_src_kernel"
    assert has(names, bwd.split(" + ")[0]) and has(names, bwd.split(" + ")[1]), names
    print(f"ran: {'gat_halo_fwd_kernel' if staged else 'gat_fwd_kernel'} + {bwd}  [{what}]")
    for s in (0, 95, n - 1):
        hp = poisoned(h0, (1, s))  # the whole row: the layer in front of a GAT layer is dense, and so is the oracle's
        contained(clean, run(hp), gat_ref(p, ei, hp), f"{what}: NaN in h[1, {s}]")


@gpu
def test_gat_through_a_row_table_contains_a_poisoned_row(hip, graphs):
    """gcl_gat_fwd_tab / gcl_gat_bwd_tab: the rows of h are a sample's own rows of a compact tensor or batch-invariant flat
    rows, which every sample reads; the reference is the oracle on the materialised rows."""
    import types

    n, ei = graphs["mesh23_tiled"]
    H, C = 1, 64
    G = hip.Graph(ei, n, hip.GRAPH_GAT)
    assert hip.gat_tab_ok(G, H, C), "no row-table form on this graph"
    nc = n // 3 + 11
    gen = torch.Generator().manual_seed(7)
    hc = rnd(B, nc, C, seed=1)
    own = torch.rand(n, generator=gen) < 0.5
    tab = torch.where(own, torch.randint(0, nc, (n,), generator=gen), -torch.randint(0, B * nc, (n,), generator=gen) - 1).to(torch.int32)
    p = types.SimpleNamespace(H=H, C=C, n=n, a_s=rnd(C, seed=3, scale=0.3), a_d=rnd(C, seed=4, scale=0.3), b=rnd(C, seed=5),
                              dy=rnd(B, n, C, seed=6))
    dev = [t.to(DEV) for t in (p.a_s, p.a_d, p.b, p.dy, tab)]

    def rows_of(hc):
        return torch.where(own[None, :, None], hc[:, tab.clamp(min=0).long()], hc.reshape(B * nc, C)[(-tab.long() - 1).clamp(min=0)][None])

    def run(hc):
        a_s, a_d, b, dy, tab_d = dev
        y, s_src, s_dst, alpha = hip.gat_fwd(G, hc.to(DEV), a_s, a_d, b, H, C, tab=tab_d)
        d_as, d_ad, d_b = (torch.full((C,), SENT, device=DEV) for _ in range(3))
        dh = hip.gat_bwd(G, dy, hc.to(DEV), a_s, a_d, s_src, s_dst, alpha, d_as, d_ad, d_b, False, H, C, tab=tab_d)
        torch.cuda.synchronize()
        al = torch.stack([hip.gat_alpha_edge_order(G, alpha[i], H) for i in range(B)])
        return [y, s_src, s_dst, al, dh, d_as, d_ad, d_b]

    clean, names = launched(lambda: run(hc))
    assert has(names, "gat_halo_fwd_kernel") and has(names, "gat_halo_bwd_dst_kernel"), names
    print(f"ran: gat_halo_fwd_kernel<{', '.join(targs(names, 'gat_halo_fwd_kernel')[0])}> + gat_halo_bwd_dst_kernel + "
          f"gat_halo_bwd_src_kernel  [gat through a row table]")
    used_own = sorted(set(tab[own].tolist()))
    used_flat = sorted(set((-tab[~own].long() - 1).tolist()))
    for b_, r in [(1, used_own[0]), (1, used_own[len(used_own) // 2]), divmod(used_flat[len(used_flat) // 2], nc)]:
        hp = poisoned(hc, (b_, r))
        contained(clean, run(hp), gat_ref(p, ei, rows_of(hp)), f"gat through a row table: NaN in h[{b_}, {r}]")


# ------------------------------------------------------------------------------------------------------------------
# A. Step glue
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_assemble_input_and_window_pack_carry_one_element(hip):
    """gcl_assemble_input (a NaN of x lands in one element of the assembled rows) and gcl_window_pack (an fp16 inf of the
    series lands in the windows that contain its frame, once each)."""
    g = torch.Generator().manual_seed(1)
    G_, M, Cd, Cs = 129, 37, 12, 4
    x, gs, ms = torch.randn(B, G_, Cd, generator=g), torch.randn(G_, Cs, generator=g), torch.randn(M, Cs, generator=g)

    def ref(x):
        top = torch.cat([x.double(), gs.double().expand(B, G_, Cs)], 2)
        return torch.cat([top, torch.cat([torch.zeros(B, M, Cd, dtype=torch.float64), ms.double().expand(B, M, Cs)], 2)], 1)

    clean, names = launched(lambda: hip.assemble_input(x.to(DEV), gs.to(DEV), ms.to(DEV)))
    torch.cuda.synchronize()
    assert has(names, "assemble"), names
    print("ran: " + " + ".join(sorted(n.split("(")[0] for n in names if "assemble" in n)) + "  [assemble_input]")
    for b, i in [(0, 0), (1, 0), (1, 95), (B - 1, G_ - 1)]:
        xp = poisoned(x, (b, i, col_of(i, Cd)))
        contained(clean, hip.assemble_input(xp.to(DEV), gs.to(DEV), ms.to(DEV)), ref(xp), f"assemble_input: NaN in x[{b}, {i}]")

    T, N, Ct, C, obs, pred = 9, 129, 5, 4, 2, 2
    series = (torch.randn(T, N, Ct, generator=g) * 30).half()
    mean, std = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    t0 = torch.tensor([3, 0, 4], dtype=torch.int64)

    def pack_ref(series):
        z = (series[:, :, :C].double() - mean.double()) / std.double()
        X = torch.stack([torch.cat([z[t + o] for o in range(obs)], 1) for t in t0.tolist()])
        Y = torch.stack([torch.cat([z[t + obs + q] for q in range(pred)], 1) for t in t0.tolist()])
        return [X, Y]

    def pack(series):
        X, Y = hip.window_pack(series.to(DEV), t0.to(DEV), mean.to(DEV), std.to(DEV), C, obs, pred)
        torch.cuda.synchronize()
        return [X, Y]

    clean, names = launched(lambda: pack(series))
    assert has(names, "window_pack"), names
    print("ran: " + " + ".join(sorted(n.split("(")[0] for n in names if "window_pack" in n)) + "  [window_pack]")
    for t, node, c in [(4, 0, 0), (5, 95, 3), (0, N - 1, 1), (5, 64, Ct - 1)]:  # (the last: a channel that is not packed)
        sp = poisoned(series, (t, node, c), INF)
        contained(clean, pack(sp), pack_ref(sp), f"window_pack: inf in series[{t}, {node}, {c}]")


@gpu
def test_loss_and_ar_step_carry_one_element(hip):
    """gcl_wmse_fwd_bwd: a NaN in delta makes the loss non-finite and the gradient non-finite at that element only.
    gcl_ar_advance / gcl_ar_step_bwd: one element of the step, of the new state and of the gradients."""
    from test_norm_glue import CHAN_KINDS, ar_step_ref, f32

    g = torch.Generator().manual_seed(2)
    G_, C = 129, len(CHAN_KINDS)
    delta, xl, y = (torch.randn(B, G_, C, generator=g) for _ in range(3))
    node_w, chan_w = torch.rand(G_, generator=g) + 0.1, torch.rand(C, generator=g) + 0.5
    inv = f32(1.0 / float((node_w.double()[:, None] * chan_w.double()).sum() * B))

    def wmse(delta):
        loss, dd, st = hip.wmse_fwd_bwd(delta.to(DEV), xl.to(DEV), y.to(DEV), node_w.to(DEV), chan_w.to(DEV), inv, 0.5,
                                        want_grad=True, want_state=True)
        torch.cuda.synchronize()
        return [loss.reshape(1), dd, st]

    def wmse_ref(delta):
        wgt = node_w.double()[:, None] * chan_w.double()
        o = delta.double() + xl.double()
        d = o - y.double()
        return [((wgt * d * d).sum() * inv).reshape(1), 2 * wgt * d * inv * 0.5, o]

    clean, names = launched(lambda: wmse(delta))
    assert has(names, "wmse_kernel") and has(names, "wmse_final_kernel"), names
    print("ran: wmse_kernel + wmse_final_kernel  [wmse_fwd_bwd]")
    for b, i in [(0, 0), (1, 0), (1, 95), (B - 1, G_ - 1)]:
        dp = poisoned(delta, (b, i, col_of(i, C)))
        want = wmse_ref(dp)
        assert not bool(torch.isfinite(want[0]).any())
        contained(clean, wmse(dp), want, f"wmse: NaN in delta[{b}, {i}]")

    obs = 3
    kinds = torch.tensor(CHAN_KINDS, dtype=torch.int32)
    state, dd, g_new = torch.randn(B, G_, obs, C, generator=g), torch.randn(B, G_, C, generator=g), torch.randn(B, G_, obs, C, generator=g)

    def advance(delta):
        out = torch.full((B, G_, 2 * C + 3), SENT, device=DEV)
        new = hip.ar_advance(state.to(DEV), delta.to(DEV), y.to(DEV), kinds.to(DEV), out, C + 1, True)
        torch.cuda.synchronize()
        assert bool((out[:, :, :C + 1] == SENT).all()) and bool((out[:, :, 2 * C + 1:] == SENT).all())
        return [out[:, :, C + 1:2 * C + 1], new]

    def advance_ref(delta):
        k = kinds.long()
        want = torch.where(k == 1, state[:, :, -1].double(), state[:, :, -1].double() + delta.double())
        want = torch.where(k == 2, y.double(), want)
        return [want, torch.cat([state[:, :, 1:].double(), want.unsqueeze(2)], 2)]

    clean, names = launched(lambda: advance(delta))
    assert has(names, "ar_advance"), names
    print("ran: " + " + ".join(sorted(n.split("(")[0] for n in names if "ar_" in n)) + "  [ar_advance]")
    for b, i, c in [(0, 0, 0), (1, 0, 3), (1, 95, 6), (B - 1, G_ - 1, 1)]:  # (channel 1 is static: the step ignores delta)
        dp = poisoned(delta, (b, i, c))
        contained(clean, advance(dp), advance_ref(dp), f"ar_advance: NaN in delta[{b}, {i}, {c}]")

    def step_bwd(dd):
        d_delta, d_state = hip.ar_step_bwd(dd.to(DEV), None, g_new.to(DEV), kinds.to(DEV), True, True, obs, want_state=True)
        torch.cuda.synchronize()
        return [d_delta, d_state]

    clean, names = launched(lambda: step_bwd(dd))
    assert has(names, "ar_step_bwd"), names
    print("ran: " + " + ".join(sorted(n.split("(")[0] for n in names if "ar_" in n)) + "  [ar_step_bwd]")
    for b, i, c in [(0, 0, 0), (1, 0, 3), (1, 95, 6), (B - 1, G_ - 1, 1)]:
        ddp = poisoned(dd, (b, i, c))
        contained(clean, step_bwd(ddp), list(ar_step_ref(delta, state, y, kinds, True, True, ddp, None, g_new)),
                  f"ar_step_bwd: NaN in dd[{b}, {i}, {c}]")


@gpu
@pytest.mark.parametrize("form", ["step", "dev", "groups"])
def test_adam_contains_a_poisoned_gradient(hip, form):
    """gcl_adam_step, _dev and _groups: one NaN gradient element poisons that element's p, m and v; every other element
    keeps the clean run's bits."""
    count = 64 * 21
    g = torch.Generator().manual_seed(4)
    p0, g0 = torch.randn(count, generator=g), torch.randn(count, generator=g)
    m0, v0 = 0.1 * torch.randn(count, generator=g), 0.01 * torch.rand(count, generator=g)
    lr, b1, b2, eps, wd = 3e-3, 0.9, 0.999, 1e-8, 0.01

    def run(grad):
        p, m, v, gd = p0.to(DEV), m0.to(DEV), v0.to(DEV), grad.to(DEV)
        if form == "step":
            hip.adam_step(p, gd, m, v, lr, b1, b2, eps, wd, 3, 0.5)
        elif form == "dev":
            hip.adam_step_dev(p, gd, m, v, lr, b1, b2, eps, wd, torch.full((1,), 2, dtype=torch.int32, device=DEV),
                              torch.zeros(2, device=DEV), 0.5)
        else:
            chunk_param = torch.tensor([0] * 5 + [1] * 9 + [2] * 7, dtype=torch.int32, device=DEV)
            hip.adam_step_groups(p, gd, m, v, chunk_param, torch.ones(3, dtype=torch.int32, device=DEV),
                                 torch.full((3,), lr, device=DEV), torch.full((3,), 2, dtype=torch.int32, device=DEV),
                                 torch.zeros(3, 2, device=DEV), b1, b2, eps, wd, 0.5)
        torch.cuda.synchronize()
        return [p, m, v]

    def ref(grad):
        gg = grad.double() * 0.5 + wd * p0.double()
        m, v = b1 * m0.double() + (1 - b1) * gg, b2 * v0.double() + (1 - b2) * gg * gg
        return [p0.double() - lr * (m / (1 - b1 ** 3)) / ((v / (1 - b2 ** 3)).sqrt() + eps), m, v]

    clean, names = launched(lambda: run(g0))
    kern = {"step": "adam_kernel", "dev": "adam_dev_kernel", "groups": "adam_groups_kernel"}[form]
    assert has(names, kern), names
    print(f"ran: {kern}  [adam {form}]")
    for i in (0, 64 * 5 - 1, 64 * 5, 64 * 10 + 31, count - 1):
        contained(clean, run(poisoned(g0, (i,))), ref(poisoned(g0, (i,))), f"adam {form}: NaN in g[{i}]")


# ------------------------------------------------------------------------------------------------------------------
# A. Whole model, forward
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("no_compact", [False, True])
@pytest.mark.parametrize("name", ["baseline", "attention", "graph_ln"])
def test_model_forward_contains_a_poisoned_sample(monkeypatch, name, no_compact):
    """One NaN at one grid node of sample 1 of 3: samples 0 and 2 are bit-equal to the clean forward, sample 1 is finite
    exactly where the float oracle is (it may be mostly non-finite: the cap here is per batch, two of three samples
    wholly finite in the reference)."""
    from test_hip_model import data, make_pair

    if no_compact:
        monkeypatch.setenv("GCL_NO_COMPACT", "1")

    def tweak(cfg):
        cfg.pipeline.encoder.mlp.layer_norm_mode = "graph"
        cfg.pipeline.processor.gcn.layer_norm_mode = "graph"

    cfg, m, o = make_pair("baseline" if name == "graph_ln" else name, [1, 2], tweak=tweak if name == "graph_ln" else None)
    if name == "graph_ln":
        m.compact = False  # graph-mode statistics couple all rows of a sample (test_graph_mode_layernorm_model)
    X, _ = data(cfg, m._num_grid_nodes, B)
    with torch.no_grad():
        clean, names = launched(lambda: m(X.to(DEV)).clone())
        torch.cuda.synchronize()
        kern = "gat_" if name == "attention" else "gcn_"
        assert has(names, kern), names
        print(f"ran: {len(names)} kernels, among them {sorted(n.split('(')[0].split('<')[0] for n in names if kern in n)}  "
              f"[model {name} GCL_NO_COMPACT={int(no_compact)}]")
        Xp = poisoned(X, (1, m._num_grid_nodes // 2 + 5, 3))
        got = m(Xp.to(DEV))
        torch.cuda.synchronize()
        ref = o(Xp)
    assert bool(torch.isfinite(ref[0]).all()) and bool(torch.isfinite(ref[2]).all()) and not bool(torch.isfinite(ref[1]).all())
    assert bool(torch.isfinite(clean).all())
    for b in (0, 2):
        assert same_bits(got[b], clean[b]), f"model {name}: sample {b} differs from the clean forward"
    assert torch.equal(torch.isfinite(got[1]).cpu(), torch.isfinite(ref[1])), \
        f"model {name}: sample 1 is finite at {int(torch.isfinite(got[1]).sum())} elements, the oracle at {int(torch.isfinite(ref[1]).sum())}"


# ------------------------------------------------------------------------------------------------------------------
# C. The band of the split-operand kernels (csrc/x3.h)
# ------------------------------------------------------------------------------------------------------------------
# The band csrc/x3.h, include/gcl.h and DESIGN.md 3.1 state, in powers of two: an operand element v is 0 or
# 2^BAND_LO <= |v| < 2^BAND_HI_OPERAND, and the sum of |products| of an output is below 2^BAND_HI_PRODUCT.  The measured
# sweep behind it is DESIGN.md 3.1's table: the BAND_CASES below, x = order_one data * 2^k, error ratio of `arbitration`.
BAND_LO, BAND_HI_OPERAND, BAND_HI_PRODUCT = -110, 127, 127
SWEEP_K = list(range(-126, -89, 4)) + list(range(90, 127, 4))  # the exponents of DESIGN.md 3.1's table


def order_one(*shape, seed):
    """Normal data cut at +-1.99, so that 2^k times it stays below 2^(k+1)."""
    return rnd(*shape, seed=seed).clamp(-1.99, 1.99)


def small_w(*shape, seed, scale=0.3):
    return rnd(*shape, seed=seed, scale=scale).clamp(-1.0, 1.0)


class BandFwd:
    """linear_x3_fwd_kernel: y = PReLU(x) W^T, 1024 x 64 -> 64."""
    want = ("linear_x3_fwd_kernel", ["2", "false", "4"])
    shape = (1024, 64)

    def __init__(self, graphs=None):
        self.W = small_w(64, 64, seed=12)
        self.a = torch.tensor([A])

    def run(self, hip, x):
        return [hip.linear_fwd(x.to(DEV), self.W.to(DEV), None, self.a.to(DEV))]

    def ref(self, x, dt):
        return [P.prelu(x, self.a).to(dt) @ self.W.to(dt).t()]


class BandBwd:
    """linear_x3_bwd_kernel: dx = (dy W) PReLU'(x), dW = dy^T PReLU(x), with db and the column sums asked for."""
    want = ("linear_x3_bwd_kernel", ["2"])
    shape = (1024, 64)
    lean = False

    def __init__(self, graphs=None):
        self.W, self.x, self.a = small_w(64, 64, seed=22), order_one(1024, 64, seed=23).clamp(-1.0, 1.0), torch.tensor([A])

    def run(self, hip, dy):
        dW, db, cs, ds = (torch.zeros(s, device=DEV) for s in ((64, 64), (64,), (64,), (1,)))
        if self.lean:
            dx = hip.linear_bwd_all(dy.to(DEV), self.W.to(DEV), self.x.to(DEV), None, None, dW, db, None, False)
        else:
            dx = hip.linear_bwd_all(dy.to(DEV), self.W.to(DEV), self.x.to(DEV), self.a.to(DEV), ds, dW, db, cs, False)
        return [dx, dW]

    def ref(self, dy, dt):
        if self.lean:
            return [dy.to(dt) @ self.W.to(dt), dy.to(dt).t() @ self.x.to(dt)]
        d = torch.where(self.x > 0, 1.0, A).to(dt)
        return [(dy.to(dt) @ self.W.to(dt)) * d, dy.to(dt).t() @ P.prelu(self.x, self.a).to(dt)]


class BandBwdLean(BandBwd):
    """linear_x3_bwd_lean_kernel: no activation, no column sums."""
    want = ("linear_x3_bwd_lean_kernel", ["2", "false", "true", "false", "false"])
    lean = True


class BandChain:
    """mlp_x3_chain_kernel<3, false>: three layers, zero biases (every z_k is linear in x); the layers behind the first
    have small weights, so that their partial sums stay a factor 2^4 below their inputs' magnitude."""
    want = ("mlp_x3_chain_kernel", ["3", "false"])
    shape = (1024, 64)

    def __init__(self, graphs=None):
        self.Ws = [small_w(64, 64, seed=31), small_w(64, 64, seed=32, scale=0.03), small_w(64, 64, seed=33, scale=0.03)]
        self.slopes = [torch.tensor([0.25]), torch.tensor([0.125])]

    def run(self, hip, x):
        got = hip.mlp_fwd_chain(x.to(DEV), [W.to(DEV) for W in self.Ws], [torch.zeros(64, device=DEV)] * 3,
                                [s.to(DEV) for s in self.slopes])
        assert got is not None, "the chained kernel must take this run"
        return list(got[0])

    def ref(self, x, dt):
        out, cur = [], x.to(dt)
        for k, W in enumerate(self.Ws):
            if k:
                cur = torch.where(cur > 0, cur, self.slopes[k - 1].to(dt) * cur)
            cur = cur @ W.to(dt).t()
            out.append(cur)
        return out


class BandGcn:
    """gcn_halo_fwd_kernel: the one-kernel GCN layer on the tile-ordered [2, 3] mesh, 64 -> 64, no activation, zero bias."""
    want = ("gcn_halo_fwd_kernel", None)

    def __init__(self, graphs):
        self.n, self.ei = graphs["mesh23_tiled"]
        self.shape = (B, self.n, 64)
        self.W = small_w(64, 64, seed=41)
        self.e2, self.w = P.gcn_norm(self.ei, self.n, torch.float64)

    def run(self, hip, x):
        G = hip.Graph(self.ei, self.n, hip.GRAPH_GCN)
        return [hip.gcn_layer_fwd(G, x.to(DEV), hip.ACT_NONE, None, self.W.to(DEV), torch.zeros(64, device=DEV)).clone()]

    def ref(self, x, dt):
        return [P._propagate_sum(x.to(dt) @ self.W.to(dt).t(), self.e2, self.w.to(dt), self.n)]


class BandTile:
    """gemm_tile_x3_kernel at the smallest row count that reaches it: 65409 x 12 -> 260."""
    want = ("gemm_tile_x3_kernel", ["0"])
    shape = (X3_TILE_ROWS, 12)

    def __init__(self, graphs=None):
        self.W = small_w(260, 12, seed=51)

    def run(self, hip, x):
        return [hip.dense_fwd(x.to(DEV), self.W.to(DEV), None)]

    def ref(self, x, dt):
        return [x.to(dt) @ self.W.to(dt).t()]


BAND_CASES = {"fwd": BandFwd, "bwd": BandBwd, "bwd_lean": BandBwdLean, "chain": BandChain, "gcn": BandGcn, "tile": BandTile}


def band_run(hip, case, op, what):
    got, names = launched(lambda: case.run(hip, op))
    torch.cuda.synchronize()
    kern, args = case.want
    if args is None:
        assert has(names, kern + "<"), f"{what}: {names}"
        print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [{what}]")
    else:
        ran(names, case.want, what)
    return got


def in_band(case, op):
    """Is every element of op 0 or in [2^BAND_LO, 2^BAND_HI_OPERAND), and the sum of |products| of every output below
    2^BAND_HI_PRODUCT (the reference on the magnitudes of all operands)?"""
    mag = op.abs()
    if not (bool((mag[mag != 0] >= 2.0 ** BAND_LO).all()) and bool((mag < 2.0 ** BAND_HI_OPERAND).all())):
        return False
    absolute = copy.copy(case)
    for key, val in vars(case).items():
        if key in ("W", "x"):
            setattr(absolute, key, val.abs())
        elif key == "Ws":
            absolute.Ws = [W.abs() for W in val]
    return all(float(t.max()) < 2.0 ** BAND_HI_PRODUCT for t in absolute.ref(mag, torch.float64))


@gpu
@pytest.mark.parametrize("side", ["low", "high"])
@pytest.mark.parametrize("name", list(BAND_CASES))
def test_split_kernels_keep_fp32_accuracy_at_the_edges_of_the_band(hip, graphs, name, side):
    """Data of magnitude [0.5, 2) times 2^k at the last exponent of DESIGN.md 3.1's sweep, on either side, for which the
    band includes the operand (in_band: -106 on the low side; on the high side it depends on how many products an output
    sums), the other operand of order one: every output is as close to float64 as a torch-CPU fp32 GEMM of the same
    operands (the rule of test_x3_linear_fwd_is_as_accurate_as_fp32)."""
    case = BAND_CASES[name](graphs)
    base = unit_range(*case.shape, seed=61).cpu()
    ks = [k for k in SWEEP_K if (k < 0) == (side == "low") and in_band(case, base * 2.0 ** k)]
    k = min(ks) if side == "low" else max(ks)
    assert k == -106 if side == "low" else 110 <= k <= 122, f"{name}: the band's {side} edge in the sweep is 2^{k}"
    op = base * 2.0 ** k
    got = band_run(hip, case, op, f"{name} at 2^{k}")
    for i, (g_, r32, r64) in enumerate(zip(got, case.ref(op, torch.float32), case.ref(op, torch.float64))):
        as_accurate_as_fp32(g_, r32, r64, f"{name} at 2^{k}: output {i}")


def anywhere_below_2_127(shape, per_sample_big):
    """Finite operand rows of every magnitude: row r is order-one data times 2^k_r, k_r cycling through -148 (fp32
    subnormals) .. 108 in steps of 7, so that 64 products of a row sum to less than 2^117 whatever the signs; every 41st
    row (per_sample_big: one row of each sample) instead holds ONE element +-(2^127 - 2^103), the largest value whose first
    piece is finite, in a column of its own, among order-one elements: its products with an operand of at most 1 stay
    below 2^127, and no two of them meet in one sum."""
    rows = math.prod(shape[:-1])
    x = order_one(rows, shape[-1], seed=71)
    ks = torch.arange(rows) % 37 * 7 - 148
    x = (x.double() * torch.pow(2.0, ks.double())[:, None]).float()
    big = [b * shape[1] + 100 + b for b in range(shape[0])] if per_sample_big else list(range(5, rows, 41))[:shape[-1]]
    for j, r in enumerate(big):
        x[r] = order_one(shape[-1], seed=72 + j)
        x[r, j % shape[-1]] = (2.0 ** 127 - 2.0 ** 103) * (1 if j % 2 else -1)
    assert bool(torch.isfinite(x).all()) and float(x.abs().max()) < 2.0 ** 127
    return x.view(shape)


@gpu
@pytest.mark.parametrize("name", list(BAND_CASES))
def test_split_kernels_give_finite_results_for_finite_operands(hip, graphs, name):
    """Finite operands anywhere below 2^127 (anywhere_below_2_127): wherever the float64 result is inside fp32's range,
    the output is finite.  A first piece that rounds to inf (a two-piece split of a wider type, an fp16 staging tile)
    turns these rows into NaN."""
    case = BAND_CASES[name](graphs)
    op = anywhere_below_2_127(case.shape, per_sample_big=len(case.shape) == 3)
    got = band_run(hip, case, op, f"{name}, finite operands")
    fmax = torch.finfo(torch.float32).max
    for i, (g_, r64) in enumerate(zip(got, case.ref(op, torch.float64))):
        inside = r64.abs() <= fmax
        assert float(inside.double().mean()) > 0.99, f"{name}: output {i}: the case itself leaves fp32's range"
        bad = ~torch.isfinite(g_.cpu()) & inside
        assert not bool(bad.any()), f"{name}: output {i}: {int(bad.sum())} non-finite elements whose float64 value is in " \
                                    f"range, first {bad.nonzero()[:4].tolist()}"


# ------------------------------------------------------------------------------------------------------------------
# A / B. GCL_LINEAR_IMPL=valu: the plain-VALU dense kernels, in a process of their own (the switch is read once)
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_valu_kernels_contain_and_follow_scales(lib_built, tmp_path):
    """linear_valu_kernel, forward and dX, one child process for all its cases (tests/helpers/valu_child.py): the
    containment cases of the forward with every activation and of dX with PReLU and SiLU, and the scale covariance of
    both."""
    import subprocess

    g = torch.Generator().manual_seed(6)
    Fin, Fout = 48, 64
    mid = poison_rows(ROWS)[1]
    x, W, b = torch.randn(ROWS, Fin, generator=g), torch.randn(Fout, Fin, generator=g) * 0.3, torch.randn(Fout, generator=g)
    dy = torch.randn(ROWS, Fout, generator=g)
    z = negative_at(x, (mid, col_of(mid, Fin)))
    ux, uW, ub, udy = (unit_range(*s, seed=i).cpu() for i, s in enumerate(((ROWS, Fin), (Fout, Fin), (Fout,), (ROWS, Fout))))
    uW = uW / 4
    jobs, checks = [], []  # checks: (kind, index of the clean / unscaled job, what, exponent)
    for act in (0, 1, 2):
        base = len(jobs)
        jobs.append({"op": "fwd", "x": x, "W": W, "b": b, "act": act})
        spots = [("x", (r, col_of(r, Fin)), NAN) for r in poison_rows(ROWS)]
        spots += [("x", (mid, Fin - 1), INF), ("b", (Fout // 2,), NAN), ("W", (Fout - 1, Fin // 2), NAN)]
        for name, idx, val in spots:
            job = dict(jobs[base])
            job[name] = poisoned(job[name], idx, val)
            jobs.append(job)
            checks.append(("contain", base, f"valu fwd act={act}: {val} in {name}{list(idx)}", None))
    for act in (1, 2):
        base = len(jobs)
        jobs.append({"op": "dx", "dy": dy, "W": W, "z": z, "act": act})
        for name, idx in [("dy", (r, col_of(r, Fout))) for r in poison_rows(ROWS)] + [("z", (mid, col_of(mid, Fin)))]:
            job = dict(jobs[base])
            job[name] = poisoned(job[name], idx)
            jobs.append(job)
            checks.append(("contain", base, f"valu dx act={act}: NaN in {name}{list(idx)}", None))
    for act in (0, 1):
        base = len(jobs)
        jobs.append({"op": "fwd", "x": ux, "W": uW, "b": ub, "act": act})
        jobs.append({"op": "dx", "dy": udy, "W": uW, "z": ux, "act": act})
        for kx, kw in [(k, 0) for k in SCALES] + [(0, k) for k in SCALES] + [(-48, -48), (48, 48)]:
            jobs.append({"op": "fwd", "x": ux * 2.0 ** kx, "W": uW * 2.0 ** kw, "b": ub * 2.0 ** (kx + kw), "act": act})
            checks.append(("scale", base, f"valu fwd act={act}: x * 2^{kx}, W * 2^{kw}", kx + kw))
            jobs.append({"op": "dx", "dy": udy * 2.0 ** kx, "W": uW * 2.0 ** kw, "z": ux, "act": act})
            checks.append(("scale", base + 1, f"valu dx act={act}: dy * 2^{kx}, W * 2^{kw}", kx + kw))
    torch.save(jobs, tmp_path / "jobs.pt")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "valu_child.py"), root, str(tmp_path / "jobs.pt"),
                    str(tmp_path / "outs.pt")], check=True, env=dict(os.environ, GCL_LINEAR_IMPL="valu"), timeout=120)
    res = torch.load(tmp_path / "outs.pt")
    names, outs = res["names"], res["outs"]
    ran(names, ("linear_valu_kernel", ["0"]), "valu forward")
    ran(names, ("linear_valu_kernel", ["1"]), "valu dX")
    assert not any(k in n for n in names for k in ("mfma", "x3", "gemm_tile")), names
    scaled = [i for i, job in enumerate(jobs) if not any(i == c[1] for c in checks)]
    assert len(scaled) == len(checks)
    for (kind, base, what, k), i in zip(checks, scaled):
        job = jobs[i]
        if kind == "scale":
            got, ref0 = (outs[i], outs[base]) if job["op"] == "fwd" else (outs[i][0], outs[base][0])
            covariant(ref0, got, k, what)
        elif job["op"] == "fwd":
            ref = act64(job["x"].double(), job["act"], A) @ job["W"].double().t() + job["b"].double()
            contained(outs[base], outs[i], ref, what)
        else:
            ref = bwd_ref(job["z"], job["W"], job["dy"], job["act"])
            keep = 2 if job["act"] == 1 else 1
            contained(outs[base][:keep], outs[i][:keep], [ref["dx"], ref["ds"]][:keep], what)
