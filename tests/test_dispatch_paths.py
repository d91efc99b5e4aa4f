"""The kernels the launchers pick when a gate or a switch moves them off the default path: the fp32-operand fallbacks
(GCL_X3=0, GCL_X3_GCN=0, GCL_X3_TILE=0), the first form of the staged GCN layer (GCL_GCN_HALO_FORM=0), the separate
and 128-row backward (GCL_NO_FUSED_BWD, GCL_NO_FUSED64), the dense kernel choice (GCL_DENSE_IMPL), the row-group order
of agg_kernel (GCL_AGG_ORDER), the Python-side switches of the model, heavy rows on the staged kernels, the `_ok`
queries against the launches they speak for, and the SparseGAT pruning on the compact pipeline.

Every test proves that the path it names ran: kernel names from torch.profiler (HIP kernel names on ROCm) or a query
of the library.  Small-integer inputs on constant-degree graphs make every path BIT-equal to float64; random inputs
are held to the suite's 1e-5 of a float64 reference."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import build_graphs, experiment
from oracle import pyg_ops as P
from oracle import train_step as T

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import has, launched, targs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
X3_SWITCHES = ("GCL_X3", "GCL_X3_GCN", "GCL_X3_TILE", "GCL_GCN_HALO", "GCL_GCN_HALO_FORM", "GCL_NO_FUSED_BWD",
               "GCL_NO_FUSED64", "GCL_DENSE_IMPL", "GCL_FUSED_GCN", "GCL_AGG_HALO", "GCL_AGG_ORDER")


def rel(a, b):
    """max(Frobenius relative error, element-wise max|diff| / max|ref|), as in the rest of the suite."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    fro = ((a - b).norm() / (b.norm() + 1e-30)).item()
    mx = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item() if b.numel() else 0.0
    return max(fro, mx)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture
def env(monkeypatch):
    """Switch setter: starts from the default of every switch; set(name=None) restores a default."""
    for k in X3_SWITCHES:
        monkeypatch.delenv(k, raising=False)

    def set_(**kv):
        for k, v in kv.items():
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, str(v))
    return set_


def ring(n, offs):
    """Every node i receives from i + d for d in offs (mod n): with its self-loop, len(offs) + 1 in-edges each."""
    idx = torch.arange(n)
    return torch.stack([torch.cat([(idx + d) % n for d in offs]), idx.repeat(len(offs))])


def _act64(x, act, a):
    if act == 0:
        return x
    if act == 1:
        return torch.where(x > 0, x, a * x)
    return x * torch.sigmoid(x)


@pytest.fixture(scope="module")
def mesh35():
    """The [3, 5] mesh graph with its nodes in tile order (what the model hands its processor)."""
    from graphcast_lite_amd.mesh import tile_order

    g = build_graphs(experiment("baseline", mesh_levels=[3, 5]))
    n = g["M"]
    deg = torch.bincount(g["proc"][1], minlength=n).numpy()
    order = torch.from_numpy(np.ascontiguousarray(tile_order(g["mesh"].vertices, 64, degree=deg)))
    pos = torch.empty(n, dtype=torch.int64)
    pos[order] = torch.arange(n)
    return dict(n=n, ei=pos[g["proc"]], order=order, pos=pos)


# ------------------------------------------------------------------------------------------------------------------
# GCL_X3=0: the fp32-operand kernels of the dense layers
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Fin,Fout", [(333, 64, 64), (129, 48, 16), (31, 36, 48), (333, 20, 32)])
def test_x3_off_linear_exact_and_accurate(hip, env, rows, Fin, Fout):
    """linear fwd + fused backward with GCL_X3 unset and GCL_X3=0: on small integers both are BIT-equal to float64
    (dX, dW, db, column sums, slope gradient); on random data both are within 1e-5 of float64."""
    g = torch.Generator().manual_seed(7)
    xi = torch.randint(-6, 7, (rows, Fin), generator=g).float()
    Wi = torch.randint(-4, 5, (Fout, Fin), generator=g).float()
    Wi[::3] += 0.5
    bi = torch.randint(-9, 10, (Fout,), generator=g).float()
    dyi = torch.randint(-3, 4, (rows, Fout), generator=g).float()
    xr, Wr, dyr = rnd(rows, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.2), rnd(rows, Fout, seed=4)
    br = rnd(Fout, seed=3)

    def ref64(x, W, b, dy, a):
        x64, W64, a64 = x.double().requires_grad_(), W.double().requires_grad_(), a.double().requires_grad_()
        b64 = b.double().requires_grad_()
        y = torch.where(x64 > 0, x64, a64 * x64) @ W64.t() + b64
        y.backward(dy.double())
        return (x.double() @ W.double().t() + b.double()), x64.grad, W64.grad, b64.grad, a64.grad

    def run(x, W, b, dy, a):
        y = hip.linear_fwd(x.to(DEV), W.to(DEV), b.to(DEV), None)
        dW, db, cs = torch.empty(Fout, Fin, device=DEV), torch.empty(Fout, device=DEV), torch.empty(Fin, device=DEV)
        da = torch.zeros(1, device=DEV)
        dx = hip.linear_bwd_all(dy.to(DEV), W.to(DEV), x.to(DEV), a.to(DEV), da, dW, db, cs, False)
        return [t.cpu().double() for t in (y, dx, dW, db, cs, da)]

    a = torch.tensor([0.5])
    for mode in (None, "0"):
        env(GCL_X3=mode)
        got, names = launched(lambda: run(xi, Wi, bi, dyi, a))
        fused64 = 33 <= Fin <= 64
        if mode is None:
            assert has(names, "linear_x3_fwd_kernel"), names
            assert has(names, "linear_x3_bwd_kernel" if fused64 else "linear_bwd_fused_kernel"), names
        else:
            assert not has(names, "linear_x3_") and not has(names, "gemm_tile_x3"), names
            assert has(names, "linear_mfma_kernel"), names
            assert has(names, "linear_bwd_fused64_kernel" if fused64 else "linear_bwd_fused_kernel"), names
        y64, dx64, dW64, db64, da64 = ref64(xi, Wi, bi, dyi, a)
        for name, t, r in zip(("y", "dx", "dW", "db", "colsum", "d_slope"), got,
                              (y64, dx64, dW64, db64, dx64.sum(0), da64)):
            assert torch.equal(t, r.reshape(t.shape)), f"GCL_X3={mode}: {name} differs from float64 on integers"
        got = run(xr, Wr, br, dyr, torch.tensor([0.25]))
        y64, dx64, dW64, db64, da64 = ref64(xr, Wr, br, dyr, torch.tensor([0.25]))
        for name, t, r, tol in zip(("y", "dx", "dW", "db", "colsum", "d_slope"), got,
                                   (y64, dx64, dW64, db64, dx64.sum(0), da64), (TOL,) * 4 + (1e-4, 1e-4)):
            assert rel(t, r.reshape(t.shape)) < tol, f"GCL_X3={mode}: {name} {rel(t, r.reshape(t.shape)):.3e}"


@pytest.mark.parametrize("Fin,Fout", [(136, 132), (256, 256)])
def test_x3_tile_switches_on_wide_tiles(hip, env, Fin, Fout):
    """gemm_tile_x3_kernel (128-row tiles, enough rows: the default) against gemm_tile_kernel (GCL_X3_TILE=0 and
    GCL_X3=0): bit-equal to float64 on small integers, within 1e-5 of it on random data."""
    rows = 98305  # >= 1536 row tiles of 128 x 2 column tiles: the tile kernels take 128-row tiles (gt_geom)
    g = torch.Generator().manual_seed(11)
    xi = torch.randint(-7, 8, (rows, Fin), generator=g).float()
    Wi = torch.randint(-5, 6, (Fout, Fin), generator=g).float()
    Wi[::3] += 0.5
    bi = torch.randint(-9, 10, (Fout,), generator=g).float()
    refi = (xi.double() @ Wi.double().t() + bi.double()).float()
    xr, Wr, br = rnd(rows, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.1), rnd(Fout, seed=3)
    a = torch.tensor([0.25])
    refr = _act64(xr.double(), 1, a.double()) @ Wr.double().t() + br.double()
    for key, mode in ((None, None), ("GCL_X3_TILE", "0"), ("GCL_X3", "0")):
        env(GCL_X3=None, GCL_X3_TILE=None)
        if key:
            env(**{key: mode})
        got, names = launched(lambda: hip.dense_fwd(xi.to(DEV), Wi.to(DEV), bi.to(DEV), hip.ACT_NONE, None).cpu())
        if key is None:
            assert has(names, "gemm_tile_x3_kernel"), names
        else:
            assert has(names, "gemm_tile_kernel") and not has(names, "gemm_tile_x3_kernel"), names
        assert torch.equal(got, refi), f"{key}={mode}: {(got != refi).sum().item()} elements differ from float64"
        y = hip.dense_fwd(xr.to(DEV), Wr.to(DEV), br.to(DEV), hip.ACT_PRELU, a.to(DEV))
        assert rel(y, refr) < TOL, f"{key}={mode}: {rel(y, refr):.3e}"


# ------------------------------------------------------------------------------------------------------------------
# GCL_DENSE_IMPL: panel vs tile kernels of the general dense entry points
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Fin,Fout", [(129, 260, 132), (1000, 160, 64), (129, 136, 96), (5000, 128, 64)])
@pytest.mark.parametrize("act", [1, 2])
def test_dense_impl_switch(hip, env, rows, Fin, Fout, act):
    """gcl_dense_fwd / bwd_dx / bwd_dw under GCL_DENSE_IMPL unset, =tile and =panel: each within 1e-5 of float64
    autograd (slope gradient 1e-4, as in test_dense_fwd_bwd_wide); =tile never runs the resident-panel kernel."""
    x = rnd(rows, Fin, seed=1).double().requires_grad_()
    W = rnd(Fout, Fin, seed=2, scale=0.1).double().requires_grad_()
    b = rnd(Fout, seed=3).double().requires_grad_()
    a = torch.tensor([0.25], dtype=torch.float64, requires_grad=True)
    dy = rnd(rows, Fout, seed=5).double()
    y = _act64(x, act, a) @ W.t() + b
    y.backward(dy)
    xd, Wd, bd, dyd = x.detach().float().to(DEV), W.detach().float().to(DEV), b.detach().float().to(DEV), dy.float().to(DEV)
    ad = a.detach().float().to(DEV) if act == 1 else None
    panel_fits = {(1000, 160, 64), (129, 136, 96), (5000, 128, 64)}
    for mode in (None, "tile", "panel"):
        env(GCL_DENSE_IMPL=mode)

        def run():
            yd = hip.dense_fwd(xd, Wd, bd, act, ad)
            d_slope = torch.zeros(1, device=DEV) if act == 1 else None
            dxd = hip.dense_bwd_dx(dyd, Wd, xd, act, ad, d_slope)
            dWd, dbd = torch.empty(Fout, Fin, device=DEV), torch.empty(Fout, device=DEV)
            hip.dense_bwd_dw(dyd, xd, dWd, dbd, False, act, ad)
            return yd, dxd, d_slope, dWd, dbd
        (yd, dxd, d_slope, dWd, dbd), names = launched(run)
        if mode == "tile":
            assert not has(names, "linear_mfma_kernel") and has(names, "gemm_tile_kernel"), names
        elif mode == "panel" and (rows, Fin, Fout) in panel_fits:
            assert has(names, "linear_mfma_kernel"), names
        elif mode is None and Fin > 128:
            assert has(names, "gemm_tile_kernel"), names
        assert rel(yd, y) < TOL, (mode, rel(yd, y))
        assert rel(dxd, x.grad) < TOL, (mode, rel(dxd, x.grad))
        assert rel(dWd, W.grad) < TOL and rel(dbd, b.grad) < TOL, (mode, rel(dWd, W.grad), rel(dbd, b.grad))
        if act == 1:
            assert abs(d_slope.item() - a.grad.item()) < 1e-4 * max(1.0, abs(a.grad.item())), mode


# ------------------------------------------------------------------------------------------------------------------
# GCL_NO_FUSED_BWD / GCL_NO_FUSED64: the separate and the 128-row backward
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Fin,Fout", [(1000, 64, 64), (300, 48, 36), (129, 72, 48)])
@pytest.mark.parametrize("switch", ["GCL_NO_FUSED_BWD", "GCL_NO_FUSED64"])
def test_linear_bwd_all_fallbacks(hip, env, rows, Fin, Fout, switch):
    """gcl_linear_bwd_all on its separate kernels (GCL_NO_FUSED_BWD=1: dW, dX, column sums) and on the 128-row fused
    form (GCL_NO_FUSED64=1): bit-equal to float64 on small integers; on random data with every combination of the
    GCL_ACC_DW / GCL_ACC_DB / GCL_ACC_COLSUM bits within the bars of test_linear_bwd_all_accumulate_bits, now of a
    float64 reference, PReLU slope gradient included."""
    env(**{switch: 1})
    g = torch.Generator().manual_seed(3)
    xi = torch.randint(-6, 7, (rows, Fin), generator=g).float()
    Wi = torch.randint(-4, 5, (Fout, Fin), generator=g).float()
    dyi = torch.randint(-3, 4, (rows, Fout), generator=g).float()

    def ref64(x, W, dy, a):
        x64, W64, a64 = x.double().requires_grad_(), W.double().requires_grad_(), a.double().requires_grad_()
        b64 = torch.zeros(Fout, dtype=torch.float64, requires_grad=True)
        (torch.where(x64 > 0, x64, a64 * x64) @ W64.t() + b64).backward(dy.double())
        return x64.grad, W64.grad, b64.grad, x64.grad.sum(0), a64.grad

    def run(x, W, dy, a, bits, fill=(0.0, 0.0, 0.0)):
        dW, db, cs = (torch.full((Fout, Fin), fill[0], device=DEV), torch.full((Fout,), fill[1], device=DEV),
                      torch.full((Fin,), fill[2], device=DEV))
        da = torch.zeros(1, device=DEV)
        dx = hip.linear_bwd_all(dy.to(DEV), W.to(DEV), x.to(DEV), a.to(DEV), da, dW, db, cs, bool(bits & 1),
                                acc_db=bool(bits & 2), acc_colsum=bool(bits & 4))
        return [t.cpu().double() for t in (dx, dW, db, cs, da)]

    a = torch.tensor([0.5])
    got, names = launched(lambda: run(xi, Wi, dyi, a, 0))
    assert not has(names, "linear_x3_bwd_kernel") and not has(names, "linear_bwd_fused64_kernel"), names
    if switch == "GCL_NO_FUSED_BWD":
        assert not has(names, "linear_bwd_fused_kernel") and has(names, "colsum_kernel"), names
    else:
        assert has(names, "linear_bwd_fused_kernel"), names
    for name, t, r in zip(("dx", "dW", "db", "colsum", "d_slope"), got, ref64(xi, Wi, dyi, a)):
        assert torch.equal(t, r.reshape(t.shape)), f"{switch}: {name} differs from float64 on integers"
    x, W, dy, a = rnd(rows, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.2), rnd(rows, Fout, seed=4), torch.tensor([0.25])
    dx64, dW64, db64, cs64, da64 = ref64(x, W, dy, a)
    for bits in range(8):
        dx, dW, db, cs, da = run(x, W, dy, a, bits, fill=(3.0, 5.0, 7.0))
        assert rel(dx, dx64) < TOL, bits
        assert rel(dW - (3.0 if bits & 1 else 0.0), dW64) < 2e-5, bits
        assert rel(db - (5.0 if bits & 2 else 0.0), db64) < 2e-5, bits
        assert rel(cs - (7.0 if bits & 4 else 0.0), cs64) < 1e-4, bits
        assert rel(da, da64) < 1e-4, bits


# ------------------------------------------------------------------------------------------------------------------
# boundaries of the dense plans (csrc/dense_plan.h) the cases above do not reach
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,queued", [(8064, 0), (8065, 1)])
def test_dw_deferral_boundary(hip, env, rows, queued):
    """gcl_dense_bwd_dw_deferred hands its final pass to the queue from 64 partial records on (plan_dw: 128 rows a block
    at these widths, so 8064 rows reduce on the spot and 8065 are queued); deferred + gcl_reduce_jobs is bit-equal to
    the immediate call either way, and both are within 1e-5 of float64."""
    x, dy = rnd(rows, 64, seed=1).to(DEV), rnd(rows, 64, seed=2).to(DEV)
    dW0, db0 = torch.empty(64, 64, device=DEV), torch.empty(64, device=DEV)
    hip.dense_bwd_dw(dy, x, dW0, db0, False)
    dW1, db1 = torch.full((64, 64), 9.0, device=DEV), torch.full((64,), 9.0, device=DEV)
    hip.defer_begin()
    try:
        hip.dense_bwd_dw(dy, x, dW1, db1, False)
        assert (len(hip._deferred.jobs) > 0) == bool(queued), len(hip._deferred.jobs)
    finally:
        hip.defer_flush()
    assert torch.equal(dW0, dW1) and torch.equal(db0, db1)
    assert rel(dW0, dy.double().t() @ x.double()) < TOL and rel(db0, dy.double().sum(0)) < TOL


@pytest.mark.parametrize("Fin", [128, 132])
def test_dw_chunk_boundary(hip, env, Fin):
    """gcl_dense_bwd_dw at one and at two 128-column input chunks (Fin 128 / 132), PReLU on the input: 1e-5 of float64."""
    rows, Fout = 1000, 48
    x, dy, a = rnd(rows, Fin, seed=1), rnd(rows, Fout, seed=2), torch.tensor([0.25])
    dW, db = torch.empty(Fout, Fin, device=DEV), torch.empty(Fout, device=DEV)
    hip.dense_bwd_dw(dy.to(DEV), x.to(DEV), dW, db, False, 1, a.to(DEV))
    assert rel(dW, dy.double().t() @ _act64(x.double(), 1, a.double())) < TOL and rel(db, dy.double().sum(0)) < TOL


@pytest.mark.parametrize("Fout,fused", [(64, True), (68, False)])
def test_linear_bwd_all_fout_boundary(hip, env, Fout, fused):
    """gcl_linear_bwd_all at the widest fused output (64) and just past it (68: the separate kernels): the path ran, and
    dx / dW / db / column sums / slope gradient are within the bars of test_linear_bwd_all_fallbacks of float64."""
    rows, Fin = 1000, 64
    x, W, dy, a = rnd(rows, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.2), rnd(rows, Fout, seed=4), torch.tensor([0.25])
    x64, W64, a64 = x.double().requires_grad_(), W.double().requires_grad_(), a.double().requires_grad_()
    b64 = torch.zeros(Fout, dtype=torch.float64, requires_grad=True)
    (torch.where(x64 > 0, x64, a64 * x64) @ W64.t() + b64).backward(dy.double())

    def run():
        dW, db, cs, da = (torch.empty(Fout, Fin, device=DEV), torch.empty(Fout, device=DEV), torch.empty(Fin, device=DEV),
                          torch.zeros(1, device=DEV))
        dx = hip.linear_bwd_all(dy.to(DEV), W.to(DEV), x.to(DEV), a.to(DEV), da, dW, db, cs, False)
        return dx, dW, db, cs, da
    (dx, dW, db, cs, da), names = launched(run)
    assert has(names, "linear_x3_bwd") == fused and has(names, "dw_mfma_kernel") == (not fused), names
    assert rel(dx, x64.grad) < TOL and rel(dW, W64.grad) < 2e-5 and rel(db, b64.grad) < 2e-5
    assert rel(cs, x64.grad.sum(0)) < 1e-4 and rel(da, a64.grad) < 1e-4


# ------------------------------------------------------------------------------------------------------------------
# GCL_X3_GCN=0, GCL_X3=0, GCL_GCN_HALO_FORM=0: the one-kernel GCN layer
# ------------------------------------------------------------------------------------------------------------------
GCN_MODES = ((None, None), ("GCL_GCN_HALO_FORM", "0"), ("GCL_X3_GCN", "0"), ("GCL_X3", "0"))


def _check_gcn_kernels(names, key):
    halo = targs(names, "gcn_halo_fwd_kernel")
    per_edge = targs(names, "gcn_fwd_kernel")
    if key is None:  # interleaved-issue form: <ACT, 4, 2, DIRECT = true, INTER = true, TAB = false>
        assert halo and all(t[1] == "4" and t[3] == "true" for t in halo) and not per_edge, names
    elif key == "GCL_GCN_HALO_FORM":  # first form: <ACT, 4, 0, false, false, false>
        assert halo and all(t[1] == "4" and t[3] == "false" for t in halo) and not per_edge, names
    else:  # per-edge kernel on fp32 operands: gcn_fwd_kernel<NS, ACT, EW, NW, SAFE, X3 = false>
        assert not halo and per_edge and all(t[5] == "false" for t in per_edge), names


@pytest.mark.parametrize("act", [0, 1])
def test_gcn_layer_switches_exact_on_ring(hip, env, act):
    """A ring with sixteen in-edges per row (edge weight 1/16) and small integers: the staged layer in both forms and
    the per-edge fp32-operand layer are all BIT-equal to float64 (PReLU slope 0.5 keeps it exact)."""
    n, Fin, Fout, B = 64 * 9 + 5, 64, 64, 3
    offs = [d for d in range(-7, 9) if d != 0]
    gh = hip.Graph(ring(n, offs), n, hip.GRAPH_GCN)
    assert gh.halo_info(False, 64) is not None
    g = torch.Generator().manual_seed(13)
    x = torch.randint(-7, 8, (B, n, Fin), generator=g).float()
    W = torch.randint(-5, 6, (Fout, Fin), generator=g).float()
    W[::3] += 0.5
    b = torch.randint(-9, 10, (Fout,), generator=g).float()
    a = torch.tensor([0.5])
    idx = torch.arange(n)
    xa = _act64(x.double(), act, 0.5)
    agg = (xa + sum(xa[:, (idx + d) % n] for d in offs)) / 16.0
    ref = (agg @ W.double().t() + b.double()).float()
    sl = a.to(DEV) if act == 1 else None
    for key, mode in GCN_MODES:
        env(**{k: None for k, _ in GCN_MODES if k})
        if key:
            env(**{key: mode})
        got, names = launched(lambda: hip.gcn_layer_fwd(gh, x.to(DEV), act, sl, W.to(DEV), b.to(DEV)).cpu())
        _check_gcn_kernels(names, key)
        assert torch.equal(got, ref), f"{key}={mode}: {(got != ref).sum().item()} elements differ from float64"


@pytest.mark.parametrize("act", [0, 1, 2])
def test_gcn_layer_switches_on_mesh(hip, env, mesh35, act):
    """The [3, 5] mesh in tile order, random data: every form of the layer within 1e-5 of float64 GCNConv."""
    n, B, Fin, Fout = mesh35["n"], 3, 64, 64
    gh = hip.Graph(mesh35["ei"], n, hip.GRAPH_GCN)
    x, W, b = rnd(B, n, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.2), rnd(Fout, seed=3)
    a = torch.tensor([0.25])
    xa = _act64(x.double(), act, a.double())
    ref = torch.stack([P.gcn_conv(xa[i], mesh35["ei"], W.double(), b.double()) for i in range(B)])
    sl = a.to(DEV) if act == 1 else None
    for key, mode in GCN_MODES:
        env(**{k: None for k, _ in GCN_MODES if k})
        if key:
            env(**{key: mode})
        got, names = launched(lambda: hip.gcn_layer_fwd(gh, x.to(DEV), act, sl, W.to(DEV), b.to(DEV)).cpu())
        _check_gcn_kernels(names, key)
        assert rel(got, ref) < TOL, f"{key}={mode}: {rel(got, ref):.3e}"


# ------------------------------------------------------------------------------------------------------------------
# Heavy rows (> 64 in-edges) on graphs with a source-tile layout
# ------------------------------------------------------------------------------------------------------------------
def test_heavy_row_gcn_layer_through_row_table_is_refused(hip):
    """gcn_halo_fwd_kernel has no records for a heavy row: gcl_gcn_layer_fwd_tab must refuse such a graph (it used to
    return bias only for that row), the query must say so, and the two-kernel path the model takes instead must be
    right."""
    n, Fin, Fout, B = 64 * 9 + 5, 64, 48, 2
    heavy_row = 300
    rng = np.random.default_rng(5)
    ring_ei = ring(n, [d for d in range(-7, 9) if d != 0])
    far = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n), np.arange(heavy_row - 8, heavy_row + 9)), 64, replace=False))
    ei = torch.cat([ring_ei, torch.stack([far, torch.full_like(far, heavy_row)])], 1)
    gh = hip.Graph(ei, n, hip.GRAPH_GCN)
    assert gh.halo_info(False, 64) is not None and gh.max_in_degree == 80
    x, W, b = rnd(B, n, Fin, seed=1), rnd(Fout, Fin, seed=2, scale=0.2), rnd(Fout, seed=3)
    xd = x.to(DEV)
    assert not hip.gcn_layer_tab_ok(gh, xd, Fout)
    tab = torch.arange(n, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="heavy rows"):
        hip.gcn_layer_fwd_tab(gh, xd, tab, hip.ACT_NONE, None, W.to(DEV), b.to(DEV))
    assert not hip.gcn_layer_fusable(gh, xd, Fin, Fout)
    h = hip.linear_fwd(xd.reshape(B * n, Fin), W.to(DEV), None, None).reshape(B, n, Fout)
    got = hip.aggregate(gh, h, b.to(DEV))
    ref = torch.stack([P.gcn_conv(x[i].double(), ei, W.double(), b.double()) for i in range(B)])
    assert rel(got, ref) < TOL
    assert rel(got[:, heavy_row], ref[:, heavy_row]) < TOL


def test_heavy_row_gat_on_tile_graph(hip, mesh35):
    """The one-head GAT kernels on a source-tile graph fall back to the per-edge kernels when a row has more than 64
    in-edges (gat.hip: n_heavy in all three gates): forward and backward against the oracle at test_gat_fwd_bwd's bars."""
    n, H, C, B, Fin = mesh35["n"], 1, 64, 2, 24
    rng = np.random.default_rng(9)
    heavy_row = 4000
    own = mesh35["ei"][0][mesh35["ei"][1] == heavy_row]
    far = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n), np.append(own.numpy(), heavy_row)), 70, replace=False))
    ei_ref = torch.cat([mesh35["ei"], torch.stack([far, torch.full_like(far, heavy_row)])], 1)
    G = hip.Graph(ei_ref, n, hip.GRAPH_GAT)
    assert G.halo_info(False, 64) is not None and G.max_in_degree > 64
    assert not hip.gat_tab_ok(G, H, C)
    x = rnd(B, n, Fin, seed=1).requires_grad_()
    W = rnd(H * C, Fin, seed=2, scale=0.3).requires_grad_()
    a_s, a_d = rnd(1, H, C, seed=3, scale=0.3).requires_grad_(), rnd(1, H, C, seed=4, scale=0.3).requires_grad_()
    b = rnd(C, seed=5).requires_grad_()
    y_ref, ei2, alpha_ref = P.gat_conv(x, ei_ref, W, a_s, a_d, b, H)
    dy = rnd(B, n, C, seed=6)
    y_ref.backward(dy)
    h_ref = x.detach() @ W.detach().t()
    hd = h_ref.to(DEV)
    asd, add_ = a_s.detach().reshape(-1).to(DEV), a_d.detach().reshape(-1).to(DEV)
    (y, s_src, s_dst, alpha), names = launched(lambda: hip.gat_fwd(G, hd, asd, add_, b.detach().to(DEV), H, C))
    assert not has(names, "gat_halo"), names
    assert rel(y, y_ref) < TOL
    assert rel(y[:, heavy_row], y_ref[:, heavy_row]) < TOL
    al_e = torch.stack([hip.gat_alpha_edge_order(G, alpha[i], H) for i in range(B)])
    assert rel(al_e, alpha_ref) < TOL
    d_as, d_ad, d_b = torch.empty(H * C, device=DEV), torch.empty(H * C, device=DEV), torch.empty(C, device=DEV)
    dh, names = launched(lambda: hip.gat_bwd(G, dy.to(DEV), hd, asd, add_, s_src, s_dst, alpha, d_as, d_ad, d_b, False, H, C))
    assert not has(names, "gat_halo"), names
    dW = dh.reshape(-1, H * C).t().cpu().double() @ x.detach().reshape(-1, Fin).double()
    assert rel(dW, W.grad) < 5e-5
    dx = dh.cpu().double() @ W.detach().double()
    assert float((dx - x.grad).norm() / x.grad.norm()) < 5e-5
    assert rel(dx[:, heavy_row], x.grad[:, heavy_row]) < 5e-5
    assert rel(d_as.cpu(), a_s.grad.reshape(-1)) < 5e-5 and rel(d_ad.cpu(), a_d.grad.reshape(-1)) < 5e-5
    assert rel(d_b, b.grad) < TOL


# ------------------------------------------------------------------------------------------------------------------
# The `_ok` queries and the launchers read one dispatch plan (csrc/tile_plan.h): a query says 1 exactly when the call runs
# ------------------------------------------------------------------------------------------------------------------
def _plan_graph(which, mesh35):
    """(edge list, n, pieces per wave of its tiles or None with a heavy row) of the ring with n = 64 * 9 + 5 rows, or of
    the [3, 5] mesh in tile order (at most 64 halo rows per tile)."""
    if which == "mesh35":
        return mesh35["ei"], mesh35["n"], 4
    n = 64 * 9 + 5
    near = ring(n, [d for d in range(-7, 9) if d != 0])  # sixteen in-edges per row: 16 halo rows per tile, 1 piece
    if which == "ring16":
        return near, n, 4
    if which == "ring40":  # offsets out to +-40: 80 halo rows per tile = 5 pieces per wave (the 8-piece kernels)
        return ring(n, [-40, -30, -20, -10, -1, 1, 10, 20, 30, 40]), n, 8
    rng = np.random.default_rng(5)  # the graph of test_heavy_row_gcn_layer_through_row_table_is_refused
    far = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n), np.arange(300 - 8, 300 + 9)), 64, replace=False))
    return torch.cat([near, torch.stack([far, torch.full_like(far, 300)])], 1), n, None


def _attempt(fn):
    """fn(), or None for a refused call: a RuntimeError from a return code, nothing launched."""
    try:
        return fn()
    except RuntimeError as exc:
        assert "libgcl_hip error" in str(exc), exc
        return None


@pytest.mark.parametrize("width", [32, 48, 64])
@pytest.mark.parametrize("which", ["ring16", "ring40", "heavy", "mesh35"])
def test_queries_agree_with_launches(hip, env, mesh35, which, width):
    """gcn_layer_tab_ok, gcn_layer_split_ok, aggregate_compact_ok and gat_tab_ok against the calls they speak for, with
    the source-tile switches on and off, and the kernel and template arguments of the form the plan implies.  (The
    source-tile aggregation needs the 8-wide edge prefix; on a ring every prefix width costs the same and the graph
    takes the narrowest, so only the mesh has a store map.)"""
    ei, n, pieces = _plan_graph(which, mesh35)
    B, Fout, head = 2, 48, 256
    gh, G = hip.Graph(ei, n, hip.GRAPH_GCN), hip.Graph(ei, n, hip.GRAPH_GAT)
    assert gh.halo_info(False, 64) is not None and G.halo_info(True, 64) is not None
    x, dy = rnd(B, n, width, seed=1).to(DEV), rnd(B, n, width, seed=6).to(DEV)
    W, b, att = rnd(Fout, width, seed=2, scale=0.2).to(DEV), rnd(Fout, seed=3).to(DEV), rnd(width, seed=4, scale=0.3).to(DEV)
    tab = torch.arange(n, dtype=torch.int32, device=DEV)
    ya, yb = torch.empty(B, head, Fout, device=DEV), torch.empty(B, n - head, Fout, device=DEV)
    outc = torch.empty(B, 8, width, device=DEV)
    smap = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    smap[:8] = torch.arange(8, dtype=torch.int32)
    dpar = [torch.empty(width, device=DEV) for _ in range(3)]
    nodes, edges = torch.empty(B, n, 1, device=DEV), torch.empty(B, G.e, 1, device=DEV)  # stand-ins for a refused gat_fwd

    def every():
        """Which of the calls ran; the plain layer (no query: it always has a kernel without heavy rows) runs last."""
        ran = dict(tab=_attempt(lambda: hip.gcn_layer_fwd_tab(gh, x, tab, hip.ACT_NONE, None, W, b)) is not None,
                   split=_attempt(lambda: hip.gcn_layer_fwd_split(gh, x, hip.ACT_NONE, None, W, b, ya, yb) or True) is not None,
                   compact=_attempt(lambda: hip.aggregate_compact(gh, x, smap, outc)) is not None)
        fwd = _attempt(lambda: hip.gat_fwd(G, x, att, att, None, 1, width, tab=tab))
        _, a_s, a_d, alpha = fwd or (None, nodes, nodes, edges)
        bwd = _attempt(lambda: hip.gat_bwd(G, dy, x, att, att, a_s, a_d, alpha, *dpar, False, 1, width, tab=tab))
        ran["gat"] = fwd is not None
        assert (bwd is not None) == ran["gat"]
        if pieces is not None:
            hip.gcn_layer_fwd(gh, x, hip.ACT_NONE, None, W, b)
        return ran

    for on in (True, False):
        env(GCL_GCN_HALO=None if on else 0, GCL_GAT_HALO=None if on else 0, GCL_AGG_HALO=None if on else 0)
        tiles = on and pieces is not None  # heavy rows have no records in the tile layout
        gcn_tile = tiles and width > 32    # 48- and 64-wide inputs
        want = dict(tab=gcn_tile and pieces == 4, split=pieces is not None and not gcn_tile,
                    compact=tiles and width > 32 and which == "mesh35", gat=tiles and width == 64)
        assert hip.gcn_layer_tab_ok(gh, x, Fout) == want["tab"]
        assert hip.gcn_layer_split_ok(gh, x, Fout, ya, yb) == want["split"]
        assert hip.aggregate_compact_ok(gh, x) == want["compact"]
        assert hip.gat_tab_ok(G, 1, width) == want["gat"]
        if pieces is None:  # every call is refused: no kernel for the profiler to record
            assert every() == want
            continue
        ran, names = launched(every)
        assert ran == want
        form = ["4", "2", "true", "true"] if pieces == 4 else ["8", "2", "true", "false"]  # MAXPW, STAUX, DIRECT, INTER
        halo = ([form + ["false", "false"]] if gcn_tile else []) + ([form + ["true", "false"]] if want["tab"] else [])  # TAB, PRED
        assert sorted(t[1:] for t in targs(names, "gcn_halo_fwd_kernel")) == sorted(halo), names
        x3 = "true" if width % 16 == 0 else "false"  # gcn_fwd_kernel<NS, ACT, EW, NW, SAFE, X3, SPLIT>
        edge = ([] if gcn_tile else [[x3, "false"]]) + ([["true", "true"]] if want["split"] else [])
        assert sorted(t[5:] for t in targs(names, "gcn_fwd_kernel")) == sorted(edge), names
        assert targs(names, "agg_halo_loop_kernel") == ([["16", "64", str(pieces), "false", "true"]] if want["compact"] else []), names
        for kern, args in (("gat_halo_fwd_kernel", ["16", str(pieces), "true"]), ("gat_halo_bwd_dst_kernel", ["16", str(pieces), "true"]),
                           ("gat_halo_bwd_src_kernel", ["16", str(pieces)])):
            assert targs(names, kern) == ([args] if want["gat"] else []), names


# ------------------------------------------------------------------------------------------------------------------
# order16: agg_kernel's processing order of 16-row groups (graphs >= 32768 rows without a tile layout)
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bipartite_40k(hip):
    """A bipartite graph of 40 007 nodes: 30 000 senders, 10 007 receivers with 3..12 random senders each, a few
    receivers with 70..300 senders and a few senders with 100 receivers (heavy rows both ways)."""
    rng = np.random.default_rng(17)
    n, ns = 40_000 + 7, 30_000
    recv = np.arange(ns, n)
    deg = rng.integers(3, 13, recv.size)
    for r, d in ((0, 300), (77, 70), (recv.size - 1, 90)):
        deg[r] = d
    dst = np.repeat(recv, deg)
    src = rng.integers(0, ns, dst.size)
    for s in (5, 12_345, ns - 1):
        src[rng.choice(dst.size, 100, replace=False)] = s
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    ei = ei[:, torch.from_numpy(np.unique(ei.numpy(), axis=1, return_index=True)[1]).sort().values]  # no duplicates
    return n, ei


@pytest.mark.parametrize("F", [16, 64, 128, 200])
def test_agg_row_group_order(hip, env, bipartite_40k, F):
    """gcl_aggregate on the same graph built with GCL_AGG_ORDER unset (order16 on) and =0: torch.equal, forward and
    transposed, B = 1 and 3, and within 1e-5 of float64.  F covers both sides of the RPW * 4 * iter <= 16 gate: at F = 16
    a block holds more than 16 rows and runs without the map; at 128 and 200 blocks run whole 16-row groups through
    it, including the masked tail group (n % 16 = 7)."""
    n, ei = bipartite_40k
    graphs = {}
    for mode in (None, "0"):
        env(GCL_AGG_ORDER=mode)
        G = hip.Graph(ei, n, hip.GRAPH_GCN)
        for tr in (False, True):
            assert G.halo_info(tr, 64) is None and G.halo_info(tr, 32) is None
            assert G.row_group_order(tr) == (mode is None)
        graphs[mode] = G
    assert graphs[None].max_in_degree > 64
    e2, w = P.gcn_norm(ei, n, torch.float64)
    for B in (1, 3):
        h = rnd(B, n, F, seed=B)
        bias = rnd(F, seed=9)
        hd, bd = h.to(DEV), bias.to(DEV)
        ref = P._propagate_sum(h.double(), e2, w, n) + bias.double()
        h64 = h.double().requires_grad_()
        P._propagate_sum(h64, e2, w, n).backward(h.double())
        for tr in (False, True):
            outs = {}
            for mode in (None, "0"):  # both outputs alive and pre-filled: a row that is not written cannot match
                outs[mode] = torch.full((B, n, F), float("nan"), device=DEV)
                hip.aggregate(graphs[mode], hd, None if tr else bd, transpose=tr, out=outs[mode])
            assert torch.equal(outs[None], outs["0"]), f"F={F} B={B} transpose={tr}: order16 on/off differ"
            assert rel(outs[None], h64.grad if tr else ref) < TOL


# ------------------------------------------------------------------------------------------------------------------
# Whole model: GCL_X3=0, and the Python-side switches
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,levels,B", [("baseline", [3, 5], 3), ("wb2_512x256_19f_ar", [1, 2], 2)])
def test_model_with_x3_off(env, name, levels, B):
    """One forward + backward with GCL_X3=0: no split-operand kernel runs; output within 1e-5 of the oracle, loss
    too, every gradient under the fp64-arbitrated rule (tests/parity.py)."""
    from test_hip_model import arbitrated_grad_check, data, make_pair

    from graphcast_lite_amd.train import batch_loss, get_lat_weights

    env(GCL_X3=0)
    cfg, m, o = make_pair(name, levels)
    X, y = data(cfg, m._num_grid_nodes, B)
    lw = T.get_lat_weights(32, 64)

    def step():
        out = m(X.to(DEV))
        loss = batch_loss(m, X.to(DEV), y.to(DEV), lat_weights=get_lat_weights(32, 64, DEV))
        loss.backward()
        return out.detach(), loss.detach()
    (out_h, loss_h), names = launched(step)
    assert not [k for k in names if "x3" in k], [k for k in names if "x3" in k]
    assert not has(names, "gcn_halo_fwd_kernel"), names
    assert has(names, "linear_mfma_kernel") and has(names, "linear_bwd_fused"), names
    for args in targs(names, "gcn_fwd_kernel"):
        assert args[5] == "false", names
    out_o = o(X)
    assert rel(out_h, out_o) < TOL, f"forward differs: {rel(out_h, out_o):.3e}"
    loss_o = T.train_step_loss(o, X, y, lat_weights=lw)
    loss_o.backward()
    assert rel(loss_h, loss_o) < TOL
    arbitrated_grad_check(m, o, lambda o64: T.train_step_loss(o64, X.double(), y.double(), lat_weights=lw.double()),
                          f"GCL_X3=0 {name}{levels}B{B}")


def test_model_python_switches(env, monkeypatch):
    """baseline [3, 5], B = 3: the default pipeline against each fallback it can be switched to - GCL_FUSED_GCN=0
    (two-kernel GCN layers), reference mesh numbering (GCL_NO_RENUMBER), the encoder MLP on all rows
    (GCL_NO_MLP_FOLD), the unfused LayerNorm column sums (GCL_NO_LN_COLSUM) and every row of the last decoder layer
    (GCL_NO_ROWS_OUT).  Outputs are bit-equal where only independent rows move, else within 2e-6; gradients as in
    test_general_path_matches_compact_path."""
    from test_hip_model import data, make_pair

    from graphcast_lite_amd import functional
    from graphcast_lite_amd.train import batch_loss

    cfg, m, o = make_pair("baseline", [3, 5])
    X, y = data(cfg, m._num_grid_nodes, 3)
    Xd, yd = X.to(DEV), y.to(DEV)

    def run(model):
        model.zero_grad(set_to_none=True)
        out, names = launched(lambda: model(Xd).detach().clone())
        batch_loss(model, Xd, yd).backward()
        return out, {n_: p.grad.clone() for n_, p in model.named_parameters()}, names

    out0, g0, names0 = run(m)
    assert rel(out0, o(X)) < TOL
    assert m._compact_eligible() and m._compact.perm is not None and m._compact.fold[3].rd > 0
    assert has(names0, "gcn_fwd_kernel") or targs(names0, "gcn_halo_fwd_kernel"), names0
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g0.values())))

    def same_grads(g, tag):
        for n_, gr in g.items():
            d = float((gr.double() - g0[n_].double()).norm())
            assert d <= 2e-5 * float(g0[n_].double().norm()) + 1e-6 * gn, f"{tag}: {n_}"

    env(GCL_FUSED_GCN=0)
    out, g, names = run(m)
    assert not has(names, "gcn_fwd_kernel"), names
    assert all(t[5] == "true" for t in targs(names, "gcn_halo_fwd_kernel")), names  # only the row-table layer stays
    assert rel(out, out0) < 2e-6
    same_grads(g, "GCL_FUSED_GCN=0")
    env(GCL_FUSED_GCN=None)

    for attr, tag in (("_LN_COLSUM", "GCL_NO_LN_COLSUM"), ("_ROWS_OUT", "GCL_NO_ROWS_OUT")):
        assert getattr(functional, attr)
        monkeypatch.setattr(functional, attr, False)
        out, g, _ = run(m)
        assert torch.equal(out, out0), tag
        same_grads(g, tag)
        monkeypatch.setattr(functional, attr, True)

    m._mlp_on_folded_rows = False
    out, g, _ = run(m)
    assert torch.equal(out, out0), "GCL_NO_MLP_FOLD"
    same_grads(g, "GCL_NO_MLP_FOLD")

    _, m2, _ = make_pair("baseline", [3, 5])
    m2._renumber_mesh = False  # before the first forward: the permutation is cached with the compact setup
    out, g, _ = run(m2)
    assert m2._compact.perm is None
    assert rel(out, out0) < 2e-6
    same_grads(g, "GCL_NO_RENUMBER")


# ------------------------------------------------------------------------------------------------------------------
# SparseGAT on the compact pipeline (tile-order mesh): the public processing_graph after pruning
# ------------------------------------------------------------------------------------------------------------------
def test_sparse_gat_prune_on_compact_path():
    """wb2_512x256_sparse_gat (GCN encoder / decoder, so the compact renumbered pipeline runs) on a 64 x 32 grid:
    after `batch_num == 0` prunes, `processing_graph` is the reference's list column for column (self-loops ascending
    by node id), the next forward runs on it, and its identity is stable afterwards."""
    from test_hip_model import data, make_pair

    cfg, m, o = make_pair("wb2_512x256_sparse_gat", [1, 2])
    assert m.using_sparse_gat and m._compact_eligible() and m._mesh_order() is not None
    X, _ = data(cfg, m._num_grid_nodes, 2)
    e0, M = m.processing_graph.shape[1], m._num_mesh_nodes
    t = 0.12
    with torch.no_grad():
        out_h = m(X=X.to(DEV), attention_threshold=t, batch_num=0)
        out_o = o(X=X, attention_threshold=t, batch_num=0)
    assert m._compact.perm is not None and m._proc_tiled[2] is m.processing_graph, "the compact renumbered path did not run"
    assert rel(out_h, out_o) < TOL
    assert m.processing_graph.shape[1] < e0 + M, "nothing was pruned"
    assert torch.equal(m.processing_graph.cpu(), o.processing_graph)
    with torch.no_grad():
        out_h = m(X=X.to(DEV), attention_threshold=t, batch_num=1)
        out_o = o(X=X, attention_threshold=t, batch_num=1)
    assert rel(out_h, out_o) < TOL
    assert torch.equal(m.processing_graph.cpu(), o.processing_graph)
    g1, tiled1 = m.processing_graph, m._processing_graph_tiled()
    with torch.no_grad():
        m(X=X.to(DEV), attention_threshold=t, batch_num=2)
    assert m.processing_graph is g1 and m._processing_graph_tiled() is tiled1
