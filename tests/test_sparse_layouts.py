"""The graph kernels (csrc/aggregate.hip, csrc/gcn_layer.hip, csrc/gat.hip, csrc/interaction.hip) through the C ABI on
padded, strided, offset and column-block rows with a gap between the samples: the contract of tests/test_dense_layouts.py
(NaN around every input, a sentinel around every output, NaN padding bit-equal to zero padding, float64 references,
refusals that leave the output alone) on graphs that are the smallest to reach each path - the [1, 2] mesh (per-edge
kernels), the tile-ordered [2, 3] mesh (source-tile kernels), a ring with one heavy row, and a seeded degree-edge graph
whose in-degrees sit on both sides of the ELL width (8), the register-held records (16) and the heavy-row limit (64),
with duplicate edges and self-loops in its list."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import build_graphs, experiment
from oracle import pyg_ops as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from layouts import DEV, NAN, SENT, U, Rows, has, launched, same_bits, targs, within  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL = -1
B = 3
DEGREES = (1, 2, 4, 5, 8, 9, 10, 16, 17, 18, 64, 65, 66)  # with the appended self-loop; one less without it (GCL_GRAPH_MEAN)


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def rnd(*shape, seed, scale=1.0):
    """CPU generator: the inputs are the same on every machine (the softmax constant below was measured on them)."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def ring(n, offs):
    idx = torch.arange(n)
    return torch.stack([torch.cat([(idx + d) % n for d in offs]), idx.repeat(len(offs))])


def degree_edge_graph(cap=None):
    """300 nodes; node i < 5 * len(DEGREES) receives DEGREES[i % 13] - 1 edges from other nodes (every third node draws
    them from eight senders only, so its list holds duplicates), the rest 1..11; node 7 sends to every row with more than
    two edges (a heavy row of the transpose); every fourth node also lists a self-loop.  cap drops the in-degrees above it."""
    rng = np.random.default_rng(41)
    n = 300
    src, dst = [], []
    for i in range(n):
        d = DEGREES[i % len(DEGREES)] if i < 5 * len(DEGREES) else int(rng.integers(2, 13))
        if cap is not None and d > cap:
            d = cap
        others = np.setdiff1d(np.arange(n), [i])
        pool = others[:8] if i % 3 == 0 else others
        s = rng.choice(pool, d - 1, replace=(i % 3 == 0 or d - 1 > pool.size))
        if d - 1 > 2 and i != 7:
            s[0] = 7
        if i % 4 == 0:
            src.append(i)
            dst.append(i)
        src.extend(s.tolist())
        dst.extend([i] * (d - 1))
    ei = torch.tensor([src, dst], dtype=torch.int64)
    perm = torch.from_numpy(rng.permutation(ei.shape[1]))
    return n, ei[:, perm]


@pytest.fixture(scope="module")
def graphs():
    """name -> (n, edge list); built once, never changed."""
    g12 = build_graphs(experiment("baseline", mesh_levels=[1, 2]))
    from test_hip_ops import _tiled

    g23 = build_graphs(experiment("baseline", mesh_levels=[2, 3]))
    n_r = 64 * 9 + 5
    rng = np.random.default_rng(5)
    far = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n_r), np.arange(300 - 8, 300 + 9)), 64, replace=False))
    heavy_ring = torch.cat([ring(n_r, [d for d in range(-7, 9) if d != 0]), torch.stack([far, torch.full_like(far, 300)])], 1)
    out = {"mesh12": (g12["M"], g12["proc"]), "mesh23_tiled": (g23["M"], _tiled(g23)[0]), "heavy_ring": (n_r, heavy_ring),
           "degree": degree_edge_graph(), "degree64": degree_edge_graph(cap=64)}
    n, ei = out["degree"]
    e2 = P.add_self_loops(P.remove_self_loops(ei), n)
    assert set(DEGREES) <= set(torch.bincount(e2[1], minlength=n).tolist())
    assert {0, 1, 4, 8, 9, 16, 17, 64, 65} <= set(torch.bincount(ei[1], minlength=n).tolist())
    assert int((ei[0] == ei[1]).sum()) > 0 and torch.unique(ei, dim=1).shape[1] < ei.shape[1]
    return out


def edges_of(kind, n, ei, hip):
    """(edge list the kernels sum over, float64 weights) as the reference layer defines them."""
    if kind == hip.GRAPH_MEAN:
        deg = torch.bincount(ei[1], minlength=n).double().clamp(min=1)
        return ei, 1.0 / deg[ei[1]]
    return P.gcn_norm(ei, n, torch.float64)


# ------------------------------------------------------------------------------------------------------------------
# gcl_aggregate
# ------------------------------------------------------------------------------------------------------------------
AGG_CASES = [  # graph, kind, F, layout of h, layout of y -> agg_kernel<.., VL, VS, ..> (and the heavy kernel's)
    ("mesh12", "gcn", 64, "pad_nan", "pad_nan"), ("mesh12", "gcn", 64, "colblock", "colblock"),
    ("mesh12", "gcn", 33, "tight", "tight"), ("mesh12", "gcn", 33, "pad_nan", "odd_ld"),
    ("mesh12", "gcn", 64, "odd_ld", "pad_nan"), ("mesh12", "gcn", 64, "offset", "offset"),
    ("mesh12", "gcn", 33, "contig", "contig"), ("mesh12", "gcn", 12, "tight", "colblock"),
    ("degree", "gcn", 64, "pad_nan", "pad_nan"), ("degree", "gcn", 33, "tight", "tight"),
    ("degree", "gcn", 64, "odd_ld", "colblock"), ("degree", "gcn", 33, "odd_ld", "offset"),
    ("degree", "mean", 64, "colblock", "pad_nan"), ("degree", "mean", 33, "tight", "odd_ld"),
    ("degree", "mean", 64, "offset", "pad_nan"), ("degree", "mean", 12, "contig", "contig"),
    ("heavy_ring", "gcn", 64, "pad_nan", "pad_nan"), ("heavy_ring", "gcn", 33, "tight", "pad_nan"),
    ("heavy_ring", "gcn", 64, "odd_ld", "pad_nan"), ("heavy_ring", "gcn", 33, "contig", "odd_ld"),
    ("mesh23_tiled", "gcn", 64, "pad_nan", "pad_nan"), ("mesh23_tiled", "gcn", 64, "colblock", "colblock"),
    ("mesh23_tiled", "gcn", 64, "pad_nan", "offset"), ("mesh23_tiled", "gcn", 33, "tight", "tight"),
]


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("gname,kind,F,lh,ly", AGG_CASES)
def test_aggregate_layouts(hip, graphs, monkeypatch, gname, kind, F, lh, ly, transpose):
    """gcl_aggregate, both directions, with and without bias: |y - ref| <= (deg + 3) U sum_e |w_e h_e| + U |bias| of
    a float64 index_add restatement; vector loads on rows of roundup(F, 4) floats (F = 33 on 36) fetch the padding and
    must not use it."""
    n, ei = graphs[gname]
    k = hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN
    G = hip.Graph(ei, n, k)
    e2, w = edges_of(k, n, ei, hip)
    if transpose:
        e2 = e2.flip(0)
    h = rnd(B, n, F, seed=F + n)
    bias = rnd(F, seed=3)
    h64 = h.double()
    deg = torch.bincount(e2[1], minlength=n).double()
    ref = P._propagate_sum(h64, e2, w, n)
    tol = (deg[None, :, None] + 3) * U * P._propagate_sum(h64.abs(), e2, w.abs(), n)
    L = hip.lib()
    hd, bd = h.to(DEV), bias.to(DEV)
    what = f"aggregate {gname} {kind} F={F} h:{lh} y:{ly} transpose={transpose}"

    def run(fill, with_bias):
        H_, Y = Rows.of(hd, lh, fill), Rows(n, F, ly, SENT, "out", B=B)
        rc = L.gcl_aggregate(G.handle, int(transpose), H_.ptr, H_.ld, H_.bs, bd.data_ptr() if with_bias else None, Y.ptr,
                             Y.ld, Y.bs, B, F, hip._stream())
        return rc, H_, Y

    for with_bias, tiles_off in ((True, False), (False, False), (True, True)):
        if tiles_off:  # where the source-tile kernel ran, the per-edge kernel on the same rows: GCL_AGG_HALO=0
            if not halo:
                break
            monkeypatch.setenv("GCL_AGG_HALO", "0")
        (rc, H_, Y), names = launched(lambda: run(NAN, with_bias))
        hip._check(rc)
        vl = "true" if H_.aligned() else "false"
        vs = "true" if Y.aligned() and F % 4 == 0 else "false"
        # 16-byte rows of more than 32 floats on a graph with a source-tile layout may run the source-tile kernel (the
        # launch code has further gates, all of them about speed); the tile-ordered mesh is there to make it run
        may_halo = (not tiles_off and vl == vs == "true" and F > 32
                    and any(G.halo_info(transpose, T) is not None for T in (64, 32)))
        halo = has(names, "agg_halo_loop_kernel")
        got = targs(names, "agg_kernel")
        assert halo != bool(got) and (may_halo or not halo), f"{what}: {names}"
        if gname == "mesh23_tiled" and vl == vs == "true" and F > 32 and not tiles_off:
            assert halo, f"{what}: the source-tile kernel did not run: {names}"
        assert all(t[1] == vl and t[2] == vs for t in got), f"{what}: {names}"
        heavy = targs(names, "agg_heavy_kernel")
        assert bool(heavy) == (int(deg.max()) > 64), f"{what}: {names}"
        assert all(t[1] == vl and t[2] == vs for t in heavy), f"{what}: {names}"
        print(f"ran: {'agg_halo_loop_kernel' if halo else 'agg_kernel<' + ', '.join(got[0]) + '>'}"
              f"{' + agg_heavy_kernel<' + ', '.join(heavy[0]) + '>' if heavy else ''}  [{what}]")
        assert Y.untouched(SENT), f"{what}: wrote outside y[:, :, :F] (padding, rows past n or the batch gap)"
        rc0, _, Y0 = run(0.0, with_bias)
        hip._check(rc0)
        assert same_bits(Y.view, Y0.view), f"{what}: NaN padding and zero padding give different results"
        if with_bias:
            within(Y.view.cpu(), ref + bias.double(), tol + U * bias.double().abs(), what + " + bias")
        else:
            within(Y.view.cpu(), ref, tol, what)


def test_aggregate_refusals(hip, graphs):
    """A GAT graph (no weights), ldh < F and ldy < F: GCL_EINVAL, a message, y untouched."""
    n, ei = graphs["mesh12"]
    L = hip.lib()
    hd = rnd(B, n, 64, seed=1).to(DEV)
    H_ = Rows.of(hd, "pad_nan", NAN)
    for G, ldh, ldy in ((hip.Graph(ei, n, hip.GRAPH_GAT), H_.ld, None), (hip.Graph(ei, n, hip.GRAPH_GCN), 60, None),
                        (hip.Graph(ei, n, hip.GRAPH_GCN), H_.ld, 60)):
        Y = Rows(n, 64, "pad_nan", SENT, "out", B=B)
        rc = L.gcl_aggregate(G.handle, 0, H_.ptr, ldh, H_.bs, None, Y.ptr, ldy or Y.ld, Y.bs, B, 64, hip._stream())
        assert rc == EINVAL and L.gcl_last_error()
        torch.cuda.synchronize()
        assert bool((Y.buf == SENT).all())


# ------------------------------------------------------------------------------------------------------------------
# gcl_gcn_layer_fwd / gcl_gcn_layer_fwd_rows
# ------------------------------------------------------------------------------------------------------------------
def act64(x, act, a):
    return x if act == 0 else torch.where(x > 0, x, a * x) if act == 1 else x * torch.sigmoid(x)


GCN_CASES = [  # graph, kind, Fin, Fout, Fout_store, layout of x, layout of y, act
    ("mesh12", "gcn", 64, 64, 64, "pad_nan", "pad_nan", 1), ("mesh12", "gcn", 48, 33, 36, "colblock", "tight", 0),
    ("mesh12", "gcn", 64, 19, 20, "tight", "colblock", 2), ("mesh12", "gcn", 12, 33, 36, "pad_nan", "pad_nan", 1),
    ("mesh23_tiled", "gcn", 64, 64, 64, "pad_nan", "colblock", 1), ("mesh23_tiled", "gcn", 64, 33, 36, "colblock", "tight", 2),
    ("mesh23_tiled", "gcn", 48, 19, 20, "tight", "pad_nan", 0),
    ("degree64", "gcn", 64, 33, 36, "pad_nan", "tight", 1), ("degree64", "gcn", 16, 64, 64, "colblock", "colblock", 2),
    ("degree64", "mean", 64, 33, 36, "tight", "pad_nan", 0), ("degree64", "mean", 32, 19, 20, "colblock", "tight", 0),
]


@pytest.mark.parametrize("gname,kind,Fin,Fout,Fs,lx,ly,act", GCN_CASES)
def test_gcn_layer_layouts(hip, graphs, monkeypatch, gname, kind, Fin, Fout, Fs, lx, ly, act):
    """The one-kernel GCNConv layer, all rows and only the first rows_out: |y - ref| <= (deg + Fin + 3) U
    sum_e |w_e| sum_k |act(x_ek) W_ok| + U |bias|; columns [Fout, Fout_store) are exact zeros, columns past Fout_store,
    rows past rows_out and the batch gap are untouched."""
    n, ei = graphs[gname]
    k = hip.GRAPH_MEAN if kind == "mean" else hip.GRAPH_GCN
    G = hip.Graph(ei, n, k)
    e2, w = edges_of(k, n, ei, hip)
    deg = torch.bincount(e2[1], minlength=n).double()
    x, W, bias = rnd(B, n, Fin, seed=Fin + Fout), rnd(Fout, Fin, seed=2, scale=0.3), rnd(Fout, seed=3)
    ax = act64(x.double(), act, 0.25)
    ref = P._propagate_sum(ax @ W.double().t(), e2, w, n) + bias.double()
    tol = (deg[None, :, None] + Fin + 3) * U * P._propagate_sum(ax.abs() @ W.double().abs().t(), e2, w.abs(), n) \
        + U * bias.double().abs()
    L = hip.lib()
    xd, Wd, bd, a = x.to(DEV), W.to(DEV), bias.to(DEV), torch.tensor([0.25], device=DEV)
    what = f"gcn_layer {gname} {kind} {Fin}->{Fout}/{Fs} x:{lx} y:{ly} act={act}"
    staged_any = False

    def run(fill, rows_out):
        X, Y = Rows.of(xd, lx, fill), Rows(n, Fs, ly, SENT, "out", B=B)
        sl = a.data_ptr() if act == 1 else None
        if rows_out is None:
            rc = L.gcl_gcn_layer_fwd(G.handle, X.ptr, X.ld, X.bs, act, sl, Wd.data_ptr(), bd.data_ptr(), Y.ptr, Y.ld, Y.bs,
                                     B, Fin, Fout, Fs, hip._stream())
        else:
            rc = L.gcl_gcn_layer_fwd_rows(G.handle, X.ptr, X.ld, X.bs, act, sl, Wd.data_ptr(), bd.data_ptr(), Y.ptr, Y.ld,
                                          Y.bs, B, Fin, Fout, Fs, rows_out, hip._stream())
        return rc, Y

    for rows_out in (None, 1, 70, n - 1, "tiles off"):
        tiles_off = rows_out == "tiles off"
        if tiles_off:  # where the source-tile layer ran, the per-edge kernel on the same rows: GCL_GCN_HALO=0
            if not staged_any:
                break
            monkeypatch.setenv("GCL_GCN_HALO", "0")
            rows_out = None
        (rc, Y), names = launched(lambda: run(NAN, rows_out))
        hip._check(rc)
        # the source-tile form takes whole layers (rows_out = n) of 48 or 64 inputs on a GCN graph with a tile layout
        # (and has further gates about speed); the tile-ordered mesh is there to make it run
        may_stage = (rows_out is None and not tiles_off and Fin in (48, 64) and kind == "gcn"
                     and G.halo_info(False, 64) is not None)
        staged = has(names, "gcn_halo_fwd_kernel")
        staged_any = staged_any or staged
        assert staged != has(names, "gcn_fwd_kernel") and (may_stage or not staged), f"{what}: {names}"
        if gname == "mesh23_tiled" and rows_out is None and Fin in (48, 64) and not tiles_off:
            assert staged, f"{what}: the source-tile layer did not run: {names}"
        kern = "gcn_halo_fwd_kernel" if staged else "gcn_fwd_kernel"
        if rows_out in (None, 70):
            print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [{what} rows_out={rows_out}]")
        r = n if rows_out is None else rows_out
        if r < n:  # rows past rows_out stay as they were
            torch.as_strided(Y.inside, (B, n - r, Fs), (Y.bs, Y.ld, 1), Y.view.storage_offset() + r * Y.ld).fill_(False)
        assert Y.untouched(SENT), f"{what} rows_out={rows_out}: wrote outside y[:, :rows_out, :Fout_store]"
        rc0, Y0 = run(0.0, rows_out)
        hip._check(rc0)
        got = Y.view[:, :r]
        assert same_bits(got, Y0.view[:, :r]), f"{what}: NaN padding and zero padding give different results"
        assert bool((got[:, :, Fout:] == 0).all()), f"{what}: columns [Fout, Fout_store) are not exact zeros"
        within(got[:, :, :Fout].cpu(), ref[:, :r], tol[:, :r], f"{what} rows_out={rows_out}")


@pytest.mark.parametrize("case", ["odd_ld x", "offset x", "odd_ld y", "offset y", "heavy rows", "Fin % 4", "Fout_store % 4",
                                  "ldy < Fout_store"])
def test_gcn_layer_refusals(hip, graphs, case):
    n, ei = graphs["heavy_ring" if case == "heavy rows" else "mesh12"]
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    Fin, Fout, Fs = (18 if case == "Fin % 4" else 16), 33, (34 if case == "Fout_store % 4" else 36)
    lx = case.split()[0] if case.endswith(" x") else "pad_nan"
    ly = case.split()[0] if case.endswith(" y") else "pad_nan"
    X = Rows.of(rnd(B, n, Fin, seed=1).to(DEV), lx, NAN)
    Y = Rows(n, 33 if case == "ldy < Fout_store" else 36, "tight" if case == "ldy < Fout_store" else ly, SENT, "out", B=B)
    Wd, bd = rnd(Fout, Fin, seed=2).to(DEV), rnd(Fout, seed=3).to(DEV)
    L = hip.lib()
    rc = L.gcl_gcn_layer_fwd(G.handle, X.ptr, X.ld, X.bs, 0, None, Wd.data_ptr(), bd.data_ptr(), Y.ptr,
                             32 if case == "ldy < Fout_store" else Y.ld, Y.bs, B, Fin, Fout, Fs, hip._stream())
    assert rc == EINVAL and L.gcl_last_error(), case
    torch.cuda.synchronize()
    assert bool((Y.buf == SENT).all()), f"{case}: a refused call wrote to y"


# ------------------------------------------------------------------------------------------------------------------
# gcl_gat_fwd / gcl_gat_bwd
# ------------------------------------------------------------------------------------------------------------------
TOL = 1e-5


def rel(a, b):
    """max(Frobenius relative error, element-wise max|diff| / max|ref|), as in test_hip_ops."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    fro = ((a - b).norm() / (b.norm() + 1e-30)).item()
    mx = ((a - b).abs().max() / (b.abs().max() + 1e-30)).item() if b.numel() else 0.0
    return max(fro, mx)


class Gat:
    """One GAT problem on `graph`: h is the layer's own input (the oracle runs with an identity weight in float64, so
    its x.grad is dh) and the library calls on the layouts of the issue: h and dh inside wider rows with a batch gap, y on
    rows wider than C, dy on padded rows that are contiguous across the batch (what gcl_gat_bwd asks for)."""

    def __init__(self, hip, n, ei, H, C, att_scale=0.3, seed=0):
        self.hip, self.n, self.H, self.C = hip, n, H, C
        self.G = hip.Graph(ei, n, hip.GRAPH_GAT)
        self.h = rnd(B, n, H * C, seed=seed + 1)
        self.a_s, self.a_d = rnd(H * C, seed=seed + 3, scale=att_scale), rnd(H * C, seed=seed + 4, scale=att_scale)
        self.b, self.dy = rnd(C, seed=seed + 5), rnd(B, n, C, seed=seed + 6)
        x = self.h.double().requires_grad_()
        as64, ad64 = self.a_s.double().view(1, H, C).requires_grad_(), self.a_d.double().view(1, H, C).requires_grad_()
        b64 = self.b.double().requires_grad_()
        y, self.ei2, alpha = P.gat_conv(x, ei, torch.eye(H * C, dtype=torch.float64), as64, ad64, b64, H)
        y.backward(self.dy.double())
        self.y, self.alpha = y.detach(), alpha.detach()
        self.dh, self.d_as, self.d_ad, self.d_b = x.grad, as64.grad.reshape(-1), ad64.grad.reshape(-1), b64.grad
        assert torch.equal(self.G.export_edges(), self.ei2)
        self.dev = [t.to(DEV) for t in (self.h, self.a_s, self.a_d, self.b, self.dy)]

    def fwd(self, lh, ly, fill, with_alpha=True):
        hip, L, n, H, C = self.hip, self.hip.lib(), self.n, self.H, self.C
        hd, asd, add_, bd, _ = self.dev
        Hh, Y = Rows.of(hd, lh, fill), Rows(n, C, ly, SENT, "out", B=B)
        s_src, s_dst = torch.full((B, n, H), SENT, device=DEV), torch.full((B, n, H), SENT, device=DEV)
        alpha = torch.full((B, self.G.e, H), SENT, device=DEV)
        rc = L.gcl_gat_fwd(self.G.handle, Hh.ptr, Hh.ld, Hh.bs, asd.data_ptr(), add_.data_ptr(), bd.data_ptr(),
                           s_src.data_ptr(), s_dst.data_ptr(), alpha.data_ptr() if with_alpha else None, Y.ptr, Y.ld, Y.bs,
                           B, H, C, hip._stream())
        return rc, Hh, Y, s_src, s_dst, alpha

    def bwd(self, lh, ldh_, fill, saved, acc=0, pre=SENT):
        hip, L, n, H, C = self.hip, self.hip.lib(), self.n, self.H, self.C
        hd, asd, add_, _, dyd = self.dev
        s_src, s_dst, alpha = saved
        Hh, DH = Rows.of(hd, lh, fill), Rows(n, H * C, ldh_, SENT, "out", B=B)
        DY = Rows.of(dyd.reshape(B * n, C), "pad_nan", fill)  # [B * n, C] on rows of C + 4: bsdy = n * lddy
        d_as, d_ad = torch.full((H * C,), pre, device=DEV), torch.full((H * C,), pre, device=DEV)
        d_b = torch.full((C,), pre, device=DEV)
        ws = hip.workspace(L.gcl_gat_bwd_ws_bytes(self.G.e, n, B, H, C), DEV)
        rc = L.gcl_gat_bwd(self.G.handle, DY.ptr, DY.ld, n * DY.ld, Hh.ptr, Hh.ld, Hh.bs, asd.data_ptr(), add_.data_ptr(),
                           s_src.data_ptr(), s_dst.data_ptr(), alpha.data_ptr(), DH.ptr, DH.ld, DH.bs, d_as.data_ptr(),
                           d_ad.data_ptr(), d_b.data_ptr(), acc, B, H, C, ws.data_ptr(), ws.numel(), hip._stream())
        return rc, DH, d_as, d_ad, d_b


GAT_CASES = [(g, H, C, lh, False) for g in ("mesh12", "degree") for H, C in ((1, 64), (4, 64), (3, 48), (1, 12))
             for lh in ("colblock", "pad_nan")] + [
    ("mesh23_tiled", 1, 64, "colblock", False), ("mesh23_tiled", 1, 64, "pad_nan", False), ("heavy_ring", 1, 64, "colblock", False),
    ("heavy_ring", 4, 64, "pad_nan", False),
    # GCL_GAT_HALO=0: the per-edge kernels where the source-tile ones run by default
    ("mesh12", 1, 64, "colblock", True), ("mesh23_tiled", 1, 64, "pad_nan", True)]


@pytest.mark.parametrize("gname,H,C,lh,tiles_off", GAT_CASES)
def test_gat_layouts(hip, graphs, monkeypatch, gname, H, C, lh, tiles_off):
    """gcl_gat_fwd / gcl_gat_bwd at test_gat_fwd_bwd's bars (1e-5 forward, 5e-5 gradients, the rows of an edge whose
    score lies within 2e-6 of LeakyReLU's kink left out of the element-wise dh check) against the float64 oracle, with
    alpha = NULL, accumulate 0 and 1, and every array outside the views untouched."""
    n, ei = graphs[gname]
    if tiles_off:
        monkeypatch.setenv("GCL_GAT_HALO", "0")
    p = Gat(hip, n, ei, H, C, seed=H * C)
    what = f"gat {gname} H={H} C={C} h:{lh}{' GCL_GAT_HALO=0' if tiles_off else ''}"
    ly, ldh_ = ("pad_nan", "colblock") if lh == "colblock" else ("colblock", "pad_nan")
    (rc, Hh, Y, s_src, s_dst, alpha), names = launched(lambda: p.fwd(lh, ly, NAN))
    hip._check(rc)
    # one head of 64 (or 128) on a graph with a tile layout and no heavy row runs the source-tile kernels; the
    # tile-ordered mesh is there to make them run
    may_stage = (not tiles_off and H == 1 and C in (64, 128) and p.G.halo_info(False, 64) is not None
                 and p.G.max_in_degree <= 64)
    tiled = has(names, "gat_halo_fwd_kernel")
    assert tiled != has(names, "gat_fwd_kernel") and (may_stage or not tiled), f"{what}: {names}"
    if gname == "mesh23_tiled" and not tiles_off:
        assert tiled, f"{what}: the source-tile kernel did not run: {names}"
    kern = "gat_halo_fwd_kernel" if tiled else "gat_fwd_kernel"
    print(f"ran: {kern}<{', '.join(targs(names, kern)[0])}>  [{what}]")
    assert Hh.ld > H * C and Y.ld > C
    assert Y.untouched(SENT), f"{what}: wrote outside y[:, :, :C]"
    assert not bool((alpha == SENT).any()) and not bool((s_src == SENT).any()) and not bool((s_dst == SENT).any())
    rc0, _, Y0, s0, d0, al0 = p.fwd(lh, ly, 0.0)
    hip._check(rc0)
    for a_, b_, name in ((Y.view, Y0.view, "y"), (alpha, al0, "alpha"), (s_src, s0, "a_src"), (s_dst, d0, "a_dst")):
        assert same_bits(a_, b_), f"{what}: {name} differs between NaN padding and zero padding"
    rcn, _, Yn, _, _, aln = p.fwd(lh, ly, NAN, with_alpha=False)
    hip._check(rcn)
    assert same_bits(Yn.view, Y.view) and bool((aln == SENT).all()), f"{what}: alpha = NULL changes y or writes alpha"
    assert rel(Y.view, p.y) < TOL, f"{what}: y {rel(Y.view, p.y):.3e}"
    al_e = torch.stack([hip.gat_alpha_edge_order(p.G, alpha[i], H) for i in range(B)])
    assert rel(al_e, p.alpha) < TOL, f"{what}: alpha {rel(al_e, p.alpha):.3e}"

    saved = (s_src, s_dst, alpha)
    (rc, DH, d_as, d_ad, d_b), names = launched(lambda: p.bwd(lh, ldh_, NAN, saved))
    hip._check(rc)
    staged_bwd = has(names, "gat_halo_bwd_dst_kernel")  # needs tile layouts in both directions, on top of the forward's gates
    assert staged_bwd == has(names, "gat_halo_bwd_src_kernel") and staged_bwd != has(names, "gat_bwd_dst_kernel"), f"{what}: {names}"
    assert tiled or not staged_bwd, f"{what}: {names}"
    print(f"ran: {'gat_halo_bwd_dst_kernel + gat_halo_bwd_src_kernel' if staged_bwd else 'gat_bwd_dst_kernel + gat_bwd_src_kernel'}"
          f"  [{what}]")
    assert DH.ld > H * C and DH.untouched(SENT), f"{what}: wrote outside dh[:, :, :H * C]"
    rc0, DH0, das0, dad0, db0 = p.bwd(lh, ldh_, 0.0, saved)
    hip._check(rc0)
    for a_, b_, name in ((DH.view, DH0.view, "dh"), (d_as, das0, "d_att_src"), (d_ad, dad0, "d_att_dst"), (d_b, db0, "d_bias")):
        assert same_bits(a_, b_), f"{what}: {name} differs between NaN padding and zero padding"
    h64 = p.h.double().reshape(B, n, H, C)
    e = ((h64 * p.a_s.double().view(H, C)).sum(-1)[:, p.ei2[0]] + (h64 * p.a_d.double().view(H, C)).sum(-1)[:, p.ei2[1]]).abs()
    near = (e < 2e-6).any(dim=2).any(dim=0)
    keep = torch.ones(n, dtype=torch.bool)
    keep[p.ei2[0][near]] = False
    keep[p.ei2[1][near]] = False
    assert int((~keep).sum()) <= max(8, n // 200)
    dh = DH.view.cpu().double()
    assert rel(dh[:, keep], p.dh[:, keep]) < 5e-5, f"{what}: dh {rel(dh[:, keep], p.dh[:, keep]):.3e}"
    assert float((dh - p.dh).norm() / p.dh.norm()) < 5e-5
    assert rel(d_as, p.d_as) < 5e-5 and rel(d_ad, p.d_ad) < 5e-5 and rel(d_b, p.d_b) < TOL, what
    # accumulate = 1 adds into what the destinations hold (3.0), one fp32 addition each
    rc, DH1, a1, a2, b1 = p.bwd(lh, ldh_, NAN, saved, acc=1, pre=3.0)
    hip._check(rc)
    assert same_bits(DH1.view, DH.view)
    for t, first, name in ((a1, d_as, "d_att_src"), (a2, d_ad, "d_att_dst"), (b1, d_b, "d_bias")):
        within(t, first.double() + 3.0, U * (first.double().abs() + 3.0), f"{what}: {name} with accumulate")


@pytest.mark.parametrize("case", ["odd_ld h", "offset h", "offset y", "odd_ld dh", "C % 4", "GCN graph"])
def test_gat_refusals(hip, graphs, case):
    n, ei = graphs["mesh12"]
    H, C = 1, (14 if case == "C % 4" else 16)
    G = hip.Graph(ei, n, hip.GRAPH_GCN if case == "GCN graph" else hip.GRAPH_GAT)
    L = hip.lib()
    lay_of = lambda who: case.split()[0] if case.endswith(" " + who) else "pad_nan"  # noqa: E731
    Hh = Rows.of(rnd(B, n, H * C, seed=1).to(DEV), lay_of("h"), NAN)
    Y, DH = Rows(n, C, lay_of("y"), SENT, "out", B=B), Rows(n, H * C, lay_of("dh"), SENT, "out", B=B)
    att, bias = rnd(H * C, seed=2).to(DEV), rnd(C, seed=3).to(DEV)
    s_src, s_dst = torch.zeros(B, n, H, device=DEV), torch.zeros(B, n, H, device=DEV)
    alpha = torch.full((B, G.e, H), 0.5, device=DEV)
    if case != "odd_ld dh":
        rc = L.gcl_gat_fwd(G.handle, Hh.ptr, Hh.ld, Hh.bs, att.data_ptr(), att.data_ptr(), bias.data_ptr(), s_src.data_ptr(),
                           s_dst.data_ptr(), alpha.data_ptr(), Y.ptr, Y.ld, Y.bs, B, H, C, hip._stream())
        assert rc == EINVAL and L.gcl_last_error(), case
    if not case.endswith(" y"):
        DY = Rows.of(rnd(B * n, C, seed=4).to(DEV), "pad_nan", NAN)
        ws = hip.workspace(L.gcl_gat_bwd_ws_bytes(G.e, n, B, H, C), DEV)
        d1, d2, d3 = torch.full((H * C,), SENT, device=DEV), torch.full((H * C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)
        rc = L.gcl_gat_bwd(G.handle, DY.ptr, DY.ld, n * DY.ld, Hh.ptr, Hh.ld, Hh.bs, att.data_ptr(), att.data_ptr(),
                           s_src.data_ptr(), s_dst.data_ptr(), alpha.data_ptr(), DH.ptr, DH.ld, DH.bs, d1.data_ptr(),
                           d2.data_ptr(), d3.data_ptr(), 0, B, H, C, ws.data_ptr(), ws.numel(), hip._stream())
        assert rc == EINVAL and L.gcl_last_error(), case
        assert bool((d1 == SENT).all()) and bool((d3 == SENT).all())
    torch.cuda.synchronize()
    assert bool((Y.buf == SENT).all()) and bool((DH.buf == SENT).all()), f"{case}: a refused call wrote to its output"


# torch's own fp32 segment softmax against float64 on the inputs of the test below (the degree-edge graph, H = 2, C = 16,
# scores scaled to max |e| = 60): max over the edges of (|alpha32 - alpha64| - U) / (U (1 + max_row |e|) alpha64),
# measured with torch 2.10 on a CPU: 1.11.  The kernel's expf and reciprocal are not torch's: 4 x that is allowed.
SOFTMAX_C_TORCH = 1.11
SOFTMAX_C = 4 * SOFTMAX_C_TORCH


def softmax_case(n, ei):
    H, C = 2, 16
    h = rnd(B, n, H * C, seed=77)
    a_s, a_d = rnd(H * C, seed=78), rnd(H * C, seed=79)
    e2 = P.add_self_loops(P.remove_self_loops(ei), n)
    h4 = h.double().view(B, n, H, C)
    raw = (h4 * a_s.double().view(H, C)).sum(-1)[:, e2[0]] + (h4 * a_d.double().view(H, C)).sum(-1)[:, e2[1]]
    s = 60.0 / float(torch.nn.functional.leaky_relu(raw, 0.2).abs().max())
    return H, C, h, (a_s.double() * s).float(), (a_d.double() * s).float(), e2


def softmax_ref(a_src32, a_dst32, e2, n):
    """float64 softmax of the scores formed from the fp32 per-node terms (the kernel's own a_src / a_dst outputs)."""
    e = torch.nn.functional.leaky_relu(a_src32.double()[:, e2[0]] + a_dst32.double()[:, e2[1]], 0.2)
    emax = torch.zeros(e.shape[0], n, e.shape[2], dtype=torch.float64).scatter_reduce(
        1, e2[1].view(1, -1, 1).expand_as(e), e.abs(), reduce="amax", include_self=True)
    return P.segment_softmax(e, e2[1], n), emax[:, e2[1]]


def test_gat_softmax_range(hip, graphs):
    """Scores up to +-60 on the degree-edge graph (rows of 1, 2, .., 66 in-edges, the `deg > EL` loop beside the register
    path): a_src / a_dst within the dot-product bound; alpha against a float64 softmax of those scores within
    c U (1 + max|e|) alpha + U (the conditioning of exp), c = SOFTMAX_C; every row's alpha finite and summing to 1 within
    deg U; y within what those alpha errors and an fp32 sum of deg terms allow."""
    n, ei = graphs["degree"]
    H, C, h, a_s, a_d, e2 = softmax_case(n, ei)
    G = hip.Graph(ei, n, hip.GRAPH_GAT)
    assert torch.equal(G.export_edges(), e2)
    bias = rnd(C, seed=80)
    L = hip.lib()
    Hh, Y = Rows.of(h.to(DEV), "colblock", NAN), Rows(n, C, "pad_nan", SENT, "out", B=B)
    s_src, s_dst = torch.full((B, n, H), SENT, device=DEV), torch.full((B, n, H), SENT, device=DEV)
    alpha = torch.full((B, G.e, H), SENT, device=DEV)
    asd, add_, bd = a_s.to(DEV), a_d.to(DEV), bias.to(DEV)
    hip._check(L.gcl_gat_fwd(G.handle, Hh.ptr, Hh.ld, Hh.bs, asd.data_ptr(), add_.data_ptr(), bd.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(), alpha.data_ptr(), Y.ptr, Y.ld, Y.bs,
                             B, H, C, hip._stream()))
    assert Y.untouched(SENT)
    h4 = h.double().view(B, n, H, C)
    for got, att, name in ((s_src, a_s, "a_src"), (s_dst, a_d, "a_dst")):
        t = h4 * att.double().view(H, C)
        within(got.cpu(), t.sum(-1), (C + 3) * U * t.abs().sum(-1), name)
    al = torch.stack([hip.gat_alpha_edge_order(G, alpha[i], H) for i in range(B)]).cpu()  # PyG edge order
    assert bool(torch.isfinite(al).all())
    ref, emax = softmax_ref(s_src.cpu(), s_dst.cpu(), e2, n)
    assert float(emax.max()) > 55.0
    # torch's fp32 softmax on the same scores, for the record (printed; the bound uses the constant above)
    e32 = torch.nn.functional.leaky_relu(s_src.cpu()[:, e2[0]] + s_dst.cpu()[:, e2[1]], 0.2)
    c_torch = float(((P.segment_softmax(e32, e2[1], n).double() - ref).abs() - U).clamp(min=0).div(U * (1 + emax) * ref + 1e-300).max())
    c_kernel = float(((al.double() - ref).abs() - U).clamp(min=0).div(U * (1 + emax) * ref + 1e-300).max())
    print(f"softmax constant: torch fp32 {c_torch:.3f}, kernel {c_kernel:.3f}, allowed {SOFTMAX_C:.3f}")
    tol_al = SOFTMAX_C * U * (1 + emax) * ref + U
    within(al, ref, tol_al, "alpha vs float64 softmax")
    deg = torch.bincount(e2[1], minlength=n).double()
    sums = torch.zeros(B, n, H, dtype=torch.float64).index_add_(1, e2[1], al.double())
    within(sums, torch.ones_like(sums), (deg * U)[None, :, None].expand_as(sums), "sum of a row's alpha")
    hj = h4[:, e2[0]]  # [B, E', H, C]
    y64 = torch.zeros(B, n, H, C, dtype=torch.float64).index_add_(1, e2[1], ref.unsqueeze(-1) * hj).mean(2) + bias.double()
    spread = torch.zeros(B, n, H, C, dtype=torch.float64).index_add_(1, e2[1], tol_al.unsqueeze(-1) * hj.abs())
    mass = torch.zeros(B, n, H, C, dtype=torch.float64).index_add_(1, e2[1], ref.unsqueeze(-1) * hj.abs())
    tol_y = (spread + (deg[None, :, None, None] + 3) * U * mass).mean(2) + U * (H * mass.mean(2) + bias.double().abs())
    within(Y.view.cpu(), y64, tol_y, "y vs float64")


# ------------------------------------------------------------------------------------------------------------------
# gcl_segment_reduce / gcl_edge_combine
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [12, 64, 132])
@pytest.mark.parametrize("mean", [0, 1])
@pytest.mark.parametrize("ls,lo", [("pad_nan", "colblock"), ("colblock", "pad_nan"), ("tight", "tight")])
def test_segment_reduce_layouts(hip, graphs, D, mean, ls, lo):
    """Segment sum / mean over the receiver-sorted edges of the degree-edge graph (empty segments included), src through
    a permutation, src and out strided with a batch gap: |out - ref| <= (deg + 3) U sum |terms| (+ U |ref| for the
    division of the mean)."""
    n, ei = graphs["degree"]
    E = ei.shape[1]
    order = torch.argsort(ei[1], stable=True)
    deg = torch.bincount(ei[1], minlength=n)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    src = rnd(B, E, D, seed=D)
    seg = ei[1][order]
    ref = torch.zeros(B, n, D, dtype=torch.float64).index_add_(1, seg, src.double()[:, order])
    mass = torch.zeros(B, n, D, dtype=torch.float64).index_add_(1, seg, src.double()[:, order].abs())
    tol = (deg.double()[None, :, None] + 3) * U * mass
    if mean:
        ref = ref / deg.double().clamp(min=1)[None, :, None]
        tol = tol / deg.double().clamp(min=1)[None, :, None] + U * ref.abs()
    L = hip.lib()
    perm_d, rp_d = order.to(torch.int32).to(DEV), rowptr.to(DEV)

    def run(fill):
        S, O = Rows.of(src.to(DEV), ls, fill), Rows(n, D, lo, SENT, "out", B=B)
        return L.gcl_segment_reduce(S.ptr, S.ld, S.bs, perm_d.data_ptr(), rp_d.data_ptr(), mean, O.ptr, O.ld, O.bs, B, n, D,
                                    hip._stream()), O

    rc, O = run(NAN)
    hip._check(rc)
    assert O.untouched(SENT)
    rc0, O0 = run(0.0)
    hip._check(rc0)
    assert same_bits(O.view, O0.view)
    assert bool((O.view[:, (deg == 0).to(DEV)] == 0).all()), "an empty segment is not exactly zero"
    within(O.view.cpu(), ref, tol, f"segment_reduce D={D} mean={mean} {ls}->{lo}")


@pytest.mark.parametrize("D", [12, 64])
@pytest.mark.parametrize("la,lc", [("pad_nan", "colblock"), ("colblock", "tight")])
def test_edge_combine_layouts(hip, graphs, D, la, lc):
    """out[b, e] = base + extra + A[b, ia[e]] * sa[ia[e]] + C[b, ic[e]] with A and C strided (NaN beside them and in
    the batch gap): each element is a sum of four terms, held to 4 U sum |terms|; every subset of operands."""
    n, ei = graphs["degree"]
    E = ei.shape[1]
    base, extra, A, Cm, sa = rnd(B, E, D, seed=1), rnd(B, E, D, seed=2), rnd(B, n, D, seed=3), rnd(B, n, D, seed=4), rnd(n, seed=5)
    ia, ic = ei[0].to(torch.int32).to(DEV), ei[1].to(torch.int32).to(DEV)
    L = hip.lib()
    bd, ed, sad = base.to(DEV), extra.to(DEV), sa.to(DEV)
    for use in ((1, 1, 1, 1), (0, 0, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1), (0, 0, 1, 0)):
        terms = [t for t, u in zip((base.double(), extra.double(), A.double()[:, ei[0]] * sa.double()[ei[0]][None, :, None],
                                    Cm.double()[:, ei[1]]), use) if u]
        ref, mass = sum(terms), sum(t.abs() for t in terms)

        def run(fill):
            Ar, Cr = Rows.of(A.to(DEV), la, fill), Rows.of(Cm.to(DEV), lc, fill)
            out = torch.full((B, E, D), SENT, device=DEV)
            rc = L.gcl_edge_combine(bd.data_ptr() if use[0] else None, ed.data_ptr() if use[1] else None,
                                    Ar.ptr if use[2] else None, Ar.ld, Ar.bs, ia.data_ptr() if use[2] else None,
                                    sad.data_ptr() if use[2] else None, Cr.ptr if use[3] else None, Cr.ld, Cr.bs,
                                    ic.data_ptr() if use[3] else None, out.data_ptr(), B, E, D, hip._stream())
            return rc, out

        rc, out = run(NAN)
        hip._check(rc)
        rc0, out0 = run(0.0)
        hip._check(rc0)
        assert same_bits(out, out0)
        within(out.cpu(), ref, 4 * U * mass, f"edge_combine D={D} operands={use}")
