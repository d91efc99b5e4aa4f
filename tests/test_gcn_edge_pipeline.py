"""The per-edge one-kernel GCNConv layer (gcn_fwd_kernel) on graphs with one to two edges per row.

Two things changed in the split-operand form and neither changes a bit of the result: the dense part's matrix chain is
straight-line code per K-step count (one branch on K / 16 in front of it instead of one around every step), and a wave
with few items starts without the stagger sleep.  GCL_GCN_EDGE_PIPE=0 (read per call) restores the stagger for every
wave; the chain has no switch, so it is held against the float64 evaluation: on small-integer data with power-of-two
edge weights every sum, piece product and partial sum is exact and the layer must equal float64 bit for bit, in each
prefix-width instantiation and for 1, 2, 3 and 4 K-steps.  Every other case compares the default with the switch off by
torch.equal.  Outputs are views inside NaN-filled tensors: nothing outside a view may be written.

A launch has one item per wave until B * tiles exceeds 2048 (256 blocks of 8 waves): the small batches cover waves with
one item or none, the large ones waves with two to four items whose tiles differ in width (a wave's next tile is
gathered at its own width, rows past the prefix go through the fix-up loop).  The pipelined item loop these cases were
first written for (next item's rows loaded under the dense part) did not pay and is not in the kernel: DESIGN.md 3.2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N = 203  # six whole 32-row tiles and a ragged one of 11 rows


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ("GCL_GCN_EDGE_PIPE", "GCL_X3", "GCL_X3_GCN", "GCL_GCN_HALO"):
        monkeypatch.delenv(k, raising=False)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bip_edges(n, head, m, seed):
    """Random bipartite-plus-self-loops edges (tests/test_encoder_output_split.py): between the first `head` rows and the
    others, both directions."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, head, m)
    b = rng.integers(head, n, m)
    k = m * 4 // 7
    return torch.unique(torch.from_numpy(np.concatenate([np.stack([a, b]), np.stack([b[:k], a[:k]])], 1)), dim=1)


def tile_edges(widths, fat, n, seed=3):
    """Edges of a graph whose 32-row tile t has `fat[t]` rows (at changing places) with widths[t] in-edges, self-loop
    included, and self-loop-only rows otherwise.  Senders are distinct rows anywhere in the graph."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for t, (d, k) in enumerate(zip(widths, fat)):
        rows = [r for r in (t * 32 + (5 * t + 7 * j) % 32 for j in range(k)) if r < n]
        for r in rows if d > 1 else []:
            s = rng.choice(n - 1, d - 1, replace=False)
            s = s + (s >= r)  # never the row itself: the self-loop is added by the graph
            src += s.tolist()
            dst += [r] * (d - 1)
    return torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)


def cover(ei, n):
    """The prefix width the layer is instantiated with (graph.hip: smallest of 2, 4 that leaves <= 2 % of the rows to the
    fix-up loop, else 8); in-degrees count the self-loop."""
    deg = np.bincount(ei[1].numpy(), minlength=n) + 1
    for cand in (2, 4):
        if (deg > cand).sum() * 50 <= n:
            return cand
    return 8


# tile widths in an order where narrow follows wide and the reverse; 17 tiles (the last ragged: 523 rows) are coprime to
# the 256 waves of an XCD group, so a wave's successive items are tiles rt, rt + 1, ... of different samples
WIDTHS = [1, 20, 2, 9, 1, 3, 8, 2, 4, 1, 5, 1, 1, 2, 1, 2, 1]
NW = 16 * 32 + 11
FAT = {2: [1] * 17,                                              # one wide row per tile: 6 rows above 2 of 523
       4: [8 if d in (3, 4) else 1 for d in WIDTHS],             # 16 rows above 2, 4 above 4
       8: [6 if d >= 5 else 1 for d in WIDTHS]}                  # 24 rows above 4
# the same with widths 1 | 4 | 16 only: every edge weight 1 / sqrt(d_i d_j) is a power of two
EXACT_W = [1, 16, 4, 1, 1, 4, 16, 1, 4, 1, 16, 1, 1, 4, 1, 1, 1]
EXACT_FAT = {2: [1] * 17, 4: [8 if d == 4 else 1 for d in EXACT_W], 8: [6 if d == 16 else 1 for d in EXACT_W]}


@pytest.fixture(scope="module")
def graphs(hip):
    """Every graph of this file, built once."""
    gs = {"bip": hip.Graph(bip_edges(N, 64, 700, 7), N, hip.GRAPH_GCN),
          "bip_mean": hip.Graph(bip_edges(N, 64, 700, 7), N, hip.GRAPH_MEAN),
          "big": hip.Graph(bip_edges(3001, 1024, 9000, 8), 3001, hip.GRAPH_GCN),
          "loops": hip.Graph(torch.arange(NW).repeat(2, 1), NW, hip.GRAPH_GCN)}
    for ew in (2, 4, 8):
        for tag, ws, fat in (("w", WIDTHS, FAT), ("x", EXACT_W, EXACT_FAT)):
            ei = tile_edges(ws, fat[ew], NW)
            assert cover(ei, NW) == ew, (tag, ew, cover(ei, NW))
            deg = np.bincount(ei[1].numpy(), minlength=NW) + 1
            assert [int(deg[t * 32: t * 32 + 32].max()) for t in range(17)] == ws
            gs[f"{tag}{ew}"] = hip.Graph(ei, NW, hip.GRAPH_GCN)
    for g in gs.values():
        assert g.max_in_degree <= 64
    return gs


def only_views_written(big, view):
    mask = torch.zeros_like(big, dtype=torch.bool)
    mask.as_strided(view.shape, view.stride(), view.storage_offset() - big.storage_offset()).fill_(True)
    return bool(torch.isnan(big[~mask]).all())


def run_layer(hip, G, x, act, W, b, rows_out=None, head=None):
    """One launch into views of NaN-filled tensors; returns the written views (clones).  The view is as wide as the stored
    row (Fout rounded up to 4: the padding columns are written, as zeros)."""
    B, n, _ = x.shape
    Fst = (W.shape[0] + 3) // 4 * 4
    sl = torch.tensor([0.25], device=DEV) if act == hip.ACT_PRELU else None
    if head is None:
        rows = rows_out or n
        big = torch.full((B, n + 5, Fst + 8), NAN, device=DEV)
        full = big[:, 2: 2 + n, 4: 4 + Fst]
        hip.gcn_layer_fwd(G, x, act, sl, W, b, out=full, rows_out=rows_out)
        view = full[:, :rows]
        assert only_views_written(big, view)
        return [view.clone()]
    big_a = torch.full((B, head + 5, Fst + 8), NAN, device=DEV)
    big_b = torch.full((B, n - head + 3, Fst), NAN, device=DEV)
    ya, yb = big_a[:, 2: 2 + head, 4: 4 + Fst], big_b[:, 1: 1 + n - head]
    assert hip.gcn_layer_split_ok(G, x, W.shape[0], ya, yb)
    hip.gcn_layer_fwd_split(G, x, act, sl, W, b, ya, yb)
    assert only_views_written(big_a, ya) and only_views_written(big_b, yb)
    return [ya.clone(), yb.clone()]


def both(hip, monkeypatch, *a, **k):
    """(default, GCL_GCN_EDGE_PIPE=0) outputs of one call, asserted torch.equal and finite; returns the default's."""
    monkeypatch.delenv("GCL_GCN_EDGE_PIPE", raising=False)
    new = run_layer(hip, *a, **k)
    monkeypatch.setenv("GCL_GCN_EDGE_PIPE", "0")
    old = run_layer(hip, *a, **k)
    monkeypatch.delenv("GCL_GCN_EDGE_PIPE", raising=False)
    for p, q in zip(new, old):
        assert bool(torch.isfinite(q).all())
        assert torch.equal(p, q), f"{(p != q).sum().item()} elements differ"
    return new


def operands(B, n, Fin, Fout, seed=0):
    return (rnd(B, n, Fin, seed=seed + 1).to(DEV), rnd(Fout, Fin, seed=seed + 2, scale=0.2).to(DEV), rnd(Fout, seed=seed + 3).to(DEV))


ACTS = {"none": "ACT_NONE", "prelu": "ACT_PRELU", "silu": "ACT_SILU"}


@pytest.mark.parametrize("B", [1, 9, 64])
@pytest.mark.parametrize("act", ["none", "prelu"])
def test_items_per_wave_none_or_one(hip, graphs, monkeypatch, B, act):
    """203 rows = 7 tiles.  B = 1: 7 items on 8 waves - one wave has none, no XCD map; B = 9: XCD map, one group holds two
    samples; B = 64.  Every wave has one item at most."""
    x, W, b = operands(B, N, 64, 64, seed=B)
    both(hip, monkeypatch, graphs["bip"], x, getattr(hip, ACTS[act]), W, b)


@pytest.mark.parametrize("Fin,Fout,act", [(64, 64, "prelu"), (64, 48, "none"), (48, 33, "silu")])
def test_three_and_four_items_per_wave(hip, graphs, monkeypatch, Fin, Fout, act):
    """3001 rows (94 tiles, the last with 25 rows), B = 72: 6768 items on 2048 waves - every wave runs three, some four
    (55 MB of input)."""
    x, W, b = operands(72, 3001, Fin, Fout, seed=5)
    both(hip, monkeypatch, graphs["big"], x, getattr(hip, ACTS[act]), W, b)


@pytest.mark.parametrize("ew", [2, 4, 8])
@pytest.mark.parametrize("act", ["none", "prelu", "silu"])
def test_width_classes_and_their_borders(hip, graphs, monkeypatch, ew, act):
    """Tiles whose widest rows have 1, 20, 2, 9, 1, 3, 8, 2, 4, 1, 5, ... in-edges, in graphs that select the 2-, 4- and
    8-wide instantiations; B = 368 gives every wave two or three items, consecutive tiles: every item is gathered at its
    own width, narrow behind wide and the reverse, and rows past the prefix go through the fix-up loop."""
    x, W, b = operands(368, NW, 64, 64, seed=ew)
    both(hip, monkeypatch, graphs[f"w{ew}"], x, getattr(hip, ACTS[act]), W, b)


def test_self_loops_only(hip, graphs, monkeypatch):
    """Every tile is gathered at width 1: y = x W^T + b row by row."""
    x, W, b = operands(368, NW, 64, 48, seed=21)
    (y,) = both(hip, monkeypatch, graphs["loops"], x, hip.ACT_NONE, W, b)
    ref = x.double() @ W.double().t() + b.double()
    assert float((y.double() - ref).abs().max()) < 1e-4 * float(ref.abs().max())  # (exactness: test_exact_on_integers)


@pytest.mark.parametrize("Fin,Fout", [(64, 64), (48, 48), (32, 48), (16, 33), (16, 20), (36, 64), (36, 20)])
@pytest.mark.parametrize("act", ["none", "prelu", "silu"])
def test_shapes(hip, graphs, monkeypatch, Fin, Fout, act):
    """Fin 64 / 48 / 32 / 16: the split-operand form with 4, 3, 2 and 1 K-steps, lanes beyond K clamped into the row;
    Fin 36: the 12-wave fp32-operand form.  Fout 33 is stored in rows of 36, Fout 20 takes the one-column-block
    instantiation."""
    x, W, b = operands(150, NW, Fin, Fout, seed=Fin + Fout)
    both(hip, monkeypatch, graphs["w4"], x, getattr(hip, ACTS[act]), W, b)


@pytest.mark.parametrize("B", [9, 330])
@pytest.mark.parametrize("entry", ["rows64", "rows70", "split64", "mean"])
def test_entry_points(hip, graphs, monkeypatch, entry, B):
    """rows_out = 64 and 70 of 203 (two and three tiles per sample), the two-part store with head 64, and a
    GCL_GRAPH_MEAN graph (the masked variant); B = 330 gives the waves of the rows_out launches more than one item."""
    x, W, b = operands(B, N, 64, 64, seed=31)
    G = graphs["bip_mean" if entry == "mean" else "bip"]
    kw = {"rows64": {"rows_out": 64}, "rows70": {"rows_out": 70}, "split64": {"head": 64}, "mean": {}}[entry]
    both(hip, monkeypatch, G, x, hip.ACT_NONE if entry == "mean" else hip.ACT_PRELU, W, b, **kw)


def test_two_part_store_with_several_items_per_wave(hip, graphs, monkeypatch):
    x, W, b = operands(72, 3001, 64, 64, seed=41)
    both(hip, monkeypatch, graphs["big"], x, hip.ACT_PRELU, W, b, head=1024)


@pytest.mark.parametrize("Fin", [64, 48])
def test_strided_input(hip, graphs, monkeypatch, Fin):
    """x is a view: row stride above Fin, batch stride above n * ld; the rest of the holder is NaN, so a load that
    left the view would show in the output."""
    B = 150
    holder = torch.full((B, NW + 3, Fin + 12), NAN, device=DEV)
    x = holder[:, 1: 1 + NW, 4: 4 + Fin]
    x.copy_(rnd(B, NW, Fin, seed=51).to(DEV))
    assert x.stride(1) > Fin and x.stride(0) > NW * x.stride(1)
    _, W, b = operands(1, 1, Fin, 64, seed=52)
    both(hip, monkeypatch, graphs["w2"], x, hip.ACT_PRELU, W, b)


@pytest.fixture(scope="module")
def exact_data():
    g = torch.Generator().manual_seed(13)
    x = torch.randint(-7, 8, (136, NW, 64), generator=g).float()
    W = torch.randint(-5, 6, (64, 64), generator=g).float()
    W[::3] += 0.5
    b = torch.randint(-9, 10, (64,), generator=g).float()
    return x, W, b


@pytest.mark.parametrize("head", [None, 256])
@pytest.mark.parametrize("Fin", [64, 48, 32, 16])
@pytest.mark.parametrize("ew", [2, 4, 8])
def test_exact_on_integers(hip, graphs, monkeypatch, exact_data, ew, Fin, head):
    """In-degrees 1, 4 and 16 only: every edge weight is a power of two, so with small-integer x and W the sums, every
    piece product and every partial sum are exact - the layer must be BIT-equal to float64 (as
    test_x3_gcn_layer_exact_on_integers), in each prefix-width instantiation, with 4, 3, 2 and 1 K-steps in the matrix
    chain, with one and with two destinations.  B = 136: 289 items on the 256 waves of an XCD group - 33 waves run a
    second item."""
    x, W, b = exact_data
    x, W = x[..., :Fin].contiguous(), W[:, :Fin].contiguous()
    G = graphs[f"x{ew}"]
    ei = G.export_edges()  # with self-loops, PyG order: (sender, receiver)
    deg = torch.bincount(ei[1], minlength=NW).double()
    wgt = 1.0 / torch.sqrt(deg[ei[0]] * deg[ei[1]])
    agg = torch.zeros(x.shape, dtype=torch.float64)
    agg.index_add_(1, ei[1], x.double()[:, ei[0]] * wgt[None, :, None])
    ref = (agg @ W.double().t() + b.double()).float()
    got = both(hip, monkeypatch, G, x.to(DEV), hip.ACT_NONE, W.to(DEV), b.to(DEV), head=head)
    got = torch.cat(got, 1).cpu()
    assert torch.equal(got, ref), f"{(got != ref).sum().item()} elements differ"
