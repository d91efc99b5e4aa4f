"""The encoder-output gradient is handed over without staging copies, and the batch sum of the folded rows keeps several
samples' loads in flight.

gcl_aggregate_split / gcl_colsum_split read a [B, n, F] source whose first `head` rows per sample and whose other rows
live in two tensors; the encoder GCN stack's backward uses them on the two parts its gradient arrives in
(GCL_NO_SPLIT_GRAD=1: the parts are copied into one buffer first).  batch_sum_rows_kernel replaces gather2_kernel's
sum_batch case (GCL_NO_BATCH_SUM=1: the old kernel).  gcl_aggregate_compact gives the source-tile aggregation a store
map, so the first processor layer's transposed aggregation writes the batch-dependent rows of its output where the dense
backward wants them (GCL_NO_COMPACT_STORE=1: a gather launch copies them).  Arithmetic and summation order are those of the existing kernels, so
every comparison with them is torch.equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("GCL_NO_SPLIT_GRAD", "GCL_NO_BATCH_SUM", "GCL_NO_COMPACT_STORE", "GCL_AGG_HALO")
NAN = float("nan")


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


N, HEAD = 203, 37  # the boundary falls inside a 4-row wave-instruction (37 = 9 * 4 + 1) and inside a 16-row group


@pytest.fixture(scope="module")
def bip_graph(hip):
    """Random bipartite-plus-self-loops graph on 203 rows: edges run between the first 37 rows and the others in both
    directions (so rows gather from both parts, transposed or not), one row has 70 in-edges and one 70 out-edges (the
    one-block-per-row kernel in either direction), and 203 rows leave a ragged last block."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, HEAD, 500)
    b = rng.integers(HEAD, N, 500)
    fwd = np.stack([a, b])
    bwd = np.stack([b[:300], a[:300]])
    heavy_in = np.stack([rng.choice(np.setdiff1d(np.arange(N), [100]), 70, replace=False), np.full(70, 100)])
    heavy_out = np.stack([np.full(70, 20), rng.choice(np.setdiff1d(np.arange(N), [20]), 70, replace=False)])
    ei = torch.unique(torch.from_numpy(np.concatenate([fwd, bwd, heavy_in, heavy_out], 1)), dim=1)
    G = hip.Graph(ei, N, hip.GRAPH_GCN)
    assert G.max_in_degree > 64
    return G


def two_parts(B, n, head, F, seed):
    """(a3 [B, head, F], b3 [B, n - head, F], dense [B, n, F]): the parts sit in separately allocated tensors with
    different row and batch strides - a3 is a slice of a wider, longer tensor - and everything around them is NaN."""
    dense = rnd(B, n, F, seed=seed)
    big_a = torch.full((B, head + 5, F + 8), NAN)
    big_a[:, 2: 2 + head, 4: 4 + F] = dense[:, :head]
    big_b = torch.full((B, n - head + 3, F), NAN)
    big_b[:, 1: 1 + n - head] = dense[:, head:]
    a3 = big_a.to(DEV)[:, 2: 2 + head, 4: 4 + F]
    b3 = big_b.to(DEV)[:, 1: 1 + n - head]
    return a3, b3, dense.to(DEV)


@pytest.mark.parametrize("F", [64, 48])
@pytest.mark.parametrize("tr", [False, True])
@pytest.mark.parametrize("head", [HEAD, 0, N])
def test_aggregate_split_equals_aggregate_on_one_tensor(hip, bip_graph, F, tr, head):
    a3, b3, dense = two_parts(3, N, head, F, seed=31 + head)
    ref = hip.aggregate(bip_graph, dense, None, transpose=tr)
    got = hip.aggregate_split(bip_graph, a3, b3, transpose=tr)
    assert bool(torch.isfinite(got).all()), "a row outside the two parts was read"
    assert torch.equal(got, ref)


@pytest.mark.parametrize("F", [64, 48])
@pytest.mark.parametrize("head", [HEAD, 0, N])
def test_colsum_split_equals_colsum_on_one_tensor(hip, F, head):
    a3, b3, dense = two_parts(3, N, head, F, seed=41 + head)
    for acc in (False, True):
        ref = torch.full((F,), 0.5, device=DEV)
        got = ref.clone()
        hip.colsum(dense.view(-1, F), ref, acc)
        hip.colsum_split(a3, b3, got, acc)
        assert bool(torch.isfinite(got).all()), "a row outside the two parts was read"
        assert torch.equal(got, ref)


@pytest.mark.parametrize("B", [6, 330])
def test_colsum_split_deferred_and_four_rows_in_flight(hip, B):
    """B = 6: 77 blocks, so the final pass is queued (gcl_reduce_jobs) - the same records as gcl_colsum_deferred.
    B = 330: 66 990 rows on 1024 blocks, so every lane group walks more than four trips (the four-rows-in-flight loop
    and its one-row tail)."""
    F = 64
    a3, b3, dense = two_parts(B, N, HEAD, F, seed=51)
    outs = []
    for split in (False, True):
        out = torch.full((F,), -2.0, device=DEV)
        hip.defer_begin()
        try:
            if split:
                hip.colsum_split(a3, b3, out, True)
            else:
                hip.colsum(dense.view(-1, F), out, True)
        finally:
            hip.defer_flush()
        outs.append(out)
    assert bool(torch.isfinite(outs[1]).all())
    assert torch.equal(outs[0], outs[1])
    now = torch.zeros(F, device=DEV)
    hip.colsum_split(a3, b3, now, False)
    ref = torch.zeros(F, device=DEV)
    hip.colsum(dense.view(-1, F), ref, False)
    assert torch.equal(now, ref)


@pytest.mark.parametrize("B", [1, 2, 7, 64])
@pytest.mark.parametrize("r", [1, 3])
def test_fold_sum_equals_old_kernel(hip, monkeypatch, B, r):
    """The batch sums of the folded rows, old kernel against new: values with heavy cancellation (1e6-sized terms of both
    signs around O(1) ones), so any change of the addition order over the batch shows."""
    from graphcast_lite_amd.functional import _fold_sum

    M, F = 255, 64  # (at least B * r = 192 rows: the map below takes B * r distinct ones)
    g3 = rnd(B, M, F, seed=61 + B)
    big = rnd(B, M, F, seed=62 + B, scale=1e6)
    big[1::2] = -big[:-1:2][: big[1::2].shape[0]]  # pairs of opposite 1e6-sized terms
    g3 = (g3 + big).to(DEV)
    gen = torch.Generator().manual_seed(63)
    inv = torch.randperm(M, generator=gen)[: B * r].to(torch.int32)
    assert inv.numel() == B * r
    if B * r > 2:
        inv[1] = -1  # a folded slot without a row: zeros
    inv = inv.to(DEV)
    outs = []
    for old in ("1", "0"):
        monkeypatch.setenv("GCL_NO_BATCH_SUM", old)
        dst = torch.full((B, r + 2, F), NAN, device=DEV)
        _fold_sum(g3, inv, r, B, dst[:, 1: 1 + r])
        assert bool(torch.isnan(dst[:, 0]).all()) and bool(torch.isnan(dst[:, 1 + r:]).all())
        outs.append(dst[:, 1: 1 + r].clone())
        plain = hip.gather2_rows(g3, None, None, None, M, B, sum_batch=True)  # no map (the dual-mesh head's call)
        outs.append(plain)
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])


def test_batch_sum_many_rows(hip, monkeypatch):
    """nd * F / 4 = 33 000 * 64 = 2 112 000 threads: the launch with 256-thread blocks, and more of them than its cap of
    8192, so the grid-stride loop runs too - branches the model's shapes never take (B = 5: one chunk of four loads and
    a single one)."""
    nd, F, B = 33000, 256, 5
    g3 = rnd(B, nd, F, seed=65).to(DEV)
    outs = []
    for old in ("1", "0"):
        monkeypatch.setenv("GCL_NO_BATCH_SUM", old)
        outs.append(hip.gather2_rows(g3, None, None, None, nd, B, sum_batch=True))
    assert torch.equal(outs[0], outs[1])


@pytest.fixture(scope="module")
def mesh23():
    """The [2, 3] mesh graph with its nodes in tile order: 642 rows = ten 64-row tiles and a two-row last one."""
    from conftest import build_graphs, experiment
    from graphcast_lite_amd.mesh import tile_order

    g = build_graphs(experiment("baseline", mesh_levels=[2, 3]))
    n = g["M"]
    deg = torch.bincount(g["proc"][1], minlength=n).numpy()
    order = torch.from_numpy(np.ascontiguousarray(tile_order(g["mesh"].vertices, 64, degree=deg)))
    pos = torch.empty(n, dtype=torch.int64)
    pos[order] = torch.arange(n)
    return dict(n=n, ei=pos[g["proc"]])


@pytest.mark.parametrize("kind", ["none", "all", "random19"])
def test_store_map_writes_each_row_once(hip, mesh23, kind):
    """Transposed source-tile aggregation with a store map, F = 64, B = 9 (more than one XCD group's 8 samples: the map
    entries kept in registers are reused).  The dense output's compact rows and the compact destination's other rows are
    NaN before and must be NaN after; every other row carries gcl_aggregate's bits."""
    n, B, F = mesh23["n"], 9, 64
    assert n % 64 == 2
    G = hip.Graph(mesh23["ei"], n, hip.GRAPH_GCN)
    h = rnd(B, n, F, seed=81).to(DEV)
    assert hip.aggregate_compact_ok(G, h, transpose=True), "the source-tile kernel does not take this graph"
    ref = hip.aggregate(G, h, None, transpose=True)
    gen = torch.Generator().manual_seed(82)
    if kind == "none":
        rows = torch.empty(0, dtype=torch.int64)
    elif kind == "all":
        rows = torch.randperm(n, generator=gen)  # every row compact, in a shuffled order (the last tile's two rows too)
    else:
        rows = torch.nonzero(torch.rand(n, generator=gen) < 0.19).flatten()
        rows = rows[torch.randperm(rows.numel(), generator=gen)]
        rows = torch.unique(torch.cat([rows, torch.tensor([n - 1])]), sorted=False)  # a row of the two-row last tile
    nc = rows.numel()
    smap = torch.full((n,), -1, dtype=torch.int32)
    smap[rows] = torch.arange(nc, dtype=torch.int32)
    out = torch.full((B, n, F), NAN, device=DEV)
    big = torch.full((B, nc + 3, F), NAN, device=DEV)
    outc = big[:, 1: 1 + nc]
    hip.aggregate_compact(G, h, smap.to(DEV), outc, transpose=True, out=out)
    compact = (smap >= 0).to(DEV)
    assert bool(torch.isnan(out[:, compact]).all()), "a compact row was also written in place"
    assert torch.equal(out[:, ~compact], ref[:, ~compact])
    assert torch.equal(outc, ref[:, rows.to(DEV)])
    assert bool(torch.isnan(big[:, 0]).all()) and bool(torch.isnan(big[:, 1 + nc:]).all())


def _step(m, X, y, calls=None):
    from graphcast_lite_amd.train import batch_loss

    m.zero_grad()
    out = m(X).detach().clone()
    batch_loss(m, X, y).backward()
    return out, {n_: p.grad.clone() for n_, p in m.named_parameters()}


@pytest.fixture
def count_split(hip, monkeypatch):
    calls = {"agg": 0, "colsum": 0, "compact": 0}
    agg, cs, cp = hip.aggregate_split, hip.colsum_split, hip.aggregate_compact

    def cp_(*a, **k):
        calls["compact"] += 1
        return cp(*a, **k)

    def agg_(*a, **k):
        calls["agg"] += 1
        return agg(*a, **k)

    def cs_(*a, **k):
        calls["colsum"] += 1
        return cs(*a, **k)

    monkeypatch.setattr(hip, "aggregate_split", agg_)
    monkeypatch.setattr(hip, "colsum_split", cs_)
    monkeypatch.setattr(hip, "aggregate_compact", cp_)
    return calls


@pytest.mark.parametrize("name,levels", [("baseline", [1, 2]), ("attention", [1, 2]), ("baseline", [3, 5])])
def test_model_equal_with_and_without_the_handoffs(name, levels, monkeypatch, count_split):
    """Prediction and every parameter gradient, all switches off against on.  [1, 2]: the smallest GCN and GAT
    configs; [3, 5]: the benchmark's mesh, where the first processor layer reads through the row table and its backward
    is the tail writer."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair(name, levels)
    X, y = data(cfg, m._num_grid_nodes, 3)
    X, y = X.to(DEV), y.to(DEV)
    out_new, g_new = _step(m, X, y)
    assert count_split["agg"] == 1 and count_split["colsum"] == 1, "the two-part reader did not engage"
    if levels == [3, 5]:
        assert count_split["compact"] == 1, "the store map did not engage on the benchmark's mesh"
    for k in ("GCL_NO_SPLIT_GRAD", "GCL_NO_BATCH_SUM", "GCL_NO_COMPACT_STORE"):
        monkeypatch.setenv(k, "1")
    out_old, g_old = _step(m, X, y)
    assert count_split["agg"] == 1 and count_split["compact"] <= 1
    assert torch.equal(out_new, out_old)
    for n_, g in g_old.items():
        assert torch.equal(g_new[n_], g), n_


def test_claim_parts_fallback_is_exact(hip):
    """The fallback's own arithmetic, bit for bit: a gradient that is not the token comes back as itself plus the two kept
    parts laid out as one dense buffer; the token with no tail part (the mesh side sent nothing) comes back as the head
    rows over zeros; the token with both parts hands the parts through untouched.  The landing is emptied each time."""
    from graphcast_lite_amd.functional import GradLanding, _token

    B, F = 3, 64
    a3, b3, dense = two_parts(B, N, HEAD, F, seed=91)
    other = rnd(B, N, F, seed=92).to(DEV)
    land = GradLanding(HEAD, head_identity=True)
    land.part_head, land.part_tail = a3, b3
    dy, parts = GradLanding.claim_parts(land, other)
    assert parts is None and torch.equal(dy, other + dense)
    assert land.part_head is None and land.part_tail is None
    land.part_head, land.part_tail = a3, None
    dy, parts = GradLanding.claim_parts(land, _token(dense, (B, N, F)))
    head_only = dense.clone()
    head_only[:, HEAD:] = 0.0
    assert parts is None and torch.equal(dy, head_only)
    land.part_head, land.part_tail = a3, b3
    tok = _token(dense, (B, N, F))
    dy, parts = GradLanding.claim_parts(land, tok)
    assert dy is tok and parts[0] is a3 and parts[1] is b3 and land.part_head is None


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_second_gradient_into_the_grid_latents_is_added(name, count_split):
    """forward_with_latents also returns the grid latents - a view of the encoder output.  A loss on them sends a second
    gradient to the encoder output, autograd sums it with the token, and the stack's backward must build the dense buffer
    and add.  Reference: a twin with plain autograd accumulation (no landing) - the switched-off path shares one buffer
    under the same one-consumer assumption, so it is no reference here; the twin differs from the landing elsewhere by
    summation order, hence the suite's usual bound for that comparison instead of torch.equal
    (test_claim_parts_fallback_is_exact checks the fallback's own arithmetic bit for bit)."""
    from test_hip_model import data, make_pair

    cfg, m1, _ = make_pair(name, [1, 2])
    _, m2, _ = make_pair(name, [1, 2])
    X, _ = data(cfg, m1._num_grid_nodes, 3)
    m2._grad_landing = False
    w = rnd(3, m1._num_grid_nodes, 1, seed=71).to(DEV)
    grads = []
    for m in (m1, m2):
        out, grid_lat, _ = m.forward_with_latents(X.to(DEV), _landing=True, _latents_discarded=True)
        (out.pow(2).mean() + (grid_lat * w).mean()).backward()
        grads.append({n_: p.grad.clone() for n_, p in m.named_parameters()})
    assert count_split["agg"] == 0, "the token was taken although a second gradient arrived"
    gn = float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads[1].values())))
    for n_, g in grads[1].items():
        d = float((grads[0][n_].double() - g.double()).norm())
        assert d <= 1e-5 * float(g.double().norm()) + 1e-7 * gn, n_
    # and the second gradient is really there: without it the encoder's gradients differ by far more than the bound
    m1.zero_grad()
    out, _, _ = m1.forward_with_latents(X.to(DEV), _landing=True, _latents_discarded=True)
    out.pow(2).mean().backward()
    far = max(float((p.grad.double() - grads[1][n_].double()).norm()) / (float(grads[1][n_].double().norm()) + 1e-30)
              for n_, p in m1.named_parameters() if n_.startswith("encoder"))
    assert far > 1e-3


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_two_forwards_in_flight_then_both_backwards(name, monkeypatch, count_split):
    """Each forward makes its own landing: two calls in flight, then both backwards, equal the switched-off path bit for
    bit."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair(name, [1, 2])
    X1, _ = data(cfg, m._num_grid_nodes, 3)
    X2, _ = data(cfg, m._num_grid_nodes, 3, seed=4321)
    res = []
    for old in ("0", "1"):
        monkeypatch.setenv("GCL_NO_SPLIT_GRAD", old)
        m.zero_grad()
        o1 = m(X1.to(DEV))
        o2 = m(X2.to(DEV))
        o1.pow(2).mean().backward()
        (0.5 * o2.pow(2).mean()).backward()
        res.append((o1.detach().clone(), o2.detach().clone(), {n_: p.grad.clone() for n_, p in m.named_parameters()}))
    assert count_split["agg"] == 2
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for n_, g in res[1][2].items():
        assert torch.equal(res[0][2][n_], g), n_
