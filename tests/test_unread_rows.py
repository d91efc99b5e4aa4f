"""Rows that a stage boundary drops are neither written by their producer nor read by their consumers.

The decoder-input gather of WeatherPrediction.forward keeps U of the M processor rows (GCL_NO_ROW_SKIP=1 restores the
dense launches).  The presence of a row is an int32 table per node, entry >= 0 = present.  Every kept row is computed by the same instructions in the same order as on the dense path,
so every comparison here is torch.equal - no tolerance."""
import numpy as np
import pytest
import torch

from conftest import build_graphs, experiment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("GCL_NO_ROW_SKIP", "GCL_AGG_HALO")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


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
    return dict(n=n, ei=pos[g["proc"]])


@pytest.fixture(scope="module")
def dec35():
    """The compact decoder graph of the baseline model at mesh [3, 5]: rows [G grid | U mesh rows with grid receivers]."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair("baseline", [3, 5])
    X, _ = data(cfg, m._num_grid_nodes, 1)
    with torch.no_grad():
        m(X.to(DEV))
    c = m._compact
    return dict(n=m._num_grid_nodes + c.U, G=m._num_grid_nodes, ei=c.dec_graph.cpu())


def random_presence(n, seed, frac=0.47):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(n, generator=g) < frac
    tab = torch.full((n,), -1, dtype=torch.int32)
    tab[keep] = torch.arange(int(keep.sum()), dtype=torch.int32)
    return tab


def with_absent(t3, tab, value):
    out = t3.clone()
    out[:, tab < 0] = value
    return out


def _agg_case(hip, G, n, B, F, tab, tr, seed):
    """aggregate_present on an input whose absent rows are NaN == aggregate on the input with zeros there."""
    ld = (F + 3) // 4 * 4
    h = torch.zeros(B, n, ld)
    h[..., :F] = rnd(B, n, F, seed=seed)
    ref = hip.aggregate(G, with_absent(h, tab, 0.0).to(DEV)[..., :F], None, transpose=tr)
    for fill in (0.0, float("nan")):
        got = hip.aggregate_present(G, with_absent(h, tab, fill).to(DEV)[..., :F], tab.to(DEV), transpose=tr)
        assert bool(torch.isfinite(got).all()), "an absent source row was read"
        assert torch.equal(got, ref)


@pytest.mark.parametrize("F", [64, 36])
@pytest.mark.parametrize("tr", [False, True])
def test_aggregate_absent_sources_mesh(hip, mesh35, F, tr, monkeypatch):
    """Mesh graph in tile order, B = 9 (uneven XCD groups): the source-tile kernel and the per-edge kernel."""
    n = mesh35["n"]
    G = hip.Graph(mesh35["ei"], n, hip.GRAPH_GCN)
    assert G.halo_info(tr, 64) is not None
    for mode in ("1", "0"):
        monkeypatch.setenv("GCL_AGG_HALO", mode)
        _agg_case(hip, G, n, 9, F, random_presence(n, 3), tr, seed=11)
        head = torch.where(torch.arange(n) < n // 3, 0, -1).to(torch.int32)
        _agg_case(hip, G, n, 9, F, head, tr, seed=12)


@pytest.mark.parametrize("F", [64, 36])
@pytest.mark.parametrize("tr", [False, True])
def test_aggregate_absent_sources_decoder_graph(hip, dec35, F, tr):
    """The compact decoder graph (3.3 edges per row: the per-edge kernel), random presence and the "row < G" form."""
    n, Gr = dec35["n"], dec35["G"]
    G = hip.Graph(dec35["ei"], n, hip.GRAPH_GCN)
    _agg_case(hip, G, n, 9, F, random_presence(n, 5), tr, seed=13)
    _agg_case(hip, G, n, 9, F, torch.where(torch.arange(n) < Gr, 0, -1).to(torch.int32), tr, seed=14)


@pytest.mark.parametrize("tr", [False, True])
def test_aggregate_absent_sources_heavy_rows(hip, mesh35, tr):
    """A row with more than 64 edges in either direction is summed by the one-block-per-row kernel: same contract."""
    n = mesh35["n"]
    rng = np.random.default_rng(0)
    heavy = 4000
    far = torch.from_numpy(rng.choice(np.setdiff1d(np.arange(n), [heavy]), 90, replace=False))
    ei = torch.cat([mesh35["ei"], torch.stack([far, torch.full_like(far, heavy)]),
                    torch.stack([torch.full_like(far, heavy + 1), far])], 1)
    ei = torch.unique(ei, dim=1)
    G = hip.Graph(ei, n, hip.GRAPH_GCN)
    assert G.max_in_degree > 64
    _agg_case(hip, G, n, 9, 64, random_presence(n, 7), tr, seed=15)


@pytest.mark.parametrize("act", ["none", "prelu"])
def test_gcn_layer_output_row_predicate(hip, mesh35, act):
    """The one-kernel layer with the predicate, into a buffer pre-filled with a sentinel: present rows are the plain
    layer's bits, absent rows are not written."""
    n, B = mesh35["n"], 9
    G = hip.Graph(mesh35["ei"], n, hip.GRAPH_GCN)
    x = rnd(B, n, 64, seed=21).to(DEV)
    W, b = rnd(64, 64, seed=22, scale=0.2).to(DEV), rnd(64, seed=23).to(DEV)
    a, slope = (hip.ACT_PRELU, torch.tensor([0.25], device=DEV)) if act == "prelu" else (hip.ACT_NONE, None)
    assert hip.gcn_layer_fusable(G, x, 64, 64)
    ref = hip.gcn_layer_fwd(G, x, a, slope, W, b)
    tab = random_presence(n, 9)
    out = torch.full((B, n, 64), 12345.0, device=DEV)
    got = hip.gcn_layer_fwd(G, x, a, slope, W, b, out=out, present=tab.to(DEV))
    keep = (tab >= 0).to(DEV)
    assert torch.equal(got[:, keep], ref[:, keep])
    assert bool((got[:, ~keep] == 12345.0).all()), "an absent row was stored"


@pytest.mark.parametrize("B,n,F", [(9, 10242, 64), (3, 1000, 64), (2, 333, 48)])
def test_layernorm_skip_pair(hip, B, n, F):
    """The mapped LayerNorm pair with skip against the mapped pair: outputs, statistics and dx of present rows, dgamma,
    dbeta and the column sums are equal; with NaN in every absent row of x and of the statistics nothing changes."""
    tab = random_presence(n, 17)
    U = int((tab >= 0).sum())
    head = 5
    pos = torch.where(tab >= 0, tab + head, tab).to(DEV)
    rlist = torch.nonzero(tab >= 0).flatten().to(torch.int32).to(DEV)
    keep = (tab >= 0).to(DEV)
    x3 = rnd(B, n, F, seed=31)
    gam, bet = (1 + 0.1 * rnd(F, seed=32)).to(DEV), rnd(F, seed=33).to(DEV)
    # reference: today's mapped pair on zeros in the absent rows
    xz = with_absent(x3, tab, 0.0).to(DEV)
    out_r = torch.full((B, head + U, F), 7.0, device=DEV)
    stats_r = hip.layernorm_fwd_map(xz.view(B * n, F), gam, bet, 1e-5, out_r, pos)
    src = rnd(B, head + U, F, seed=34).to(DEV)

    def bwd(x2, stats, skip):
        dg, db, cs = torch.zeros(F, device=DEV), torch.zeros(F, device=DEV), torch.zeros(F, device=DEV)
        dx = hip.layernorm_bwd(None, x2, gam, stats, dg, db, False, colsum_dx=cs, dy_map=(src, pos), skip=skip)
        return dx.view(B, n, F), dg, db, cs

    dx_r, dg_r, db_r, cs_r = bwd(xz.view(B * n, F), stats_r, False)
    for fill in (0.0, float("nan")):
        xs = with_absent(x3, tab, fill).to(DEV)
        out_s = torch.full((B, head + U, F), 7.0, device=DEV)
        stats_s = hip.layernorm_fwd_map_skip(xs.view(B * n, F), gam, bet, 1e-5, out_s, pos, rlist)
        assert torch.equal(out_s, out_r) and bool(torch.isfinite(out_s).all())
        assert torch.equal(stats_s.view(B, n, 2)[:, keep], stats_r.view(B, n, 2)[:, keep])
        st = stats_s.view(B, n, 2).clone()
        st[:, ~keep] = fill  # whatever the unwritten statistics hold
        dx_s, dg_s, db_s, cs_s = bwd(xs.view(B * n, F), st.view(B * n, 2), True)
        assert torch.equal(dx_s[:, keep], dx_r[:, keep])
        for got, ref in ((dg_s, dg_r), (db_s, db_r), (cs_s, cs_r)):
            assert bool(torch.isfinite(got).all()), "an absent row entered a partial sum"
            assert torch.equal(got, ref)


class _Kinds:
    """Launch probe that records the kinds it sees, and the node count of the graph of every `aggregate_present`."""

    def __init__(self):
        self.kinds, self.present_n = [], []

    def begin(self, kind, **info):
        self.kinds.append(kind)
        if kind == "aggregate_present":
            self.present_n.append(info["graph"].n)
        return None

    def end(self, tok):
        pass


def _one_step(name, monkeypatch, off):
    from graphcast_lite_amd import hip as H
    from graphcast_lite_amd.train import batch_loss
    from test_hip_model import data, make_pair

    monkeypatch.setenv("GCL_NO_ROW_SKIP", "1") if off else monkeypatch.delenv("GCL_NO_ROW_SKIP", raising=False)
    cfg, m, _ = make_pair(name, [3, 5])
    X, y = data(cfg, m._num_grid_nodes, 5)
    probe = _Kinds()
    monkeypatch.setattr(H, "PROBE", probe)
    out = m(X.to(DEV))
    loss = batch_loss(m, X.to(DEV), y.to(DEV))
    loss.backward()
    monkeypatch.setattr(H, "PROBE", None)
    sizes = dict(mesh=m._num_mesh_nodes)
    return out.detach(), loss.detach(), {n_: p.grad.clone() for n_, p in m.named_parameters()}, probe, sizes


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_model_equal_with_and_without_skips(name, monkeypatch):
    """Prediction, loss and every parameter gradient are the same bits with the row skip and with it switched off."""
    out_s, loss_s, g_s, pr_s, sz = _one_step(name, monkeypatch, off=False)
    out_d, loss_d, g_d, pr_d, _ = _one_step(name, monkeypatch, off=True)
    if name == "baseline":  # the GCN processor's tail takes the row-skip launches, which report under their own kinds
        assert pr_s.present_n == [sz["mesh"]] and "gcn_layer_fwd_present" in pr_s.kinds
    assert "aggregate_present" not in pr_d.kinds and "gcn_layer_fwd_present" not in pr_d.kinds
    assert torch.equal(out_s, out_d) and torch.equal(loss_s, loss_d)
    assert g_s.keys() == g_d.keys()
    for n_ in g_s:
        assert torch.equal(g_s[n_], g_d[n_]), n_


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_captured_train_step_equal_with_and_without_skips(name, monkeypatch):
    """Three steps of a captured TrainStep (warm-up, capture, replay): the weights after the third step are equal."""
    from graphcast_lite_amd.train import TrainStep
    from test_hip_model import data, make_pair

    weights = []
    for off in (False, True):
        monkeypatch.setenv("GCL_NO_ROW_SKIP", "1") if off else monkeypatch.delenv("GCL_NO_ROW_SKIP", raising=False)
        cfg, m, _ = make_pair(name, [3, 5])
        X, y = data(cfg, m._num_grid_nodes, 5)
        ts = TrainStep(m, lr=1e-3, use_graph=True)
        for _ in range(3):
            ts(X.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        assert ts.graph_active
        weights.append({n_: p.detach().clone() for n_, p in m.named_parameters()})
    for n_ in weights[0]:
        assert torch.equal(weights[0][n_], weights[1][n_]), n_


def test_second_gradient_into_processor_output_is_an_error_not_garbage(monkeypatch):
    """With the row skip on, the dropped rows of the processor's tail do not exist, so a gradient that reaches the
    processor's output from anywhere but the decoder-input gather cannot be honoured: the backward raises and names the
    switch.  With GCL_NO_ROW_SKIP=1 the same model takes the dense path and the backward runs."""
    from graphcast_lite_amd.train import batch_loss
    from test_hip_model import data, make_pair

    def run():
        cfg, m, _ = make_pair("baseline", [3, 5])
        orig = m.processor.forward

        def fwd(*a, **k):
            out = orig(*a, **k)
            out.register_hook(lambda g: g + 1.0)  # a second consumer: the token becomes a real dense gradient
            return out

        m.processor.forward = fwd
        X, y = data(cfg, m._num_grid_nodes, 2)
        batch_loss(m, X.to(DEV), y.to(DEV)).backward()
        return m

    with pytest.raises(RuntimeError, match="GCL_NO_ROW_SKIP"):
        run()
    monkeypatch.setenv("GCL_NO_ROW_SKIP", "1")
    m = run()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
