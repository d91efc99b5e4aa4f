"""The encoder output is stored where its two readers take it from.

gcl_gcn_layer_fwd_split is the one-kernel GCNConv layer with a two-part destination: rows < head of every sample go to
one tensor, the others to a second one with strides of its own.  Inside WeatherPrediction.forward the encoder's last conv
uses it to store the grid rows straight into the decoder's input and the mesh rows compact, so neither reader copies
(GCL_NO_SPLIT_OUT=1: one tensor and two copy launches).  Tokens - the stride-0 zeros that stand in autograd's graph for
such rows - expand one zero per device instead of launching a fill each.  No arithmetic changes, so every comparison is
torch.equal."""
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
    for k in ("GCL_NO_SPLIT_OUT", "GCL_NO_ROW_SKIP"):
        monkeypatch.delenv(k, raising=False)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


@pytest.fixture(scope="module")
def bip_graph(hip):
    """Random bipartite-plus-self-loops graph on 203 rows: edges run between the first 64 rows and the others in both
    directions, so rows on either side of every tested boundary gather from both sides.  No row has more than 64 in-edges
    (the one-kernel layer's range)."""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 64, 700)
    b = rng.integers(64, N, 700)
    ei = torch.unique(torch.from_numpy(np.concatenate([np.stack([a, b]), np.stack([b[:400], a[:400]])], 1)), dim=1)
    G = hip.Graph(ei, N, hip.GRAPH_GCN)
    assert G.max_in_degree <= 64
    return G


def two_dests(B, n, head, F, pad_a=8):
    """(big_a, ya, big_b, yb): NaN-filled tensors and the two destination views inside them - ya a slice of a wider,
    longer tensor, yb of a longer one, so row and batch strides differ between the parts."""
    big_a = torch.full((B, head + 5, F + pad_a), NAN, device=DEV)
    big_b = torch.full((B, n - head + 3, F), NAN, device=DEV)
    return big_a, big_a[:, 2: 2 + head, 4: 4 + F], big_b, big_b[:, 1: 1 + n - head]


def only_views_written(big, view):
    """Every element of `big` outside `view` is still NaN."""
    mask = torch.zeros_like(big, dtype=torch.bool)
    mask.as_strided(view.shape, view.stride(), view.storage_offset() - big.storage_offset()).fill_(True)
    return bool(torch.isnan(big[~mask]).all())


@pytest.fixture(scope="module")
def layer_ref(hip, bip_graph):
    """gcl_gcn_layer_fwd on one tensor, once per (Fin, activation): the reference of every head."""
    B, Fout = 3, 64
    slope = torch.tensor([0.25], device=DEV)
    ref = {}
    for Fin in (64, 48):
        x = rnd(B, N, Fin, seed=11 + Fin).to(DEV)
        W = rnd(Fout, Fin, seed=12 + Fin, scale=0.2).to(DEV)
        b = rnd(Fout, seed=13 + Fin).to(DEV)
        for act in (hip.ACT_NONE, hip.ACT_PRELU):
            sl = slope if act == hip.ACT_PRELU else None
            ref[(Fin, act)] = (x, W, b, sl, hip.gcn_layer_fwd(bip_graph, x, act, sl, W, b).clone())
    return ref


@pytest.mark.parametrize("head", [32, 64, 160])
@pytest.mark.parametrize("act", ["none", "prelu"])
@pytest.mark.parametrize("Fin", [64, 48])
def test_split_layer_equals_the_layer_on_one_tensor(hip, bip_graph, layer_ref, Fin, act, head):
    x, W, b, sl, ref = layer_ref[(Fin, hip.ACT_PRELU if act == "prelu" else hip.ACT_NONE)]
    B, Fout = x.shape[0], W.shape[0]
    big_a, ya, big_b, yb = two_dests(B, N, head, Fout)
    assert hip.gcn_layer_split_ok(bip_graph, x, Fout, ya, yb)
    hip.gcn_layer_fwd_split(bip_graph, x, hip.ACT_PRELU if act == "prelu" else hip.ACT_NONE, sl, W, b, ya, yb)
    assert torch.equal(ya, ref[:, :head]) and torch.equal(yb, ref[:, head:])
    assert only_views_written(big_a, ya) and only_views_written(big_b, yb)


def _raw(hip, G, x, W, b, ya, yb, head):
    """(the _ok query, the entry's return code) with the given head, bypassing the Python wrapper's own checks."""
    L = hip.lib()
    B, n, Fin = x.shape
    Fout = W.shape[0]
    ok = L.gcl_gcn_layer_fwd_split_ok(G.handle, x.stride(1), x.stride(0), ya.stride(1), ya.stride(0), yb.stride(1), yb.stride(0),
                                      head, B, Fin, Fout, Fout)
    rc = L.gcl_gcn_layer_fwd_split(G.handle, x.data_ptr(), x.stride(1), x.stride(0), hip.ACT_NONE, None, W.data_ptr(),
                                   b.data_ptr(), ya.data_ptr(), ya.stride(1), ya.stride(0), yb.data_ptr(), yb.stride(1),
                                   yb.stride(0), head, B, Fin, Fout, Fout, None)
    torch.cuda.synchronize()
    return ok, rc


@pytest.mark.parametrize("case", ["head37", "head0", "headn", "stride"])
def test_split_layer_refusals(hip, bip_graph, layer_ref, case):
    """A boundary inside a 32-row tile, an empty part and a part whose rows are not whole 16-byte units: the query says
    0, the entry returns an error and writes nothing."""
    x, W, b, _, _ = layer_ref[(64, hip.ACT_NONE)]
    head = {"head37": 37, "head0": 0, "headn": N, "stride": 64}[case]
    rows_a = head if 0 < head < N else 64  # (the views only have to exist: an empty part is refused on `head` alone)
    big_a, ya, big_b, yb = two_dests(3, N, rows_a, 64, pad_a=6 if case == "stride" else 8)
    if case == "stride":
        assert ya.stride(1) % 4 != 0
    ok, rc = _raw(hip, bip_graph, x, W, b, ya, yb, head)
    assert ok == 0 and rc != 0
    assert bool(torch.isnan(big_a).all()) and bool(torch.isnan(big_b).all())
    if case == "head37":
        assert not hip.gcn_layer_split_ok(bip_graph, x, 64, ya, yb)
    # the accepted shape next to it, so that the refusals above are refusals of the case and not of the set-up
    big_a, ya, big_b, yb = two_dests(3, N, 64, 64)
    assert _raw(hip, bip_graph, x, W, b, ya, yb, 64) == (1, 0)


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def counts(hip, monkeypatch):
    calls = {"copy": 0, "split": 0}
    cp, sp = hip.copy_rows, hip.gcn_layer_fwd_split

    def cp_(*a, **k):
        calls["copy"] += 1
        return cp(*a, **k)

    def sp_(*a, **k):
        calls["split"] += 1
        return sp(*a, **k)

    monkeypatch.setattr(hip, "copy_rows", cp_)
    monkeypatch.setattr(hip, "gcn_layer_fwd_split", sp_)
    return calls


def _step(m, X, y):
    from graphcast_lite_amd.train import batch_loss

    m.zero_grad()
    out = m(X).detach().clone()
    loss = batch_loss(m, X, y)
    loss.backward()
    return out, loss.detach().clone(), {n_: p.grad.clone() for n_, p in m.named_parameters()}


def _both_ways(m, X, y, monkeypatch, counts):
    """((prediction, loss, gradients), copies, split launches) on the default path and with GCL_NO_SPLIT_OUT=1."""
    res = []
    for off in ("0", "1"):
        monkeypatch.setenv("GCL_NO_SPLIT_OUT", off)
        counts["copy"] = counts["split"] = 0
        r = _step(m, X, y)
        res.append((r, counts["copy"], counts["split"]))
    return res


def _assert_equal_steps(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for n_, g in b[2].items():
        assert torch.equal(a[2][n_], g), n_


@pytest.mark.parametrize("name,levels", [("baseline", [1, 2]), ("attention", [1, 2]), ("baseline", [3, 5])])
def test_model_equal_with_and_without_the_split(name, levels, monkeypatch, counts):
    """64 x 32 grid, B = 3, the smallest GCN and GAT configs and the benchmark's mesh: prediction, loss and every
    parameter gradient, and the launches that went away - per forward the copy in the decoder-input gather, and the copy
    of the compact mesh rows in the forward (GAT) or in the backward (GCN).  _step runs two forwards and one backward."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair(name, levels)
    X, y = data(cfg, m._num_grid_nodes, 3)
    (new, cp_new, sp_new), (old, cp_old, sp_old) = _both_ways(m, X.to(DEV), y.to(DEV), monkeypatch, counts)
    assert sp_new == 2 and sp_old == 0, "the two-part store did not engage"
    assert cp_old - cp_new == (4 if name == "attention" else 3), (cp_old, cp_new)
    assert cp_new == 0
    _assert_equal_steps(new, old)


@pytest.mark.parametrize("case", ["grid63x31", "no_table"])
def test_model_keeps_the_old_path_where_the_split_is_refused(case, monkeypatch, counts):
    """63 x 31 = 1953 grid nodes: no multiple of 32, the boundary would fall inside a wave tile.  no_table: the mesh
    side gathers its latents (MeshLatFn) instead of reading through a LatSource.  Both take today's path and equal
    themselves with the switch."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair("baseline", [1, 2], **({"nlat": 31, "nlon": 63} if case == "grid63x31" else {}))
    if case == "no_table":
        m._lat_through_table = False
    assert (m._num_grid_nodes % 32 != 0) == (case == "grid63x31")
    X, y = data(cfg, m._num_grid_nodes, 3)
    (new, cp_new, sp_new), (old, cp_old, sp_old) = _both_ways(m, X.to(DEV), y.to(DEV), monkeypatch, counts)
    assert sp_new == 0 and sp_old == 0 and cp_new == cp_old and cp_old >= 2
    _assert_equal_steps(new, old)


def test_forward_with_latents_sees_the_grid_latents(monkeypatch, counts):
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair("baseline", [1, 2])
    X, _ = data(cfg, m._num_grid_nodes, 3)
    res = []
    for off in ("0", "1"):
        monkeypatch.setenv("GCL_NO_SPLIT_OUT", off)
        with torch.no_grad():
            out, grid_lat, _ = m.forward_with_latents(X.to(DEV))
        res.append((out.clone(), grid_lat.clone()))
    assert counts["split"] == 0, "a caller that sees the latents got the two-part store"
    assert res[0][1].shape == (3, m._num_grid_nodes, 64) and bool(torch.isfinite(res[0][1]).all())
    assert float(res[0][1].abs().max()) > 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    monkeypatch.setenv("GCL_NO_SPLIT_OUT", "0")
    with torch.no_grad():
        assert torch.equal(m(X.to(DEV)), res[0][0])  # ... and forward(), which does split, predicts the same
    assert counts["split"] == 1


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_two_forwards_in_flight_then_both_backwards(name, counts):
    """Each forward has its own landing, decoder input and compact rows: two calls in flight, then both backwards, equal
    the two run one after the other."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair(name, [1, 2])
    X1, _ = data(cfg, m._num_grid_nodes, 3)
    X2, _ = data(cfg, m._num_grid_nodes, 3, seed=4321)
    X1, X2 = X1.to(DEV), X2.to(DEV)
    m.zero_grad()
    o1 = m(X1)
    o2 = m(X2)
    o1.pow(2).mean().backward()
    (0.5 * o2.pow(2).mean()).backward()
    flight = (o1.detach().clone(), o2.detach().clone(), {n_: p.grad.clone() for n_, p in m.named_parameters()})
    assert counts["split"] == 2
    m.zero_grad()
    p1 = m(X1)
    p1.pow(2).mean().backward()
    p2 = m(X2)
    (0.5 * p2.pow(2).mean()).backward()
    assert torch.equal(flight[0], p1.detach()) and torch.equal(flight[1], p2.detach())
    for n_, p in m.named_parameters():
        assert torch.equal(flight[2][n_], p.grad), n_


@pytest.mark.parametrize("name", ["baseline", "attention"])
def test_tokens_share_a_zero_nobody_writes(name, monkeypatch, counts):
    """Hooks send a second gradient into the processor's output and into the encoder output - both are tokens in the
    forward and receive tokens in the backward, so autograd adds the hook's tensor to the shared zero and GradLanding.claim
    / claim_parts take their dense fallbacks.  The zero must still be zero, and the gradients those of the switched-off
    run (where the same hooks meet the same fallbacks on a real encoder output)."""
    from graphcast_lite_amd import functional as Fn
    from test_hip_model import data, make_pair

    monkeypatch.setenv("GCL_NO_ROW_SKIP", "1")  # (a dense gradient into the processor's output needs its dropped rows kept)
    cfg, m, _ = make_pair(name, [1, 2])
    B = 3
    X, y = data(cfg, m._num_grid_nodes, B)
    X, y = X.to(DEV), y.to(DEV)
    seen = {}

    def hooked(mod, key, seed):
        orig = mod.forward

        def fwd(*a, **k):
            out = orig(*a, **k)
            t = out[0] if isinstance(out, tuple) else out
            extra = rnd(*t.shape, seed=seed, scale=1e-3).to(DEV)
            seen[key] = seen.get(key, 0) + 1
            t.register_hook(lambda g: g + extra)
            return out

        mod.forward = fwd

    hooked(m.encoder.graph_layer, "enc", 5)
    hooked(m.processor, "proc", 6)
    (new, _, sp_new), (old, _, sp_old) = _both_ways(m, X, y, monkeypatch, counts)
    assert seen == {"enc": 4, "proc": 4} and sp_new == 2 and sp_old == 0
    zero = Fn._ZERO[torch.device(DEV)]
    assert zero.shape == () and float(zero) == 0.0
    _assert_equal_steps(new, old)
    # the hooks did reach the gradients: without them the encoder's differ
    del m.encoder.graph_layer.forward, m.processor.forward
    plain = _step(m, X, y)
    assert any(not torch.equal(plain[2][n_], g) for n_, g in new[2].items() if n_.startswith("encoder"))
