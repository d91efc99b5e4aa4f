"""Rows with more than 64 edges are summed by one block each - as the first blocks of the per-edge aggregation's own
launch (agg_kernel<.., HV>) instead of a second launch behind it (GCL_AGG_HEAVY_SEPARATE=1: the second launch).  Both
run one text (agg_heavy_row: the same lane-group stride over the edges, the same fixed-order combine), so the results
are compared with torch.equal; gcl_aggregate_heavy_launches counts the separate launches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N, HEAD = 203, 37


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ("GCL_AGG_HEAVY_SEPARATE", "GCL_AGG_ITER", "GCL_AGG_EW"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GCL_AGG_HALO", "0")  # the per-edge kernel is the subject (the source-tile one keeps the second launch)


def rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.fixture(scope="module")
def heavy_graph(hip):
    """Bipartite-plus-self-loops graph on 203 rows (a ragged last block) in which row 100 has 70 in-edges and row 20 has
    70 out-edges: a heavy row in either direction of the call."""
    rng = np.random.default_rng(5)
    a = rng.integers(0, HEAD, 500)
    b = rng.integers(HEAD, N, 500)
    heavy_in = np.stack([rng.choice(np.setdiff1d(np.arange(N), [100]), 70, replace=False), np.full(70, 100)])
    heavy_out = np.stack([np.full(70, 20), rng.choice(np.setdiff1d(np.arange(N), [20]), 70, replace=False)])
    ei = torch.unique(torch.from_numpy(np.concatenate([np.stack([a, b]), np.stack([b[:300], a[:300]]), heavy_in, heavy_out], 1)),
                      dim=1)
    G = hip.Graph(ei, N, hip.GRAPH_GCN)
    assert G.max_in_degree > 64
    return G


def _run(hip, G, kind, h, tr, B, F):
    """One aggregation into a view of a NaN-filled tensor -> (result, padding still NaN?, separate heavy launches)."""
    big = torch.full((B, N + 4, F + 8), NAN, device=DEV)
    out = big[:, 2: 2 + N, 4: 4 + F]
    before = hip.aggregate_heavy_launches()
    if kind == "plain":
        hip.aggregate(G, h, None, transpose=tr, out=out)
    elif kind == "present":
        present = torch.arange(N, dtype=torch.int32)
        present[3::5] = -1  # absent sources: among them sources of both heavy rows
        hsrc = h.clone()
        hsrc[:, 3::5] = NAN  # ... which must never be read
        hip.aggregate_present(G, hsrc, present.to(DEV), transpose=tr, out=out)
    else:
        big_a = torch.full((B, HEAD + 5, F + 8), NAN, device=DEV)
        big_a[:, 2: 2 + HEAD, 4: 4 + F] = h[:, :HEAD]
        big_b = torch.full((B, N - HEAD + 3, F), NAN, device=DEV)
        big_b[:, 1: 1 + N - HEAD] = h[:, HEAD:]
        hip.aggregate_split(G, big_a[:, 2: 2 + HEAD, 4: 4 + F], big_b[:, 1: 1 + N - HEAD], transpose=tr, out=out)
    torch.cuda.synchronize()
    launches = hip.aggregate_heavy_launches() - before
    res = out.clone()
    big[:, 2: 2 + N, 4: 4 + F] = NAN
    return res, bool(torch.isnan(big).all()), launches


@pytest.mark.parametrize("kind", ["plain", "present", "split"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [64, 48, 36])
@pytest.mark.parametrize("tr", [False, True])
def test_heavy_rows_inside_the_main_launch(hip, heavy_graph, monkeypatch, tr, F, B, kind):
    h = rnd(B, N, F, seed=7 + F + B).to(DEV)
    one, pad_one, l_one = _run(hip, heavy_graph, kind, h, tr, B, F)
    monkeypatch.setenv("GCL_AGG_HEAVY_SEPARATE", "1")
    two, pad_two, l_two = _run(hip, heavy_graph, kind, h, tr, B, F)
    assert l_one == 0, "the heavy rows ran in a launch of their own"
    assert l_two == 1, "the switch did not restore the second launch"
    assert bool(torch.isfinite(one).all()) and torch.equal(one, two)
    assert pad_one and pad_two, "something outside the output view was written"
    # the heavy row's sum is really there (70 terms: not the zero a skipped row would leave in a zero-filled output)
    row = 20 if tr else 100
    assert float(one[:, row].abs().max()) > 0
