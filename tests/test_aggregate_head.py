"""gcl_aggregate_head: the aggregation over a source whose rows >= head are zeros that exist nowhere (the gradient of a
layer that returned only its first rows).  It runs agg_kernel<.., SPLIT> with the library's own zero row as the second
part, so the result is compared with torch.equal against hip.aggregate on the pad_rows-widened source - the adds of
w * 0 are performed on both sides."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
N, HEAD, B = 303, 101, 3


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in ("GCL_AGG_HEAVY_SEPARATE", "GCL_AGG_ITER", "GCL_AGG_EW", "GCL_AGG_HALO"):
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module")
def graph(hip):
    """Bipartite graph (head rows <-> the rest) on 303 rows - a ragged last block - in which row 200 has 70 in-edges and
    row 20 has 70 out-edges: a heavy row in either direction, fed from both sides of `head`."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, HEAD, 800)
    b = rng.integers(HEAD, N, 800)
    heavy_in = np.stack([rng.choice(np.setdiff1d(np.arange(N), [200]), 70, replace=False), np.full(70, 200)])
    heavy_out = np.stack([np.full(70, 20), rng.choice(np.setdiff1d(np.arange(N), [20]), 70, replace=False)])
    ei = torch.unique(torch.from_numpy(np.concatenate([np.stack([a, b]), np.stack([b[:500], a[:500]]), heavy_in, heavy_out], 1)),
                      dim=1)
    G = hip.Graph(ei, N, hip.GRAPH_GCN)
    assert G.max_in_degree > 64
    return G


@pytest.mark.parametrize("F", [36, 20])
@pytest.mark.parametrize("tr", [False, True])
def test_head_rows_and_a_zero_tail(hip, graph, tr, F):
    h = torch.randn(B, HEAD, F, generator=torch.Generator().manual_seed(3 + F)).to(DEV)
    ref = hip.aggregate(graph, hip.pad_rows(h, N, F), None, transpose=tr)
    # the head rows as a view of a NaN-filled tensor: neither their padding nor anything behind row `head` is read
    src = torch.full((B, HEAD + 6, F + 8), NAN, device=DEV)
    src[:, 1:1 + HEAD, 4:4 + F] = h
    big = torch.full((B, N + 4, F + 8), NAN, device=DEV)
    out = big[:, 2:2 + N, 4:4 + F]
    before = hip.aggregate_heavy_launches()
    hip.aggregate_head(graph, src[:, 1:1 + HEAD, 4:4 + F], transpose=tr, out=out)
    torch.cuda.synchronize()
    assert hip.aggregate_heavy_launches() == before, "the heavy rows ran in a launch of their own"
    got = out.clone()
    assert bool(torch.isfinite(got).all()) and torch.equal(got, ref)
    big[:, 2:2 + N, 4:4 + F] = NAN
    assert bool(torch.isnan(big).all()), "something outside the output view was written"
    row = 20 if tr else 200
    assert float(got[:, row].abs().max()) > 0  # the heavy row's sum is really there


def test_head_equal_to_n_is_the_plain_aggregation(hip, graph):
    h = torch.randn(B, N, 36, generator=torch.Generator().manual_seed(9)).to(DEV)
    assert torch.equal(hip.aggregate_head(graph, h, transpose=True), hip.aggregate(graph, h, None, transpose=True))


def test_bad_layouts_are_refused(hip, graph):
    h = torch.zeros(B, HEAD, 36, device=DEV)
    with pytest.raises(Exception):
        hip.aggregate_head(graph, h[..., :33], transpose=True, out=torch.empty(B, N, 33, device=DEV))  # F % 4 != 0
    with pytest.raises(Exception):
        hip.aggregate_head(graph, torch.zeros(B, N + 1, 36, device=DEV), transpose=True)  # head > n
