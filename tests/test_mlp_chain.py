"""The chained MLP forward (gcl_mlp_fwd_chain: the last two or three Linear layers of an MLP in one launch) against the
per-layer launches it replaces (GCL_MLP_CHAIN=0).  A layer runs the same code in both, so everything is compared with
torch.equal: every z_k, the output, the LayerNorm statistics, and through a whole model the loss and every gradient."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_CU = 256  # gcl::kNumCU: the chained kernel launches at most one block a CU, the per-layer kernel two


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def make_params(widths, has_ln, seed=0, device=DEV):
    """[W1, b1, a1, ..., WL, bL] (+ [gamma, beta]) of MLPFn, the PReLU slopes distinct."""
    g = torch.Generator().manual_seed(seed)
    params = []
    L = len(widths) - 1
    for k in range(L):
        params += [torch.randn(widths[k + 1], widths[k], generator=g) * 0.3, torch.randn(widths[k + 1], generator=g)]
        if k < L - 1:
            params.append(torch.tensor([0.25 - 0.1 * k]))
    if has_ln:
        params += [1 + 0.1 * torch.randn(widths[-1], generator=g), 0.1 * torch.randn(widths[-1], generator=g)]
    return [p.to(device) for p in params]


def run_mlp(x, params, has_ln):
    """MLPFn.forward on a stand-in ctx: (output, [z_k], LayerNorm statistics or None)."""
    from graphcast_lite_amd.functional import MLPFn

    ctx = types.SimpleNamespace()
    out = MLPFn.forward(ctx, x, None, has_ln, 1e-5, *params)
    torch.cuda.synchronize()
    return out, ctx.zs, ctx.stats


def both_paths(monkeypatch, x, params, has_ln):
    monkeypatch.setenv("GCL_MLP_CHAIN", "0")
    ref = run_mlp(x, params, has_ln)
    monkeypatch.delenv("GCL_MLP_CHAIN")
    return ref, run_mlp(x, params, has_ln)


def same(a, b, equal_nan=False):
    if equal_nan:
        return a.shape == b.shape and torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)
    return torch.equal(a, b)


def assert_same_run(ref, got, equal_nan=False):
    (o1, z1, s1), (o2, z2, s2) = ref, got
    assert len(z1) == len(z2)
    for k, (a, b) in enumerate(zip(z1, z2)):
        assert same(a, b, equal_nan), f"z_{k} differs"
    assert same(o1, o2, equal_nan), "output differs"
    assert (s1 is None) == (s2 is None)
    if s1 is not None:
        assert same(s1, s2, equal_nan), "LayerNorm statistics differ"


def chain_ok(hip, x, widths, act0=0, ln=False):
    """gcl_mlp_fwd_chain_ok for the layers widths[0] -> widths[1] -> .. (-> LayerNorm) on fresh contiguous outputs."""
    n = len(widths) - 1
    zs = [torch.empty(x.shape[0], w, device=x.device) for w in widths[1:]]
    args = []
    for k in range(3):
        args += [zs[k].data_ptr(), widths[k + 1], widths[k + 1]] if k < n else [None, 0, 0]
    ln_args = [None, None, 0, None]
    if ln:
        y, stats = torch.empty_like(zs[-1]), torch.empty(x.shape[0], 2, device=x.device)
        ln_args = [y.data_ptr(), y.data_ptr(), widths[-1], stats.data_ptr()]
    return hip.lib().gcl_mlp_fwd_chain_ok(x.data_ptr(), x.stride(0), x.shape[0], widths[0], act0, n, *args, *ln_args)


# (the last one: the LayerNorm epilogue on rows narrower than the 64-column tile)
CHAINS = [((64, 64, 64, 64), False), ((48, 48, 64), True), ((64, 48, 36), False), ((64, 64, 36), True)]
# 7 rows; one full 128-row tile plus a tile with wave 0 full, 5 rows in wave 1 and none in waves 2-3; more tiles than
# twice the per-layer grid, so a block of either kernel walks several tiles and the prefetch hands over
ROWS = [7, 165, 2 * NUM_CU * 128 + 165]


@pytest.mark.parametrize("widths,has_ln", CHAINS)
@pytest.mark.parametrize("rows", ROWS)
def test_chain_equals_per_layer(hip, monkeypatch, widths, has_ln, rows):
    x = torch.randn(rows, widths[0], generator=torch.Generator().manual_seed(rows)).to(DEV)
    params = make_params(widths, has_ln, seed=1)
    assert chain_ok(hip, x, widths) == 1 and chain_ok(hip, x, widths, ln=True) == (1 if len(widths) == 3 else 0)
    assert_same_run(*both_paths(monkeypatch, x, params, has_ln))


@pytest.mark.parametrize("widths,has_ln", CHAINS)
def test_chain_on_a_strided_input(hip, monkeypatch, widths, has_ln):
    """The first layer reads a column block of a wider tensor (ldx > K)."""
    wide = torch.randn(1000, widths[0] + 12, generator=torch.Generator().manual_seed(3)).to(DEV)
    x = wide[:, 4: 4 + widths[0]]
    assert x.stride(0) > widths[0] and chain_ok(hip, x, widths) == 1
    params = make_params(widths, has_ln, seed=2)
    ref, got = both_paths(monkeypatch, x, params, has_ln)
    assert_same_run(ref, got)
    assert_same_run(ref, run_mlp(x.contiguous(), params, has_ln))


def test_chain_exact_on_integers(hip):
    """Small integers (and PReLU slopes that are powers of two) make every product and partial sum exact, so the chain
    must give the float64 evaluation bit for bit: a row or a column that the hand-off between layers misplaces shows
    up as a wrong number."""
    g = torch.Generator().manual_seed(5)
    widths = (64, 64, 48, 64)
    rows = 1000
    x = torch.randint(-3, 4, (rows, widths[0]), generator=g).float()
    Ws = [torch.randint(-2, 3, (widths[k + 1], widths[k]), generator=g).float() for k in range(3)]
    bs = [torch.randint(-3, 4, (widths[k + 1],), generator=g).float() for k in range(3)]
    slopes = [torch.tensor([0.5]), torch.tensor([0.25])]
    refs, cur = [], x.double()
    for k in range(3):
        if k:
            cur = torch.where(cur > 0, cur, cur * slopes[k - 1].double())
        # what "exact" needs: operands of at most 16 bits (no third piece), sums of magnitudes below 2^24 (units of 1/8)
        assert float(cur.abs().max()) * 8 < 2 ** 16
        assert float((cur.abs() @ Ws[k].double().abs().t() + bs[k].double().abs()).max()) * 8 < 2 ** 24
        cur = cur @ Ws[k].double().t() + bs[k].double()
        refs.append(cur)
    got = hip.mlp_fwd_chain(x.to(DEV), [W.to(DEV) for W in Ws], [b.to(DEV) for b in bs], [s.to(DEV) for s in slopes])
    assert got is not None, "the chained kernel must take this run"
    zs = got[0]
    for k in range(3):
        assert torch.equal(zs[k].cpu().double(), refs[k]), f"z_{k} is not exact"


@pytest.mark.parametrize("widths,has_ln", CHAINS)
def test_a_nan_row_stays_one_row(hip, monkeypatch, widths, has_ln):
    rows, bad = 300, 171
    x = torch.randn(rows, widths[0], generator=torch.Generator().manual_seed(9))
    x[bad, 5] = float("nan")
    x = x.to(DEV)
    params = make_params(widths, has_ln, seed=4)
    ref, got = both_paths(monkeypatch, x, params, has_ln)
    assert_same_run(ref, got, equal_nan=True)
    for z in got[1] + [got[0]]:
        nan_rows = torch.isnan(z).any(dim=1).nonzero().flatten().tolist()
        assert nan_rows == [bad] and bool(torch.isnan(z[bad]).all())


def test_fallbacks(hip, monkeypatch):
    rows = 500
    x64 = torch.randn(rows, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    x72 = torch.randn(rows, 72, generator=torch.Generator().manual_seed(2)).to(DEV)
    # a 72-wide first layer: not chained as a whole, the two layers behind it are
    assert chain_ok(hip, x72, (72, 48, 48, 64)) == 0
    assert chain_ok(hip, x64[:, :48].contiguous(), (48, 48, 64), act0=hip.ACT_PRELU, ln=True) == 1
    assert_same_run(*both_paths(monkeypatch, x72, make_params((72, 48, 48, 64), True, seed=6), True))
    # SiLU in front of the run, an inner width of 33, widths outside 33..64
    assert chain_ok(hip, x64, (64, 64, 64), act0=hip.ACT_SILU) == 0
    assert chain_ok(hip, x64, (64, 33, 64)) == 0
    assert chain_ok(hip, x64, (64, 128, 64)) == 0
    assert chain_ok(hip, x64, (64, 32, 64)) == 0
    for widths in ((64, 33, 64), (64, 32, 64)):
        assert_same_run(*both_paths(monkeypatch, x64, make_params(widths, False, seed=7), False))
    # three layers and a LayerNorm: the layers are chained, the LayerNorm is a launch of its own
    assert chain_ok(hip, x64, (64, 64, 64, 64), ln=True) == 0 and chain_ok(hip, x64, (64, 64, 64, 64)) == 1
    assert_same_run(*both_paths(monkeypatch, x64, make_params((64, 64, 64, 64), True, seed=9), True))
    # the switches, read per call
    monkeypatch.setenv("GCL_X3", "0")
    assert chain_ok(hip, x64, (64, 64, 64)) == 0
    off = run_mlp(x64, make_params((64, 64, 64), False, seed=8), False)
    monkeypatch.delenv("GCL_X3")
    monkeypatch.setenv("GCL_MLP_CHAIN", "0")
    assert chain_ok(hip, x64, (64, 64, 64)) == 0
    monkeypatch.delenv("GCL_MLP_CHAIN")
    assert chain_ok(hip, x64, (64, 64, 64)) == 1
    on = run_mlp(x64, make_params((64, 64, 64), False, seed=8), False)
    for a, b in zip(off[1], on[1]):  # GCL_X3=0 is the fp32-operand kernel: the same numbers to fp32 accuracy, not bits
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def _model_and_data(B=2):
    import numpy as np

    from conftest import experiment
    from graphcast_lite_amd.models import WeatherPrediction

    cfg = experiment("baseline", mesh_levels=[1, 2])
    torch.manual_seed(42)
    lats, lons = np.linspace(-90, 90, 32, endpoint=True), np.linspace(0, 360, 64, endpoint=False)
    m = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, torch.device(DEV))
    g = torch.Generator().manual_seed(1234)
    F, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    X = torch.randn(B, m._num_grid_nodes, obs * F, generator=g)
    y = X[..., (obs - 1) * F:] + 0.1 * torch.randn(B, m._num_grid_nodes, F, generator=g)
    return m, X.to(DEV), y.to(DEV)


def test_whole_model_forward_backward(monkeypatch):
    from graphcast_lite_amd.train import batch_loss, get_lat_weights

    lw = get_lat_weights(32, 64, DEV)
    runs = []
    for off in (True, False):
        if off:
            monkeypatch.setenv("GCL_MLP_CHAIN", "0")
        else:
            monkeypatch.delenv("GCL_MLP_CHAIN")
        m, X, y = _model_and_data()
        loss = batch_loss(m, X, y, lat_weights=lw)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys()
    for n, g in runs[0][1].items():
        assert torch.equal(g, runs[1][1][n]), n


def test_whole_model_captured_step(monkeypatch):
    from graphcast_lite_amd.train import TrainStep, get_lat_weights

    lw = get_lat_weights(32, 64, DEV)
    runs = []
    for off in (True, False):
        if off:
            monkeypatch.setenv("GCL_MLP_CHAIN", "0")
        else:
            monkeypatch.delenv("GCL_MLP_CHAIN")
        m, X, y = _model_and_data()
        step = TrainStep(m, lr=1e-3, lat_weights=lw, use_graph=True)
        # two eager warm-up calls, the call that captures, two replays
        losses = [step(X * (1 + 0.01 * i), y).detach().clone() for i in range(5)]
        torch.cuda.synchronize()
        assert step.use_graph and step._graph is not None
        runs.append((losses, {n: p.detach().clone() for n, p in m.named_parameters()}))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for n, p in runs[0][1].items():
        assert torch.equal(p, runs[1][1][n]), n
