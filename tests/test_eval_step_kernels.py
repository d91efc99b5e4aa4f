"""Contract of `gcl_eval_colstats` / `gcl_eval_accumulate` (csrc/eval_step.hip) as include/gcl.h states it, against a
restatement in numpy (sums in extended precision, rounded to float64) on the same float32 prediction.

Bounds, from the number formats: every term of a sum is formed in float64 from float32 data (relative error about
1e-16 per term) and a sum of G <= 2051 such terms in any fixed order keeps a relative error far below 1e-12, the bar
for each of the seven sums (the signed sums lose the factor sum |t| / |sum t| to cancellation: a few hundred at most on
these inputs); the three scores are a few hundred float64 operations on those sums: 1e-10."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# G below, across and well beyond one 64-row chunk; 197: a last chunk of 5 rows, fewer than the 8 row lanes; 32835: 506
# chunks of 65 rows, more than one pass of the 64-lane combine
SHAPES = [(1, 2, 1), (2, 48, 5), (3, 203, 33), (2, 2051, 19), (2, 197, 19), (2, 32835, 3)]
LD = np.longdouble


def _case(B, G, C, seed, kinds_on, node_on, chan_on):
    """Inputs as the evaluator passes them: x_last the last slot of a [B, G, 3C] window, y step 0 of [B, G, 2C]."""
    g = torch.Generator().manual_seed(seed)
    Xw = torch.randn(B, G, 3 * C, generator=g)
    Yw = Xw[..., 2 * C:].repeat(1, 1, 2) + 0.3 * torch.randn(B, G, 2 * C, generator=g)
    Dw = 0.2 * torch.randn(B, G, C + 3, generator=g)
    kinds = torch.zeros(C, dtype=torch.int32)
    if kinds_on == "some":
        kinds[1::3], kinds[2::3] = 1, 2
    elif kinds_on == "all":  # every channel static or forcing: the ACC keeps all of them
        kinds[:] = 1 + torch.arange(C, dtype=torch.int32) % 2
    node_w = chan_w = None
    if node_on:
        node_w = torch.rand(G, generator=g) + 0.5
        node_w[::3] = 0.0
    if chan_on:
        chan_w = torch.rand(C, generator=g) + 0.5
        chan_w[::2] = 0.0
    dev = lambda t: None if t is None else t.to(DEV)  # noqa: E731
    Xw, Yw, Dw = Xw.to(DEV), Yw.to(DEV), Dw.to(DEV)
    return dict(X=Xw, x_last=Xw.view(B, G, 3, C)[:, :, 2, :], y=Yw[:, :, :C], delta=Dw[:, :, 1:C + 1], kinds=dev(kinds),
                node_w=dev(node_w), chan_w=dev(chan_w))


def _ref_o(c, residual):
    """The one-step prediction in float32, as gcl.h states it."""
    x, d, y = (c[k].cpu().numpy() for k in ("x_last", "delta", "y"))
    o = (x + d).astype(np.float32) if residual else d.copy()
    k = c["kinds"].cpu().numpy()
    o[..., k == 1] = x[..., k == 1]
    o[..., k == 2] = y[..., k == 2]
    return o


def _ref_stats(o, y, node_w):
    o, y = o.astype(LD), y.astype(LD)
    w = np.ones(o.shape[1], dtype=LD) if node_w is None else node_w.cpu().numpy().astype(LD)
    d2 = (o - y) ** 2
    op, yp = o - o[:, :1], y - y[:, :1]
    s = [d2.sum(1), (w[None, :, None] * d2).sum(1), op.sum(1), (op * op).sum(1), yp.sum(1), (yp * yp).sum(1), (op * yp).sum(1)]
    return np.stack(s, axis=-1).astype(np.float64)  # [B, C, 7]


def _ref_scores(stats, chan_w, kinds, inv_wsum, G):
    B, C, _ = stats.shape
    cw = np.ones(C) if chan_w is None else chan_w.cpu().numpy().astype(np.float64)
    keep = kinds.cpu().numpy() == 0
    if not keep.any():
        keep[:] = True
    loss = inv_wsum * float((cw[None, :] * stats[:, :, 1]).sum())
    raw = float(stats[:, :, 0].sum()) / (B * G * C)
    cov = (stats[..., 6] - stats[..., 2] * stats[..., 4] / G) / G
    so = np.sqrt(np.maximum(stats[..., 3] - stats[..., 2] ** 2 / G, 0) / (G - 1))
    sy = np.sqrt(np.maximum(stats[..., 5] - stats[..., 4] ** 2 / G, 0) / (G - 1))
    acc = float((cov / ((so + 1e-8) * (sy + 1e-8)))[:, keep].mean(1).mean())
    return loss, acc, raw


def _inv_wsum(c, B, G, C):
    sn = float(c["node_w"].double().sum()) if c["node_w"] is not None else float(G)
    sc = float(c["chan_w"].double().sum()) if c["chan_w"] is not None else float(C)
    return 1.0 / max(B * sn * sc, 1e-12)


def _close(got, want, rel):
    return np.all(np.abs(got - want) <= rel * np.abs(want))


@pytest.mark.parametrize("B,G,C", SHAPES)
def test_sums_and_scores_match_the_restatement(B, G, C, lib_built):
    from graphcast_lite_amd import hip

    worst_sum = worst_score = 0.0
    for n, (residual, node_on, chan_on, kinds_on) in enumerate(itertools.product((True, False), (False, True),
                                                                                 (False, True), ("none", "some", "all"))):
        c = _case(B, G, C, 100 * G + n, kinds_on, node_on, chan_on)
        stats = torch.full((B, C, 7), float("nan"), dtype=torch.float64, device=DEV)
        hip.eval_colstats(c["delta"], c["x_last"], c["y"], c["node_w"], c["kinds"], residual, stats)
        want = _ref_stats(_ref_o(c, residual), c["y"].cpu().numpy(), c["node_w"])
        got = stats.cpu().numpy()
        err = float((np.abs(got - want) / np.maximum(np.abs(want), 1e-300)).max())
        worst_sum = max(worst_sum, err)
        assert _close(got, want, 1e-12), (n, err)
        state = torch.zeros(4, dtype=torch.float64, device=DEV)
        inv = _inv_wsum(c, B, G, C)
        for _ in range(2):
            hip.eval_accumulate(stats, c["chan_w"], c["kinds"], inv, G, state)
        got_s = state.cpu().numpy()
        want_s = _ref_scores(want, c["chan_w"], c["kinds"], inv, G)
        assert got_s[3] == 2.0
        for a, b in zip(got_s[:3] / 2, want_s):
            worst_score = max(worst_score, abs(a - b) / max(1.0, abs(b)))
            assert abs(a - b) <= 1e-10 * max(1.0, abs(b)), (n, got_s, want_s)
    print(f"B={B} G={G} C={C}: worst relative error of a sum {worst_sum:.2e}, of a score {worst_score:.2e}")


@pytest.mark.parametrize("B,G,C", SHAPES)
@pytest.mark.parametrize("residual", [True, False])
def test_stored_prediction_has_ar_advance_bits(B, G, C, residual, lib_built):
    from graphcast_lite_amd import hip

    c = _case(B, G, C, 7 + G, "some", True, False)
    stats = torch.empty(B, C, 7, dtype=torch.float64, device=DEV)
    wide = torch.full((B + 1, G + 2, C + 5), -7.0, device=DEV)  # a padded, offset output
    out = wide[1:, 1:G + 1, 2:C + 2]
    hip.eval_colstats(c["delta"], c["x_last"], c["y"], c["node_w"], c["kinds"], residual, stats, out3=out)
    want = torch.empty(B, G, C, device=DEV)
    hip.ar_advance(c["X"].view(B, G, 3, C), c["delta"], c["y"], c["kinds"], want, 0, residual)
    assert torch.equal(out, want)
    assert np.array_equal(want.cpu().numpy(), _ref_o(c, residual))
    untouched = wide.clone()
    untouched[1:, 1:G + 1, 2:C + 2] = -7.0
    assert bool((untouched == -7.0).all())
    # the sums do not depend on whether the prediction is stored
    stats2 = torch.empty_like(stats)
    hip.eval_colstats(c["delta"], c["x_last"], c["y"], c["node_w"], c["kinds"], residual, stats2)
    assert torch.equal(stats, stats2)


def test_constant_column_has_exactly_zero_centred_sums(lib_built):
    """A prediction that is 0.1 at every node: the two-pass float64 value of its ACC term is about 1e-9 (rounding of
    the mean), the shifted one-pass sums are exactly 0."""
    from graphcast_lite_amd import hip

    B, G, C = 2, 203, 5
    c = _case(B, G, C, 3, "none", False, False)
    delta = c["delta"].contiguous()
    delta[:, :, 2] = 0.1
    stats = torch.empty(B, C, 7, dtype=torch.float64, device=DEV)
    hip.eval_colstats(delta, c["x_last"], c["y"], None, None, False, stats)
    s = stats.cpu().numpy()
    assert np.all(s[:, 2, [2, 3, 6]] == 0.0)
    cov = (s[:, 2, 6] - s[:, 2, 2] * s[:, 2, 4] / G) / G
    sy = np.sqrt(np.maximum(s[:, 2, 5] - s[:, 2, 4] ** 2 / G, 0) / (G - 1))
    term = cov / ((0.0 + 1e-8) * (sy + 1e-8))
    assert np.all(np.abs(term) <= 1e-6) and np.all(term == 0.0)
    # through the accumulate kernel: only that channel kept
    kinds = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32, device=DEV)
    state = torch.zeros(4, dtype=torch.float64, device=DEV)
    hip.eval_colstats(delta, c["x_last"], c["y"], None, None, False, stats)  # (kinds None: the column stays 0.1)
    hip.eval_accumulate(stats, None, kinds, 1.0, G, state)
    assert abs(float(state[1])) <= 1e-6


def test_two_runs_are_bit_equal_and_padding_stays(lib_built):
    from graphcast_lite_amd import hip

    B, G, C = 2, 2051, 19
    c = _case(B, G, C, 11, "some", True, True)
    pad, n = 13, B * C * 7
    bufs = [torch.full((n + 2 * pad,), -3.0, dtype=torch.float64, device=DEV) for _ in range(2)]
    states = []
    for buf in bufs:
        stats = buf[pad:pad + n].view(B, C, 7)
        hip.eval_colstats(c["delta"], c["x_last"], c["y"], c["node_w"], c["kinds"], True, stats)
        state = torch.zeros(4, dtype=torch.float64, device=DEV)
        hip.eval_accumulate(stats, c["chan_w"], c["kinds"], _inv_wsum(c, B, G, C), G, state)
        states.append(state)
        assert bool((buf[:pad] == -3.0).all()) and bool((buf[pad + n:] == -3.0).all())
        assert not bool((stats == -3.0).any())
    assert torch.equal(bufs[0], bufs[1]) and torch.equal(states[0], states[1])


def test_wrapper_rejects_what_the_kernel_cannot_address(lib_built):
    from graphcast_lite_amd import hip

    c = _case(2, 48, 5, 1, "none", False, False)
    stats = torch.empty(2, 5, 7, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError):
        hip.eval_colstats(c["delta"], c["x_last"][:1], c["y"], None, None, True, stats)
    with pytest.raises(ValueError):
        hip.eval_colstats(c["delta"], c["x_last"], c["y"], None, None, True, stats[:, :4])
    with pytest.raises(ValueError):
        hip.eval_colstats(c["delta"], c["x_last"], c["y"], torch.ones(47, device=DEV), None, True, stats)
    one = _case(1, 2, 1, 1, "none", False, False)
    with pytest.raises(RuntimeError, match="at least 2 nodes"):
        hip.eval_colstats(one["delta"][:, :1], one["x_last"][:, :1], one["y"][:, :1], None, None, True,
                          torch.empty(1, 1, 7, dtype=torch.float64, device=DEV))
