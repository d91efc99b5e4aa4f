"""The loss gradient handed to the decoder's backward where it was born: ARStepLossFn writes d loss / d pred in the padded
row layout of delta, returns it without a launch when the upstream gradient is the constant one of const_one, and
GCNStackFn.backward reads it in place (gcl_aggregate_head + a strided colsum) instead of widening it with gcl_pad_rows.
GCL_NO_LOSS_GRAD_INPLACE=1 is the path before: every gradient must be torch.equal between the two."""
import types

import numpy as np
import pytest
import torch

from helpers.layouts import has, launched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, HEAD, B, C, D = 303, 101, 3, 33, 64
SWITCH = "GCL_NO_LOSS_GRAD_INPLACE"


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    monkeypatch.delenv(SWITCH, raising=False)


@pytest.fixture(scope="module")
def case(hip):
    """A decoder-shaped stack: 2 GCNConvs (64 -> 64 -> 33) on a bipartite graph with a heavy row, of which the first
    HEAD rows are returned; a 2-slot window, targets for two steps and loss weights."""
    rng = np.random.default_rng(11)
    a = rng.integers(0, HEAD, 800)
    b = rng.integers(HEAD, N, 800)
    heavy_in = np.stack([rng.choice(np.setdiff1d(np.arange(N), [200]), 70, replace=False), np.full(70, 200)])
    heavy_out = np.stack([np.full(70, 20), rng.choice(np.setdiff1d(np.arange(N), [20]), 70, replace=False)])
    ei = torch.unique(torch.from_numpy(np.concatenate([np.stack([a, b]), np.stack([b[:500], a[:500]]), heavy_in, heavy_out], 1)),
                      dim=1)
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)  # noqa: E731
    return types.SimpleNamespace(
        graph=hip.Graph(ei, N, hip.GRAPH_GCN), x=r(B, N, D), params=[r(D, D) / 8, r(D) / 4, r(C, D) / 8, r(C) / 4, torch.tensor([0.25]).to(DEV)],
        state=r(B, HEAD, 2, C), y=r(B, HEAD, 2, C), node_w=torch.rand(HEAD, generator=g).to(DEV) + 0.5,
        chan_w=torch.rand(C, generator=g).to(DEV) + 0.5, kinds=(torch.arange(C) % 3).to(torch.int32).to(DEV), owner=types.SimpleNamespace())


def _leaves(case):
    x = case.x.clone().requires_grad_(True)
    params = [p.clone().requires_grad_(True) for p in case.params]
    return x, params


def _stack(case, x, params):
    from graphcast_lite_amd.functional import GCNStackFn

    return GCNStackFn.apply(x, case.owner, case.graph, 2, False, 1e-5, HEAD, None, None, None, *params)


def _loss(case, delta, s=0, state=None, prev=None, advance=False, y=None):
    from graphcast_lite_amd.functional import ARStepLossFn

    y = case.y if y is None else y
    return ARStepLossFn.apply(case.state if state is None else state, delta, y[:, :, s, :], prev, case.node_w, case.chan_w,
                              0.01, case.kinds if (advance or prev is not None) else None, True, advance)


def _run(case, mode, dy_of=None):
    """One forward + backward -> [d x, d params...]."""
    from graphcast_lite_amd.functional import const_one

    x, params = _leaves(case)
    delta = _stack(case, x, params)
    if mode == "dy":  # a gradient of delta handed in from outside
        delta.backward(dy_of(delta))
    elif mode == "two_steps":
        l1, st1 = _loss(case, delta, 0, advance=True)
        x2 = x + torch.nn.functional.pad(st1.reshape(B, HEAD, 2 * C)[..., :D], (0, 0, 0, N - HEAD))
        l2, _ = _loss(case, _stack(case, x2, params), 1, state=st1, prev=l1)
        l2.backward(const_one(l2))
    elif mode == "two_losses":
        la, _ = _loss(case, delta)
        lb, _ = _loss(case, delta, y=case.y.flip(0))
        (la + lb).backward(const_one(la))
    else:
        loss, _ = _loss(case, delta)
        if mode == "one":
            loss.backward(const_one(loss))
        elif mode == "plain":
            loss.backward()
        else:
            (2 * loss).backward()
    torch.cuda.synchronize()
    grads = [x.grad] + [p.grad for p in params]
    assert all(t is not None and bool(torch.isfinite(t).all()) for t in grads)
    return grads


def _both(case, monkeypatch, mode, dy_of=None):
    new, names = launched(lambda: _run(case, mode, dy_of))
    monkeypatch.setenv(SWITCH, "1")
    old, names_old = launched(lambda: _run(case, mode, dy_of))
    monkeypatch.delenv(SWITCH)
    for k, (a, b) in enumerate(zip(new, old)):
        assert torch.equal(a, b), f"{mode}: gradient {k} differs from the {SWITCH}=1 path"
    assert has(names_old, "pad_rows_kernel"), "the switch did not restore the widening pass"
    if mode != "dy":
        assert has(names_old, "ar_step_bwd_kernel") and has(names_old, "wmse_kernel<false>")
    return names


def test_constant_one_root_launches_neither_pass(case, monkeypatch):
    names = _both(case, monkeypatch, "one")
    assert not has(names, "pad_rows_kernel") and not has(names, "ar_step_bwd")
    assert has(names, "wmse_kernel<true>")


@pytest.mark.parametrize("mode", ["plain", "scaled", "two_steps"])
def test_other_upstream_gradients_take_the_strided_fallback(case, monkeypatch, mode):
    names = _both(case, monkeypatch, mode)
    assert has(names, "ar_step_bwd_ld_kernel") and not has(names, "ar_step_bwd_kernel") and not has(names, "pad_rows_kernel")


def test_two_losses_on_one_delta_give_the_sum(case, monkeypatch):
    names = _both(case, monkeypatch, "two_losses")
    assert has(names, "pad_rows_kernel")  # autograd's sum of the two gradients is dense: the path before takes it


def _short(delta):
    """33-wide rows 36 apart in a buffer that ends with the last row's 33rd float: 12 bytes short of B * G * 36."""
    Bn, Gn, Cn = delta.shape
    buf = torch.randn((Bn * Gn - 1) * 36 + Cn, generator=torch.Generator().manual_seed(5)).to(DEV)
    return torch.as_strided(buf, (Bn, Gn, Cn), (Gn * 36, 36, 1), 0)


def _other_batch_stride(delta):
    Bn, Gn, Cn = delta.shape
    buf = torch.randn(Bn, Gn + 1, 36, generator=torch.Generator().manual_seed(6)).to(DEV)
    return buf[:, :Gn, :Cn]


def _whole(delta):
    Bn, Gn, Cn = delta.shape
    buf = torch.randn(Bn, Gn, 36, generator=torch.Generator().manual_seed(7)).to(DEV)
    buf[..., Cn:] = 0
    return buf[..., :Cn]


@pytest.mark.parametrize("dy_of", [_short, _other_batch_stride], ids=["storage_ends_early", "other_batch_stride"])
def test_a_gradient_that_fails_the_storage_rule_is_widened_as_before(case, monkeypatch, dy_of):
    names = _both(case, monkeypatch, "dy", dy_of)
    assert has(names, "pad_rows_kernel")


def test_a_foreign_gradient_in_the_padded_layout_is_read_in_place(case, monkeypatch):
    names = _both(case, monkeypatch, "dy", _whole)
    assert not has(names, "pad_rows_kernel")
