"""The loss gradient in a caller-given row layout: gcl_wmse_fwd_bwd_ld writes d loss / d pred with a row stride (padding
columns zero) and gcl_ar_step_bwd_ld reads and writes that layout.  Both keep the thread-to-element map, the sums and
their order of the dense entries, so everything is compared with torch.equal against hip.wmse_fwd_bwd / hip.ar_step_bwd
on contiguous tensors."""
import itertools

import pytest
import torch

from helpers.layouts import NAN, SENT, Guarded, Rows, rand, randn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, G = 3, 37


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def _pad4(c):
    return (c + 3) // 4 * 4


def _operands(Bn, Gn, C, seed):
    """delta with rows roundup4(C) apart (NaN padding), x_last = last slot of a [B, G, 2, C] window, y a strided slice."""
    delta = Rows.of(randn(Bn, Gn, C, seed=seed), "tight", NAN).view
    state = randn(Bn, Gn, 2, C, seed=seed + 1)
    ybig = randn(Bn, Gn, 2, C + 3, seed=seed + 2)
    return delta, state[:, :, 1, :], ybig[:, :, 1, 1:1 + C]


def _wmse_ld(hip, delta, xl, y, node_w, chan_w, inv, loss_prev, ldo):
    """gcl_wmse_fwd_bwd_ld into a [B, G, ldo] tensor with a sentinel frame -> (loss, that tensor, frame untouched?)."""
    Bn, Gn, C = delta.shape
    out = Guarded((Bn, Gn, ldo))
    out.view.fill_(SENT)
    loss = torch.empty((), device=DEV)
    ws = hip.workspace(hip.lib().gcl_wmse_ws_bytes(Bn, Gn, C), delta.device)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = hip.lib().gcl_wmse_fwd_bwd_ld(
        p(delta), delta.stride(1), delta.stride(0), p(xl), xl.stride(1), xl.stride(0), p(y), y.stride(1), y.stride(0),
        p(node_w), p(chan_w), float(inv), 1.0, p(out.view), ldo, Gn * ldo, None, p(loss_prev), p(loss), Bn, Gn, C,
        ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return loss, out.view, out.untouched()


@pytest.mark.parametrize("C", [33, 19, 4, 1])
def test_wmse_ld_matches_the_dense_entry(hip, C):
    delta, xl, y = _operands(B, G, C, seed=10 + C)
    nw, cw = rand(G, seed=3) + 0.5, rand(C, seed=4) + 0.5
    prev = torch.tensor(0.375, device=DEV)
    for ldo, use_nw, use_cw, use_prev in itertools.product(sorted({C, _pad4(C)}), [True, False], [True, False], [True, False]):
        a = (nw if use_nw else None, cw if use_cw else None, 0.013)
        lp = prev if use_prev else None
        loss_ref, dd_ref, _ = hip.wmse_fwd_bwd(delta, xl, y, a[0], a[1], a[2], 1.0, loss_prev=lp)
        loss, full, framed = _wmse_ld(hip, delta, xl, y, a[0], a[1], a[2], lp, ldo)
        what = f"C={C} ldd_out={ldo} node_w={use_nw} chan_w={use_cw} loss_prev={use_prev}"
        assert torch.equal(loss, loss_ref), what
        assert bool(torch.isfinite(dd_ref).all()) and torch.equal(full[..., :C], dd_ref), what
        assert bool((full[..., C:] == 0).all()), f"{what}: padding columns not zero"
        assert framed, f"{what}: written outside the output"


def test_wmse_ld_wrapper_returns_the_padded_view(hip):
    C = 33
    delta, xl, y = _operands(B, G, C, seed=77)
    loss_ref, dd_ref, _ = hip.wmse_fwd_bwd(delta, xl, y, None, None, 0.02, 1.0)
    loss, dd, _ = hip.wmse_fwd_bwd(delta, xl, y, None, None, 0.02, 1.0, ldd_out=36)
    assert dd.shape == (B, G, C) and dd.stride() == (G * 36, 36, 1) and dd.untyped_storage().nbytes() == B * G * 36 * 4
    assert torch.equal(loss, loss_ref) and torch.equal(dd, dd_ref)


def test_wmse_ld_grid_stride_loop_runs_twice(hip):
    """More than 1024 blocks x 256 threads x 4 elements: every thread owns elements of two trips."""
    Bn, Gn, C = 9, 4099, 33
    assert Bn * Gn * C > 1024 * 256 * 4
    delta, xl, y = _operands(Bn, Gn, C, seed=5)
    nw, cw = rand(Gn, seed=6) + 0.5, rand(C, seed=7) + 0.5
    loss_ref, dd_ref, _ = hip.wmse_fwd_bwd(delta, xl, y, nw, cw, 1e-4, 1.0)
    loss, full, framed = _wmse_ld(hip, delta, xl, y, nw, cw, 1e-4, None, 36)
    assert torch.equal(loss, loss_ref) and torch.equal(full[..., :C], dd_ref)
    assert bool((full[..., C:] == 0).all()) and framed


@pytest.mark.parametrize("C", [33, 4])
@pytest.mark.parametrize("obs", [1, 2])
def test_ar_step_bwd_with_row_strides(hip, obs, C):
    ldp = _pad4(C) if C % 4 else C + 4
    dd = randn(B, G, C, seed=20 + C)
    wide = torch.full((B, G, ldp), NAN, device=DEV)
    wide[..., :C] = dd
    g_loss = torch.tensor(0.7, device=DEV)
    kinds = (torch.arange(C, device=DEV) % 3).to(torch.int32)
    for with_new, with_state, has_y, residual in itertools.product([False, True], [False, True], [False, True], [False, True]):
        g_new = randn(B, G, obs, C, seed=31) if with_new else None
        ref_d, ref_s = hip.ar_step_bwd(dd, g_loss, g_new, kinds, has_y, residual, obs, with_state)
        got_d, got_s = hip.ar_step_bwd(wide[..., :C], g_loss, g_new, kinds, has_y, residual, obs, with_state, ldd_out=ldp)
        what = f"obs={obs} C={C} g_new={with_new} d_state={with_state} has_y={has_y} residual={residual}"
        assert got_d.stride() == (G * ldp, ldp, 1), what
        assert torch.equal(got_d, ref_d), what
        full = torch.as_strided(got_d, (B, G, ldp), (G * ldp, ldp, 1), got_d.storage_offset())
        assert bool((full[..., C:] == 0).all()), f"{what}: padding columns not zero"
        assert (got_s is None) == (ref_s is None) and (ref_s is None or torch.equal(got_s, ref_s)), what
