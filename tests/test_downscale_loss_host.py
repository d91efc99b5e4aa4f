"""The downscaler's objective and scores without a GPU (tests/golden/downscale_loss_vectors.npz, made by
tests/golden/make_downscale_loss_golden.py from the reference's own functions).

Rules:
  formulas     a float64 numpy restatement of masked_mse_loss, spectral_loss and gradient_loss and of their gradients
               with respect to the output, written here, equals the fixture's float64 values (the reference functions
               and torch autograd) to 1e-12 relative (E = max |x - ref| / max |ref|) on every case; the regenerated
               inputs have the digests the fixture recorded.
  validation   every unsupported operand raises before any GPU work (the tensors are on the CPU, no GPU is present).
  strings      the test table and the results.json keys against what the reference's main() logged and wrote.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import downscale_loss_case as LC  # noqa: E402

CASES = [(si, r, m) for si in range(len(LC.SHAPES)) for r in (0, 1) for m in (0, 1)]


@pytest.fixture(scope="module")
def D():
    from graphcast_lite_amd import downscale

    return downscale


@pytest.fixture(scope="module")
def gv():
    return LC.golden()


def restate(o, y, m):
    """(terms [3], gradients [3, B, C, H, W]) in float64: o, y [B, C, H, W], m [C]."""
    B, C, H, W = o.shape
    mc = m.reshape(1, C, 1, 1)
    e = o - y
    mse = (mc * e ** 2).sum() / e.size
    g_mse = 2.0 * mc * e / e.size
    dy, dx = e[:, :, 1:, :] - e[:, :, :-1, :], e[:, :, :, 1:] - e[:, :, :, :-1]
    ny, nx = B * C * (H - 1) * W, B * C * H * (W - 1)
    grad = (mc * dy ** 2).sum() / ny + (mc * dx ** 2).sum() / nx
    g_grad = np.zeros_like(e)
    g_grad[:, :, 1:, :] += 2.0 * mc * dy / ny
    g_grad[:, :, :-1, :] -= 2.0 * mc * dy / ny
    g_grad[:, :, :, 1:] += 2.0 * mc * dx / nx
    g_grad[:, :, :, :-1] -= 2.0 * mc * dx / nx
    KX = W // 2 + 1
    fh = np.exp(-2j * np.pi * np.outer(np.arange(H), np.arange(H)) / H)       # [ky, h]
    fw = np.exp(-2j * np.pi * np.outer(np.arange(W), np.arange(KX)) / W)      # [w, kx]
    s = 1.0 / np.sqrt(H * W)
    P = s * np.einsum("yh,bchw,wx->bcyx", fh, mc * o, fw)
    T = s * np.einsum("yh,bchw,wx->bcyx", fh, mc * y, fw)
    aP, aT = np.abs(P), np.abs(T)
    count = B * C * H * KX
    spec = np.abs(aP - aT).sum() / count
    G = np.where(aP > 0, np.sign(aP - aT) * P / np.where(aP > 0, aP, 1.0), 0.0) / count
    g_spec = mc * s * np.real(np.einsum("yh,bcyx,wx->bchw", fh.conj(), G, fw.conj()))
    return np.array([mse, spec, grad]), np.stack([g_mse, g_spec, g_grad])


@pytest.mark.parametrize("case", CASES, ids=lambda c: LC.case_key(*c))
def test_float64_restatement_equals_the_reference(gv, case):
    si, r, m = case
    out, Y, x_last = LC.inputs(LC.SHAPES[si])
    assert LC.digest((out, Y, x_last)) == str(gv[f"s{si}_digest"]), "the regenerated inputs are not the fixture's"
    o = (x_last + out if r else out).numpy()
    C = o.shape[1]
    mask = np.ones(C) if not m else LC.mask_for(C, True).numpy()
    terms, grads = restate(o, Y.numpy(), mask)
    key = LC.case_key(si, r, m)
    for k, name in enumerate(LC.TERMS):
        assert LC.E(terms[k], gv[f"{key}_t64"][k]) <= 1e-12, name
    basis = gv[f"{LC.case_key(si, r, 0)}_g64"] * mask.reshape(1, 1, C, 1, 1)
    for k, name in enumerate(LC.TERMS):
        assert LC.E(grads[k], basis[k]) <= 1e-12, f"gradient of {name}"
    for wi, (sw, gw) in enumerate(LC.WEIGHTS):
        assert LC.E(terms[0] + sw * terms[1] + gw * terms[2], gv[f"{key}_tot64"][wi]) <= 1e-12


def test_fixture_is_well_conditioned_and_complete(gv):
    assert gv["cond_gap"].shape == (len(LC.SHAPES), 2, 2) and gv["cond_gap"].min() >= LC.MIN_GAP
    assert gv["cond_p"].min() >= LC.MIN_P and float(gv["basis_dev"]) < 1e-14
    assert [tuple(s) for s in gv["shapes"]] == LC.SHAPES and [tuple(w) for w in gv["weights"]] == LC.WEIGHTS
    for si, r, m in CASES:
        assert gv[f"{LC.case_key(si, r, m)}_E32"].shape == (len(LC.WEIGHTS), 5)


# ---- validation: before any GPU work ---------------------------------------------------------------------------------
def _pair(shape):
    return torch.zeros(*shape), torch.zeros(*shape)


@pytest.mark.parametrize("shape,limit", [((1, 2, 1, 4), "2 .. 256"), ((1, 2, 4, 1), "2 .. 256"), ((1, 2, 257, 4), "2 .. 256"),
                                         ((1, 2, 4, 257), "2 .. 256"), ((1, 65, 4, 4), "at most 64")])
def test_unsupported_sizes_raise_naming_the_limit(D, shape, limit):
    pred, target = _pair(shape)
    for fn in (D.masked_mse_loss, D.spectral_loss, D.gradient_loss, D.downscaler_loss):
        with pytest.raises(ValueError, match=limit):
            fn(pred, target)


def test_bad_operands_raise(D):
    pred, target = _pair((2, 3, 4, 5))
    for fn in (D.masked_mse_loss, D.spectral_loss, D.gradient_loss):
        with pytest.raises(ValueError, match="channel mask"):
            fn(pred, target, torch.ones(4))
        with pytest.raises(RuntimeError, match="GPU"):
            fn(pred, target, torch.ones(3))
        with pytest.raises(ValueError, match="requires grad"):
            fn(pred, target.clone().requires_grad_(True))
        with pytest.raises(ValueError, match="one shape"):
            fn(pred, target[:, :2])
    with pytest.raises(ValueError, match="channel mask"):
        D.downscaler_loss(pred, target, channel_mask=torch.ones(2))
    with pytest.raises(RuntimeError, match="GPU"):
        D.downscaler_loss(pred, target, spectral_weight=0.1, gradient_weight=0.05)
    with pytest.raises(ValueError, match="needs the input X"):
        D.downscaler_loss(pred, target, residual=True)
    with pytest.raises(ValueError, match="3 frames of 3 channels"):
        D.downscaler_loss(pred, target, X=torch.zeros(2, 8, 4, 5), obs_window=3, residual=True)
    with pytest.raises(RuntimeError, match="GPU"):
        D.downscaler_loss(pred, target, X=torch.zeros(2, 8, 4, 5), obs_window=2, residual=True)
    m = D.DownscalerMetrics(3, np.ones(3))
    with pytest.raises(ValueError, match="no batch"):
        m.results()
    with pytest.raises(ValueError, match="4 channels for 3"):
        D.DownscalerMetrics(3, np.ones(4))
    with pytest.raises(RuntimeError, match="GPU"):
        m.update(pred, torch.zeros(2, 8, 4, 5), target)


# ---- strings ---------------------------------------------------------------------------------------------------------
def test_table_and_results_match_the_reference_strings(D, gv):
    names, static = json.loads(str(gv["main_variables"])), [int(c) for c in gv["main_static"]]
    rm, rc, sk = gv["main_rmse_model"], gv["main_rmse_coarse"], gv["main_skill"]
    m = D.DownscalerMetrics(len(names), np.ones(len(names)), static)
    assert "\n".join(m.table(names, (rm, rc, sk))) == str(gv["main_table"])
    ref = json.loads(str(gv["main_results_json"]))
    ours = D.downscaler_results(float(gv["main_test_loss"]), rm, sk, names, static)
    assert list(ours) == list(ref) == ["test_loss", "mean_skill_vs_coarse", "per_channel_rmse", "per_channel_skill"]
    assert list(ours["per_channel_rmse"]) == list(ref["per_channel_rmse"])
    assert list(ours["per_channel_skill"]) == list(ref["per_channel_skill"])
    assert ours["test_loss"] == ref["test_loss"] and ours["per_channel_rmse"] == ref["per_channel_rmse"]
    assert ours["per_channel_skill"] == ref["per_channel_skill"]
    assert abs(ours["mean_skill_vs_coarse"] - ref["mean_skill_vs_coarse"]) <= 1e-6 * abs(ref["mean_skill_vs_coarse"])
    assert json.loads(json.dumps(ours, indent=2)) == ours
