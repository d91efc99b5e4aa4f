"""The kernels of the downscaler's objective and scores (csrc/downscale_loss.hip) called through their thin hip.py
wrappers on operands between guard elements, against the reference's own float64 values
(tests/golden/downscale_loss_vectors.npz, made by tests/golden/make_downscale_loss_golden.py).

Rules:
  accuracy     for every fixture case (six shapes x residual x mask x four weights) and every quantity - the three
               terms, the total and dOut - E(kernel) <= 4 * max(E(ref32), 2^-24), E(x) = max |x - x64| / max |x64| and
               E(ref32) the error of the reference's own float32 run from the fixture.  The margin of 4 covers another
               summation order and a direct DFT of up to 256 terms where the FFT sums in log2 stages.  No case and no
               element is left out.
  mask         dOut on a masked channel is exactly 0.
  skipped      a term whose weight is 0 leaves its record untouched (the sentinel stays).
  repeatable   two runs give the same bits; storing the spectral gradient equals adding it to zeros.
  guards       out, Y, the larger X that x_last is a strided slice of, dOut, the record, the metrics state and the
               counter lie between guard elements, which stay intact.
  metrics      after batches of 4, 4 and 1 samples the state is within 1e-12 relative of a float64 restatement of the
               per-batch-mean rule and within 64 * 2^-24 relative of the reference's float32 result (non-negative
               terms, torch reduces pairwise over 4096 elements or fewer); the counter reads 3; captured by
               torch.cuda.graph and replayed twice more it reads 5 and the sums match the restatement.
The worst error / bound per rule is printed (run with -s).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import downscale_loss_case as LC  # noqa: E402

# the wrappers under test, reached below through the `H` fixture once the library is built
from graphcast_lite_amd.hip import (downscale_loss_fwd_bwd, downscale_loss_scale, downscale_metrics,  # noqa: F401
                                    downscale_spectral_fwd_bwd)

gpu = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.25  # exact in float32, float64 and as an integer's negative
EPS = 2.0 ** -24
CASES = [(si, r, m) for si in range(len(LC.SHAPES)) for r in (0, 1) for m in (0, 1)]
WORST = {}


@pytest.fixture(scope="module")
def H(lib_built):
    from graphcast_lite_amd import hip

    return hip


@pytest.fixture(scope="module")
def gv():
    return LC.golden()


class Archive:
    """A contiguous array of `shape` inside a buffer with `guard` sentinel elements either side."""

    def __init__(self, shape, guard=8, dtype=torch.float32, sent=SENT):
        n = math.prod(shape)
        self.guard, self.n, self.sent = guard, n, sent
        self.buf = torch.full((n + 2 * guard,), sent, dtype=dtype, device=DEV)
        self.view = self.buf[guard:guard + n].view(shape)

    def put(self, t):
        self.view.copy_(t.to(self.view.dtype))
        return self.view

    def host(self):
        return self.view.cpu().numpy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return (b[:self.guard] == self.sent).all() and (b[self.guard + self.n:] == self.sent).all()


def note(rule, err, bound):
    WORST[rule] = max(WORST.get(rule, 0.0), err / bound)
    return err <= bound


class Operands:
    """out, Y and x_last (channels C .. 2C of an X of 2C + 1 channels) in float32 between guards."""

    def __init__(self, si, residual, masked):
        out, Y, x_last = LC.inputs(LC.SHAPES[si])
        B, C, Hh, W = out.shape
        self.shape = (B, C, Hh, W)
        self.out, self.Y = Archive(self.shape, 5), Archive(self.shape, 3)
        self.out.put(out), self.Y.put(Y)
        self.X = Archive((B, 2 * C + 1, Hh, W), 7)
        self.X.view[:, C:2 * C].copy_(x_last.to(torch.float32))
        self.x_last = self.X.view[:, C:2 * C] if residual else None
        m = LC.mask_for(C, masked, torch.float32)
        self.mask = None if m is None else m.to(DEV)
        self.dout, self.rec = Archive(self.shape, 9), Archive((3,), 2, torch.float64)
        self.everything = (self.out, self.Y, self.X, self.dout, self.rec)

    def run(self, H, sw, gw, dout=True):
        self.rec.buf.fill_(SENT)
        d = self.dout.view if dout else None
        H.downscale_loss_fwd_bwd(self.out.view, self.Y.view, self.rec.view, self.x_last, self.mask, 1.0, gw, d)
        if sw > 0:
            H.downscale_spectral_fwd_bwd(self.out.view, self.Y.view, self.rec.view, self.x_last, self.mask, sw, d, accumulate=True)
        return self.rec.host().copy(), self.dout.host().copy()


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: LC.case_key(*c))
def test_terms_total_and_gradient_within_the_reference_float32_error(H, gv, case):
    si, r, m = case
    op = Operands(si, r, m)
    B, C, Hh, W = op.shape
    key = LC.case_key(si, r, m)
    t64, tot64, E32 = gv[f"{key}_t64"], gv[f"{key}_tot64"], gv[f"{key}_E32"]
    mc = np.ones(C) if not m else LC.mask_for(C, True).numpy()
    basis = gv[f"{LC.case_key(si, r, 0)}_g64"] * mc.reshape(1, 1, C, 1, 1)
    for wi, (sw, gw) in enumerate(LC.WEIGHTS):
        rec, dout = op.run(H, sw, gw)
        bound = lambda k: 4.0 * max(E32[wi][k], EPS)  # noqa: E731
        assert note("mse", LC.E(rec[0], t64[0]), bound(0)), (key, sw, gw, rec[0], t64[0])
        if sw > 0:
            assert note("spec", LC.E(rec[2], t64[1]), bound(1)), (key, sw, gw, rec[2], t64[1])
        else:
            assert rec[2] == SENT, "a skipped spectral term wrote its record"
        if gw > 0:
            assert note("grad", LC.E(rec[1], t64[2]), bound(2)), (key, sw, gw, rec[1], t64[2])
        else:
            assert rec[1] == SENT, "a skipped gradient term wrote its record"
        total = rec[0] + (sw * rec[2] if sw > 0 else 0.0) + (gw * rec[1] if gw > 0 else 0.0)
        assert note("total", LC.E(np.float32(total), tot64[wi]), bound(3)), (key, sw, gw, total, tot64[wi])
        g64 = basis[0] + sw * basis[1] + gw * basis[2]
        err = LC.E(dout, g64)
        print(f"{key} sw={sw} gw={gw}: E(dOut) = {err:.3e}, bound {bound(4):.3e}")
        assert note("dOut", err, bound(4)), (key, sw, gw, err, bound(4))
        if m:
            assert (dout[:, LC.MASKED_CHANNEL] == 0).all(), "dOut on the masked channel is not exactly 0"
        for a in op.everything:
            assert a.guards_intact()
    rec2, dout2 = op.run(H, sw, gw)  # the last weights again
    assert rec2.tobytes() == rec.tobytes() and dout2.tobytes() == dout.tobytes(), "two runs differ in their bits"
    print("worst error / bound so far:", {k: round(v, 4) for k, v in WORST.items()})


@gpu
@pytest.mark.parametrize("si", [1, 3, 5])
def test_spectral_alone_stores_what_it_would_add_to_zeros(H, si):
    op = Operands(si, True, True)
    stored, added = Archive(op.shape, 4), Archive(op.shape, 4)
    added.view.zero_()
    rec = Archive((3,), 2, torch.float64)
    for dst, acc in ((stored, False), (added, True)):
        H.downscale_spectral_fwd_bwd(op.out.view, op.Y.view, rec.view, op.x_last, op.mask, 1.0, dst.view, accumulate=acc)
    assert stored.host().tobytes() == added.host().tobytes() and np.abs(stored.host()).max() > 0
    before = rec.host().copy()
    H.downscale_spectral_fwd_bwd(op.out.view, op.Y.view, rec.view, op.x_last, op.mask, 1.0, None)  # forward only
    assert rec.host().tobytes() == before.tobytes() and before[0] == SENT and before[1] == SENT
    assert stored.guards_intact() and added.guards_intact() and rec.guards_intact()


@gpu
def test_gradient_term_alone_and_the_scale_kernel(H, gv):
    """mse_weight 0: only the finite-difference term runs (the record of the mse stays), and dOut is its gradient;
    the backward scale multiplies by a device scalar."""
    si = 3
    op = Operands(si, False, False)
    op.rec.buf.fill_(SENT)
    H.downscale_loss_fwd_bwd(op.out.view, op.Y.view, op.rec.view, None, None, 0.0, 1.0, op.dout.view)
    rec, key = op.rec.host(), LC.case_key(si, 0, 0)
    assert rec[0] == SENT and rec[2] == SENT
    assert LC.E(rec[1], gv[f"{key}_t64"][2]) <= 4.0 * max(gv[f"{key}_E32"][0][2], EPS)
    assert LC.E(op.dout.host(), gv[f"{key}_g64"][2]) <= 4.0 * max(gv[f"{key}_Eg32"][2], EPS)
    scaled = Archive(op.shape, 6)
    H.downscale_loss_scale(op.dout.view, torch.tensor([2.5], device=DEV), scaled.view)
    assert (scaled.host() == op.dout.host() * np.float32(2.5)).all() and scaled.guards_intact()
    with pytest.raises(RuntimeError, match="neither term"):
        H.downscale_loss_fwd_bwd(op.out.view, op.Y.view, op.rec.view, None, None, 0.0, 0.0, op.dout.view)


# ---- metrics ---------------------------------------------------------------------------------------------------------
def metrics_restated(batches, residual):
    """float64 [C, 2]: the sum over the batches of the per-batch means of the float32 differences squared."""
    state = np.zeros((LC.METRICS_C, 2))
    C, obs = LC.METRICS_C, LC.METRICS_OBS
    for X, Y, out in batches:
        xl = X[:, (obs - 1) * C:obs * C]
        o = xl + out if residual else out  # float32
        for q, d in enumerate((o - Y, xl - Y)):
            state[:, q] += (d.numpy().astype(np.float64) ** 2).mean(axis=(0, 2, 3))
    return state


@gpu
@pytest.mark.parametrize("residual", [False, True])
def test_metrics_state_counter_and_graph_replay(H, gv, residual):
    batches = LC.metrics_inputs()
    assert LC.digest([t for b in batches for t in b]) == str(gv["metrics_digest"])
    C, obs = LC.METRICS_C, LC.METRICS_OBS
    state, count = Archive((C, 2), 3, torch.float64), Archive((1,), 2, torch.int64, -7)
    state.view.zero_(), count.view.zero_()
    dev = []
    for X, Y, out in batches:
        Xa, Ya, oa = Archive(tuple(X.shape), 5), Archive(tuple(Y.shape), 3), Archive(tuple(out.shape), 1)
        Xa.put(X), Ya.put(Y), oa.put(out)
        dev.append((Xa, Ya, oa))
        H.downscale_metrics(oa.view, Xa.view[:, (obs - 1) * C:obs * C], Ya.view, residual, state.view, count.view)
    want = metrics_restated(batches, residual)
    got = state.host().copy()
    assert note("metrics vs float64", float(np.max(np.abs(got - want) / want)), 1e-12)
    assert int(count.host()[0]) == 3
    r = int(residual)
    ref = np.stack([gv[f"metrics_r{r}_rmse_model"].astype(np.float64) ** 2,
                    gv[f"metrics_r{r}_rmse_coarse"].astype(np.float64) ** 2], axis=1)  # std = 1: the float32 means
    assert note("metrics vs float32", float(np.max(np.abs(got / 3 - ref) / ref)), 64 * EPS)

    Xa, Ya, oa = dev[0]
    xl = Xa.view[:, (obs - 1) * C:obs * C]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H.downscale_metrics(oa.view, xl, Ya.view, residual, state.view, count.view)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert int(count.host()[0]) == 5
    want5 = want + 2 * metrics_restated(batches[:1], residual)
    assert note("metrics replayed vs float64", float(np.max(np.abs(state.host() - want5) / want5)), 1e-12)
    for a in (state, count) + tuple(x for t in dev for x in t):
        assert a.guards_intact()
    print("worst error / bound so far:", {k: round(v, 4) for k, v in WORST.items()})
