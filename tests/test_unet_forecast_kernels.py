"""`gcl_grid_window_pack` and `gcl_grid_forecast_step` (csrc/unet_forecast.hip) called directly, at the smallest shapes that
can still go wrong, against the numpy restatements of tests/helpers/unet_forecast_case.py.

Shapes: 9 x 11 (odd: the one-float-per-lane path, partial tiles, two rows of tiles), 8 x 16 (the float4 path), 1 x 5, and -
beyond the issue's list, because the code takes other paths there - 17 x 40 (two columns of tiles, the second 8 wide),
65 x 260 and 65 x 259 (81 tiles: two tiles per chunk, on either path).  Ct = 7 with C = 5 (an odd run of halves, a channel
subset) and Ct = C = 4; obs 1, 2, 3; B = 3 with the middle row skipped.

Bounds: everything that is copied or carried is bit-equal to its source.  The sums differ from the restatement in the
order of their float64 additions only, so 1e-12 relative to the sum of the terms' magnitudes."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_forecast_case as FC  # noqa: E402
from layouts import DEV, SENT, Guarded, same_bits  # noqa: E402
from poison import poisoned  # noqa: E402

pytestmark = pytest.mark.gpu

AR = 3
KINDS = {"none": ([], []), "carry": ([4], [3]), "both": ([4, 3], [3])}
# (H, W, Ct, C, obs, channel table)
SHAPES = [(9, 11, 7, 5, 2, "carry"), (9, 11, 7, 5, 1, "none"), (9, 11, 7, 5, 3, "both"), (9, 11, 4, 4, 2, "none"),
          (8, 16, 7, 5, 2, "carry"), (8, 16, 4, 4, 3, "none"), (8, 16, 7, 5, 1, "both"),
          (1, 5, 7, 5, 2, "carry"), (1, 5, 4, 4, 1, "none"),
          (17, 40, 7, 5, 2, "carry"), (65, 260, 4, 4, 2, "none"), (65, 259, 7, 5, 2, "carry")]
IDS = [f"{h}x{w}-Ct{ct}-C{c}-obs{o}-{k}" for h, w, ct, c, o, k in SHAPES]


def hip():
    from graphcast_lite_amd import hip as H

    return H


class Case:
    """Series, scalers, window starts [1, -1, 2] and a random `out` of one shape; the numpy side is built once."""

    def __init__(self, H, W, Ct, C, obs, kinds, seed=0, starts=(1, -1, 2)):
        rng = np.random.default_rng(1000 * H + W + 17 * Ct + obs + seed)
        self.H, self.W, self.Ct, self.C, self.obs = H, W, Ct, C, obs
        self.T = obs + AR + 3
        self.series = (rng.standard_normal((self.T, W, H, Ct)) * 2 + 1).astype(np.float16)
        self.mean = rng.standard_normal(C).astype(np.float32)
        self.std = (0.5 + rng.random(C)).astype(np.float32)
        self.static, self.forcing = KINDS[kinds]
        self.kind = FC.kinds_of(C, self.static, self.forcing)
        self.starts = list(starts)
        self.B = len(starts)
        self.out = rng.standard_normal((self.B, C, H, W)).astype(np.float32)
        self.X = np.stack([FC.window_np(self.series, max(t, 0), self.mean, self.std, C, 0, obs) for t in self.starts])
        self.init = rng.standard_normal((AR, C, 5))
        self.d = {k: torch.from_numpy(v).to(DEV) for k, v in
                  {"series": self.series, "mean": self.mean, "std": self.std, "kind": self.kind, "out": self.out, "X": self.X}.items()}

    def t0(self, starts=None):
        return torch.tensor(self.starts if starts is None else starts, dtype=torch.int64, device=DEV)

    def step(self, step, out=None, X=None, starts=None, state=None, acc_count=None, count=None, with_pred=True, rows=None):
        """One call; returns (X_next guard, pred guard or None, state, acc_count, count, ws)."""
        out = self.d["out"] if out is None else out
        X = self.d["X"] if X is None else X
        if rows is not None:
            out, X = out[rows].contiguous(), X[rows].contiguous()
        B = out.shape[0]
        xn = Guarded((B, self.obs * self.C, self.H, self.W))
        pr = Guarded((B, self.C, self.H, self.W)) if with_pred else None
        state = torch.from_numpy(self.init).to(DEV) if state is None else state
        acc_count = torch.full((AR, self.C), 5, dtype=torch.int64, device=DEV) if acc_count is None else acc_count
        count = torch.full((AR,), 11, dtype=torch.int64, device=DEV) if count is None else count
        need = int(hip().lib().gcl_grid_forecast_step_ws_bytes(B, self.H, self.W, self.C))
        assert need % (72 * B * self.C) == 0
        ws = torch.full((need // 8,), math.nan, dtype=torch.float64, device=DEV)
        hip().grid_forecast_step(out, X, self.d["series"], self.t0(starts), self.d["kind"], self.d["mean"], self.d["std"], step,
                                 xn.view, state, acc_count, count, pred=pr.view if pr is not None else None, ws=ws)
        torch.cuda.synchronize()
        return xn, pr, state, acc_count, count, ws

    def reference(self, step, b, out=None):
        out = self.out if out is None else out
        return FC.step_np(out[b], self.X[b], self.series, self.starts[b], self.kind, self.mean, self.std, self.obs, step)


def chunk_sums(ws, B, C):
    """[B, C, 9] of the workspace's partial sums (see gcl_grid_forecast_step)."""
    n = ws.numel() // (9 * B * C)
    first = ws[:B * C * 6 * n].view(B, C, 6, n).sum(-1)
    second = ws[B * C * 6 * n:].view(B, C, 3, n).sum(-1)
    return torch.cat([first, second], dim=2).cpu().numpy()


def close(got, want, scale, what):
    bound = 1e-12 * np.maximum(np.abs(scale), 1e-300)
    bad = ~(np.abs(got - want) <= bound)
    assert not bad.any(), f"{what}: {got[bad][:4]} against {want[bad][:4]} (bound {bound[bad][:4]})"


# ---------------------------------------------------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Ct,C,obs,kinds", SHAPES, ids=IDS)
def test_pack_is_the_loader_bit_for_bit(H, W, Ct, C, obs, kinds):
    c = Case(H, W, Ct, C, obs, kinds)
    starts = [1, -1, c.T - obs, c.T - obs + 1, 0]  # in range, before the series, the last window, one past it, the first
    buf = Guarded((len(starts), obs * C, H, W))
    hip().grid_window_pack(c.d["series"], c.t0(starts), c.d["mean"], c.d["std"], obs, out=buf.view)
    got = buf.view.cpu()
    assert buf.untouched()
    for b, t in enumerate(starts):
        if 0 <= t and t + obs <= c.T:
            assert same_bits(got[b], torch.from_numpy(FC.window_np(c.series, t, c.mean, c.std, C, 0, obs))), (b, t)
        else:
            assert bool(got[b].isnan().all()), (b, t)


def test_pack_rejects_bad_arguments():
    c = Case(8, 16, 4, 4, 2, "none")
    with pytest.raises(ValueError, match="C <="):
        hip().grid_window_pack(c.d["series"], c.t0(), torch.zeros(5, device=DEV), torch.ones(5, device=DEV), 2)
    with pytest.raises(ValueError, match="float16"):
        hip().grid_window_pack(c.d["series"].float(), c.t0(), c.d["mean"], c.d["std"], 2)
    with pytest.raises(ValueError, match="out"):
        hip().grid_window_pack(c.d["series"], c.t0(), c.d["mean"], c.d["std"], 2, out=torch.zeros(3, 8, 16, 8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, AR - 1])
@pytest.mark.parametrize("H,W,Ct,C,obs,kinds", SHAPES, ids=IDS)
def test_step_against_the_restatement(H, W, Ct, C, obs, kinds, step):
    """Carry and shift bit for bit, the skipped row and the guards untouched, the nine sums of every (sample, channel) and
    the state's five (with the correlation the tenth) to 1e-12."""
    c = Case(H, W, Ct, C, obs, kinds)
    xn, pr, state, acc_count, count, ws = c.step(step)
    assert xn.untouched() and pr.untouched()
    got_xn, got_pr = xn.view.cpu().numpy(), pr.view.cpu().numpy()
    sums = chunk_sums(ws, c.B, C)
    want_state, want_cnt = c.init[step].copy(), np.full(C, 5, dtype=np.int64)
    for b, t in enumerate(c.starts):
        if t < 0:
            assert (got_xn[b] == SENT).all() and (got_pr[b] == SENT).all(), "a skipped sample's outputs were written"
            continue
        p, ref = c.reference(step, b)
        assert same_bits(torch.from_numpy(got_pr[b]), torch.from_numpy(p)), f"sample {b}: out'"
        assert same_bits(torch.from_numpy(got_xn[b, (obs - 1) * C:]), torch.from_numpy(p)), f"sample {b}: X_next's last frame"
        assert same_bits(torch.from_numpy(got_xn[b, :(obs - 1) * C]), torch.from_numpy(c.X[b, C:])), f"sample {b}: the shift"
        for ch in c.static:
            if c.kind[ch] == 1:
                assert same_bits(torch.from_numpy(got_pr[b, ch]), torch.from_numpy(c.X[b, (obs - 1) * C + ch]))
        g = FC.window_np(c.series, t, c.mean, c.std, C, obs + step, 1)
        for ch in c.forcing:
            assert same_bits(torch.from_numpy(got_pr[b, ch]), torch.from_numpy(g[ch]))
        mag = np.abs(p.astype(np.float64)).sum((1, 2)), np.abs(g.astype(np.float64)).sum((1, 2))
        scale = np.stack([ref[:, 0], ref[:, 1], ref[:, 2], ref[:, 3], mag[0], mag[1], ref[:, 6], ref[:, 7],
                          np.sqrt(ref[:, 6] * ref[:, 7])], axis=1)
        close(sums[b], ref[:, :9], scale, f"sample {b}: the nine sums")
        counted = ~np.isnan(ref[:, 9])
        want_state[:, :4] += ref[:, :4]
        want_state[:, 4] += np.where(counted, ref[:, 9], 0.0)
        want_cnt += counted
    got_state = state.cpu().numpy()
    close(got_state[step], want_state, np.abs(c.init[step]) + np.abs(want_state) + 1.0, "state")
    other = [s for s in range(AR) if s != step]
    assert np.array_equal(got_state[other], c.init[other]), "another step's state was touched"
    assert np.array_equal(acc_count.cpu().numpy()[step], want_cnt)
    assert (acc_count.cpu().numpy()[other] == 5).all()
    want_count = np.full(AR, 11)
    want_count[step] += H * W * sum(t >= 0 for t in c.starts)
    assert np.array_equal(count.cpu().numpy(), want_count)


def test_truth_frame_past_the_series_is_skipped():
    c = Case(9, 11, 7, 5, 2, "carry")
    last = c.T - c.obs - 1  # truth frame of step 0 is the last frame; of step 1 it is outside
    xn, pr, state, acc_count, count, _ = c.step(1, starts=[last, 0, last])
    assert (xn.view[0] == SENT).all() and (xn.view[2] == SENT).all() and not (xn.view[1] == SENT).any()
    assert int(count[1]) == 11 + 9 * 11


def test_pred_may_be_null():
    c = Case(9, 11, 7, 5, 2, "carry")
    a = c.step(0)
    b = c.step(0, with_pred=False)
    assert same_bits(a[0].view, b[0].view) and same_bits(a[2], b[2]) and b[1] is None


def test_acc_gate_leaves_a_constant_field_uncounted():
    c = Case(9, 11, 7, 5, 2, "none")
    out = c.out.copy()
    out[:, 1] = 0.37  # a dynamic channel that is constant in space: its centred norm is exactly zero
    _, _, state, acc_count, _, _ = c.step(0, out=torch.from_numpy(out).to(DEV))
    assert same_bits(state[0, 1, 4].cpu(), torch.tensor(c.init[0, 1, 4])), "acc_sum moved"
    assert acc_count[0].tolist() == [7, 5, 7, 7, 7]
    assert bool(torch.isfinite(state).all())


@pytest.mark.parametrize("H,W", [(9, 11), (8, 16), (65, 260)])
def test_batch_size_does_not_reach_the_bits(H, W):
    c = Case(H, W, 7, 5, 2, "carry", starts=(1, 0, 2))
    whole = c.step(1)
    state = torch.from_numpy(c.init).to(DEV)
    acc_count = torch.full((AR, c.C), 5, dtype=torch.int64, device=DEV)
    count = torch.full((AR,), 11, dtype=torch.int64, device=DEV)
    for b in range(3):
        one = c.step(1, rows=[b], starts=[c.starts[b]], state=state, acc_count=acc_count, count=count)
        assert same_bits(one[0].view[0], whole[0].view[b])
    assert same_bits(state, whole[2]) and torch.equal(acc_count, whole[3]) and torch.equal(count, whole[4])


def test_nan_stays_in_its_sample():
    c = Case(9, 11, 7, 5, 2, "carry", starts=(1, 0, 2))
    clean = c.step(0)
    dirty = c.step(0, out=poisoned(c.d["out"], (0, 0, 3, 4)), X=poisoned(c.d["X"], (0, 7, 1, 1)))  # a value the shift carries
    for b in (1, 2):
        assert bool(torch.isfinite(dirty[0].view[b]).all()) and same_bits(dirty[0].view[b], clean[0].view[b])
    assert bool(dirty[0].view[0].isnan().any())
    assert bool(dirty[2][0, 0].isnan().any()), "the NaN reaches its sample's sums and so the state, as in the reference"
    assert bool(torch.isfinite(dirty[2][0, 1:3]).all())


def test_acc_with_a_huge_mean_and_a_tiny_spread():
    """out' and the truth are 1e4 +- 1e-2: the two-pass float64 sums give the correlation of the float32 fields to 1e-6
    (a one-pass float32 or float64 form loses every digit)."""
    H, W, C, obs = 9, 11, 5, 2
    c = Case(H, W, 7, C, obs, "none", starts=(1,))
    rng = np.random.default_rng(5)
    c.series = (1e-2 * rng.standard_normal(c.series.shape)).astype(np.float16)
    c.mean, c.std = np.full(C, -1e4, dtype=np.float32), np.ones(C, dtype=np.float32)
    g = FC.window_np(c.series, 1, c.mean, c.std, C, obs, 1)
    out = (1e4 + 0.7 * (g.astype(np.float64) - 1e4) + 0.7e-2 * rng.standard_normal(g.shape)).astype(np.float32)[None]
    c.X = np.stack([FC.window_np(c.series, 1, c.mean, c.std, C, 0, obs)])
    c.d.update({k: torch.from_numpy(v).to(DEV) for k, v in {"series": c.series, "mean": c.mean, "std": c.std, "X": c.X}.items()})
    state = torch.zeros(AR, C, 5, dtype=torch.float64, device=DEV)
    acc_count = torch.zeros(AR, C, dtype=torch.int64, device=DEV)
    c.step(0, out=torch.from_numpy(out).to(DEV), state=state, acc_count=acc_count)
    _, ref = FC.step_np(out[0], c.X[0], c.series, 1, c.kind, c.mean, c.std, obs, 0)
    assert acc_count[0].tolist() == [1] * C
    corr = state[0, :, 4].cpu().numpy()
    assert 0.3 < ref[:, 9].min() and ref[:, 9].max() < 0.95, ref[:, 9]  # a correlation that says something
    assert np.abs(corr - ref[:, 9]).max() < 1e-6, (corr, ref[:, 9])


def test_step_rejects_bad_arguments():
    c = Case(8, 16, 4, 4, 2, "none")
    state = torch.zeros(AR, 4, 5, dtype=torch.float64, device=DEV)
    acc_count = torch.zeros(AR, 4, dtype=torch.int64, device=DEV)
    count = torch.zeros(AR, dtype=torch.int64, device=DEV)
    xn = torch.empty_like(c.d["X"])
    args = (c.d["out"], c.d["X"], c.d["series"], c.t0(), c.d["kind"], c.d["mean"], c.d["std"])
    with pytest.raises(RuntimeError, match="step 3 of 3"):
        hip().grid_forecast_step(*args, 3, xn, state, acc_count, count)
    with pytest.raises(RuntimeError, match="must not be X"):
        hip().grid_forecast_step(*args, 0, c.d["X"], state, acc_count, count)
    with pytest.raises(RuntimeError, match="workspace"):
        hip().grid_forecast_step(*args, 0, xn, state, acc_count, count, ws=torch.zeros(8, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="state"):
        hip().grid_forecast_step(*args, 0, xn, state[:, :, :3].contiguous(), acc_count, count)
    with pytest.raises(ValueError, match="chan_kind"):
        hip().grid_forecast_step(*args[:4], c.d["kind"].int(), *args[5:], 0, xn, state, acc_count, count)


def test_launch_counts():
    c = Case(9, 11, 7, 5, 2, "carry")
    n0 = hip().unet_forecast_launches()
    hip().grid_window_pack(c.d["series"], c.t0(), c.d["mean"], c.d["std"], 2)
    assert hip().unet_forecast_launches() == n0 + 1
    c.step(0)
    assert hip().unet_forecast_launches() == n0 + 4
