"""The final passes of a backward, queued (hip.defer_begin .. hip.defer_flush) against the same calls made immediately.

A queued pass sums the same partial records in the same order as the immediate one, so every comparison is torch.equal.
Shapes are the smallest that still take the 16-byte reducer, which needs 64 partial records: 70 x 16 rows for the
LayerNorm backward and the column sums (16 rows per block at F = 64 and F = 48), 70 x 128 rows for the dW kernel (a block
takes at least two 64-row steps) and 70 x 64 rows for the fused dense backward."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
JOBS_PER_LAUNCH = 24  # kJobsPerLaunch of csrc/linear.hip
LN_ROWS, DW_ROWS, ALL_ROWS = 70 * 16, 70 * 128, 70 * 64


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _queue_closed(hip):
    yield
    hip.defer_flush(drop=True)  # a failed test must not leave the queue open for the next one


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).to(DEV)


def dest(shape, acc):
    """A destination: holding 1.5 when the call adds into it, NaN when the call has to overwrite it."""
    return torch.full(shape, 1.5 if acc else float("nan"), device=DEV)


def pending(hip):
    return len(hip._deferred.jobs)


class LN:
    """One LayerNorm backward (dense, mapped or mapped + skip) with destinations of its own."""

    def __init__(self, hip, F, seed, acc=False, acc_cs=False, cs=True, mode="dense", rows=LN_ROWS):
        self.hip, self.F, self.acc, self.acc_cs, self.mode = hip, F, acc, acc_cs, mode
        self.x = rnd(rows, F, seed=seed)
        self.gm = 1 + 0.1 * rnd(F, seed=seed + 1)
        _, self.stats = hip.layernorm_fwd(self.x, self.gm, torch.zeros(F, device=DEV))
        self.dy = rnd(rows, F, seed=seed + 2)
        n = rows // 2  # two samples
        keep = torch.rand(n, generator=torch.Generator().manual_seed(seed + 3)) < 0.6
        pos = torch.full((n,), -1, dtype=torch.int32)
        pos[keep] = torch.arange(int(keep.sum()), dtype=torch.int32)
        self.pos = pos.to(DEV)
        self.src3 = rnd(2, int(keep.sum()) + 1, F, seed=seed + 4)
        self.present = keep.to(DEV).repeat(2)
        self.with_cs = cs

    def run(self):
        F = self.F
        dg, db = dest((F,), self.acc), dest((F,), self.acc)
        cs = dest((F,), self.acc_cs) if self.with_cs else None
        if self.mode == "dense":
            dx = self.hip.layernorm_bwd(self.dy, self.x, self.gm, self.stats, dg, db, self.acc, colsum_dx=cs, acc_colsum=self.acc_cs)
        else:
            dx = self.hip.layernorm_bwd(None, self.x, self.gm, self.stats, dg, db, self.acc, colsum_dx=cs, acc_colsum=self.acc_cs,
                                        dy_map=(self.src3, self.pos), skip=self.mode == "skip")
        return lambda: [dx[self.present] if self.mode == "skip" else dx, dg, db] + ([cs] if cs is not None else [])


class ColSum:
    def __init__(self, hip, F, seed, acc=False, rows=LN_ROWS):
        self.hip, self.acc = hip, acc
        self.x = rnd(rows, F, seed=seed)

    def run(self):
        out = dest((self.x.shape[1],), self.acc)
        self.hip.colsum(self.x, out, self.acc)
        return lambda: [out]


class DW:
    """The dW kernel: dW and db come from two partial buffers, that is two queued passes."""

    def __init__(self, hip, Fin, Fout, seed, acc=False, bias=True):
        self.hip, self.acc, self.bias = hip, acc, bias
        rows = DW_ROWS * (2 if Fin > 128 else 1)  # a block of a layer with several input chunks takes four steps
        self.dy, self.x = rnd(rows, Fout, seed=seed), rnd(rows, Fin, seed=seed + 1)

    def run(self):
        dW = dest((self.dy.shape[1], self.x.shape[1]), self.acc)
        db = dest((self.dy.shape[1],), self.acc) if self.bias else None
        self.hip.dense_bwd_dw(self.dy, self.x, dW, db, self.acc)
        return lambda: [dW] + ([db] if db is not None else [])


class All:
    """The fused dense backward with a PReLU slope: its slope gradient is ADDED to `dslope`, which calls may share."""

    def __init__(self, hip, F, seed, dslope):
        self.hip, self.dslope = hip, dslope
        self.dy, self.x = rnd(ALL_ROWS, F, seed=seed), rnd(ALL_ROWS, F, seed=seed + 1)
        self.W, self.slope = rnd(F, F, seed=seed + 2) / 8, torch.full((1,), 0.25, device=DEV)

    def run(self):
        F = self.W.shape[0]
        dW, db = dest((F, F), False), dest((F,), False)
        dx = self.hip.linear_bwd_all(self.dy, self.W, self.x, self.slope, self.dslope[0], dW, db, None, False)
        return lambda: [dx, dW, db, self.dslope[0]]


def immediate_and_queued(hip, calls, slopes=(), jobs=None):
    """Run `calls` immediately, then through the queue, and compare everything they wrote.  `slopes`: the shared slope
    gradient holders ([tensor]), reset between the two rounds."""
    def fresh():
        for s in slopes:
            s[0] = torch.full((1,), 0.5, device=DEV)

    fresh()
    want_fns = [c.run() for c in calls]
    want = [t.clone() for f in want_fns for t in f()]
    fresh()
    hip.defer_begin()
    got_fns = [c.run() for c in calls]
    if jobs is not None:
        assert pending(hip) == jobs, f"{pending(hip)} passes are queued, expected {jobs}"
    hip.defer_flush()
    assert not hip._deferred.active and pending(hip) == 0
    got = [t for f in got_fns for t in f()]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert bool(torch.isfinite(g).all()), f"output {k} holds a non-finite value"
        assert torch.equal(g, w), f"output {k} differs between the queued and the immediate pass"


@pytest.mark.parametrize("F", [64, 48])
@pytest.mark.parametrize("acc,acc_cs", list(itertools.product([False, True], repeat=2)))
@pytest.mark.parametrize("mode", ["dense", "map", "skip"])
def test_layernorm_backward_queued(hip, F, acc, acc_cs, mode):
    immediate_and_queued(hip, [LN(hip, F, 11, acc, acc_cs, mode=mode)], jobs=1)


@pytest.mark.parametrize("F", [64, 48])
def test_layernorm_backward_without_column_sums_queued(hip, F):
    immediate_and_queued(hip, [LN(hip, F, 12, cs=False), LN(hip, F, 13, acc=True, cs=False)], jobs=2)


@pytest.mark.parametrize("F", [64, 48])
@pytest.mark.parametrize("acc", [False, True])
def test_colsum_queued(hip, F, acc):
    immediate_and_queued(hip, [ColSum(hip, F, 21, acc)], jobs=1)


@pytest.mark.parametrize("Fin,Fout", [(64, 64), (48, 64), (72, 48), (200, 64)])
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_dw_queued(hip, Fin, Fout, acc, bias):
    """72 inputs is the first encoder layer of the flagship model; 200 inputs are two 128-column chunks (two segments)."""
    immediate_and_queued(hip, [DW(hip, Fin, Fout, 31, acc, bias)], jobs=2 if bias else 1)


def test_too_few_records_reduce_on_the_spot(hip):
    """Fewer than 64 partial records: the immediate pass takes the other reducer, so nothing may be queued."""
    immediate_and_queued(hip, [LN(hip, 64, 41, rows=40 * 16), ColSum(hip, 64, 42, rows=40 * 16)], jobs=0)


def test_more_jobs_than_one_launch_holds(hip):
    calls = [ColSum(hip, 64, 100 + k, acc=bool(k % 2)) for k in range(JOBS_PER_LAUNCH + 3)]
    immediate_and_queued(hip, calls, jobs=JOBS_PER_LAUNCH + 3)


def test_two_jobs_share_a_slope(hip):
    s = [None]
    immediate_and_queued(hip, [All(hip, 64, 51, s), All(hip, 64, 52, s)], slopes=[s], jobs=2)


def test_three_jobs_share_a_slope_across_a_launch_boundary(hip):
    """Jobs 22 and 23 are the last two of the first launch, job 24 the first of the second."""
    s = [None]
    calls = [ColSum(hip, 64, 200 + k) for k in range(JOBS_PER_LAUNCH - 2)] + [All(hip, 64, 61 + k, s) for k in range(3)]
    immediate_and_queued(hip, calls, slopes=[s], jobs=JOBS_PER_LAUNCH + 1)


def test_queue_without_slope_partials(hip):
    immediate_and_queued(hip, [ColSum(hip, 64, 71), LN(hip, 48, 72), DW(hip, 64, 64, 73)], jobs=4)


def test_only_the_last_job_has_slope_partials(hip):
    s = [None]
    immediate_and_queued(hip, [ColSum(hip, 64, 81), LN(hip, 64, 82), All(hip, 64, 83, s)], slopes=[s], jobs=3)


def test_same_destination_flushes_in_between(hip):
    """The second call adds into what the first one writes: the first pass has to run before the second is queued."""
    x1, x2 = rnd(LN_ROWS, 64, seed=91), rnd(LN_ROWS, 64, seed=92)
    want = torch.full((64,), float("nan"), device=DEV)
    hip.colsum(x1, want, False)
    hip.colsum(x2, want, True)
    out = torch.full((64,), float("nan"), device=DEV)
    other = torch.zeros(64, device=DEV)
    hip.defer_begin()
    hip.colsum(x1, out, False)
    hip.colsum(x1, other, False)
    assert pending(hip) == 2
    hip.colsum(x2, out, True)
    assert pending(hip) == 1 and hip._deferred.active, "the queued passes were not flushed before the colliding call"
    hip.defer_flush()
    assert torch.equal(out, want)
    ref_other = torch.empty(64, device=DEV)
    hip.colsum(x1, ref_other, False)
    assert torch.equal(other, ref_other)


def test_partials_outlive_other_workspace_users(hip):
    """Two queued LayerNorm backwards with an unrelated user of the shared scratch workspace in between and after: their
    partial records live in workspaces of the queue's own."""
    a, b = LN(hip, 64, 95, mode="skip"), LN(hip, 48, 96)
    want = [t.clone() for f in [a.run(), b.run()] for t in f()]
    hip.defer_begin()
    fa = a.run()
    hip.workspace(1 << 22, DEV).fill_(255)  # every float of it a NaN
    fb = b.run()
    hip.workspace(1 << 22, DEV).fill_(255)
    assert pending(hip) == 2
    hip.defer_flush()
    got = fa() + fb()
    for g, w in zip(got, want):
        assert torch.equal(g, w)
