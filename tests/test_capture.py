"""capture.Captured, the warm-up / capture / replay state machine of every captured path, on the CPU: the hipGraph
is replaced by a fake whose capture records the callable and whose replay runs it again on the static buffers."""
import warnings

import pytest
import torch

from graphcast_lite_amd import capture as CAP
from graphcast_lite_amd import models


class FakeGraph:
    made = 0

    def __init__(self):
        FakeGraph.made += 1
        self.fn = None

    def capture(self, fn):
        self.fn = fn
        return fn()  # a real capture runs the callable once too, recording instead of launching

    def replay(self):
        self.fn()


class BrokenGraph(FakeGraph):
    def capture(self, fn):
        raise RuntimeError("capture refused (test)")


class Owner(CAP.Captured):
    """A captured path whose work logs which tensors it ran on and whether the handle cache was pinning."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.calls, self.pinning = [], []

    def _work(self, x, y=None, scale=1.0):
        self.calls.append((x, y, scale))
        self.pinning.append(models._graphs.pin is not None)
        return x * scale


@pytest.fixture
def fake(monkeypatch):
    FakeGraph.made = 0
    monkeypatch.setattr(CAP, "_new_graph", FakeGraph)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)


def test_capture_on_third_call_then_replay_from_static_buffers(fake, monkeypatch):
    w = Owner()
    x = torch.arange(3.0)
    for i in range(2):
        xi = x + i
        assert torch.equal(w._run(xi, scale=2.0), xi * 2)
        assert not w.graph_active and FakeGraph.made == 0 and w.calls[-1] == (xi, None, 2.0)
    out = w._run(x + 2, scale=2.0)
    assert w.graph_active and FakeGraph.made == 1 and w.launch_mode == "hipGraph replay"
    assert out is w._result and torch.equal(out, x + 2)  # keyword arguments reach the eager calls only
    assert len(w.calls) == 4 and all(c[0] is w._static[0] and c[2] == 1.0 for c in w.calls[2:])
    assert w.pinning == [False, False, True, False]  # the handle cache pins during the capture only
    assert models._graphs.pin is None

    # new inputs are copied into the static buffers before the replay
    assert w._run(x + 5) is w._result
    assert torch.equal(w._static[0], x + 5) and w.calls[-1][0] is w._static[0] and FakeGraph.made == 1

    # the static buffers passed back are not copied onto themselves
    copies = []
    real_copy = torch.Tensor.copy_
    monkeypatch.setattr(torch.Tensor, "copy_", lambda self, src, *a: copies.append(self) or real_copy(self, src, *a))
    w._static[0].fill_(7.0)
    w._run(w._static[0])
    assert copies == [] and torch.equal(w._static[0], torch.full((3,), 7.0))
    w._run(x)
    assert len(copies) == 1 and copies[0] is w._static[0]


def test_step_policy_other_shapes_run_eagerly_and_keep_the_graph(fake):
    w = Owner()
    x, y = torch.ones(3), torch.ones(2)
    for _ in range(3):
        w._run(x, y)
    graph = w._graph
    x4 = torch.ones(4)
    assert torch.equal(w._run(x4, y), x4) and w.calls[-1][0] is x4
    y5 = torch.ones(5)
    w._run(x, y5)
    assert w.calls[-1][1] is y5
    assert w._graph is graph and FakeGraph.made == 1
    w._run(x, y)
    assert w.calls[-1][0] is w._static[0]  # the next batch of the captured shapes replays

    # reset_graph() drops the graph and restarts the warm-up count
    w.reset_graph()
    assert not w.graph_active
    w._run(x, y), w._run(x, y)
    assert not w.graph_active
    w._run(x, y)
    assert w.graph_active and FakeGraph.made == 2


def test_rollout_policy_new_signature_warms_up_and_recaptures(fake):
    w = Owner(recapture=True)
    x = torch.ones(1, 3)
    for _ in range(3):
        w._run(x, None)
    assert w.graph_active and FakeGraph.made == 1
    x2 = torch.ones(2, 3)
    for _ in range(2):  # two eager calls for the new signature
        assert w._run(x2, None) is not w._result
        assert not w.graph_active and w.calls[-1][0] is x2
    w._run(x2, None)
    assert w.graph_active and FakeGraph.made == 2 and w._static[0].shape == x2.shape
    # an argument that appears (None -> tensor) is a new signature too
    w._run(x2, torch.ones(3))
    assert not w.graph_active
    # a signature change during the warm-up restarts it
    w._run(x, None), w._run(x2, None), w._run(x2, None)
    assert not w.graph_active
    w._run(x2, None)
    assert w.graph_active and FakeGraph.made == 3


def test_failed_capture_raises_when_the_graph_is_required(fake, monkeypatch):
    monkeypatch.setattr(CAP, "_new_graph", BrokenGraph)
    w = Owner(required=True)
    x = torch.ones(3)
    w._run(x), w._run(x)
    with pytest.raises(RuntimeError, match=r"Owner\(use_graph=True\): hipGraph capture failed"):
        w._run(x)
    assert models._graphs.pin is None
    assert not w.use_graph and not w.graph_active and "capture refused (test)" in w.capture_error


def test_failed_optional_capture_warns_once_and_stays_eager(fake, monkeypatch):
    monkeypatch.setattr(CAP, "_new_graph", BrokenGraph)
    w = Owner()
    x = torch.ones(3)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for i in range(6):
            xi = x + i
            assert torch.equal(w._run(xi), xi) and w.calls[-1][0] is xi
    msgs = [str(c.message) for c in caught if issubclass(c.category, RuntimeWarning)]
    assert len(msgs) == 1 and "hipGraph capture unavailable" in msgs[0]
    assert models._graphs.pin is None
    assert not w.graph_active and w.launch_mode.startswith("eager (capture failed")
    assert BrokenGraph.made == 1 and len(w.calls) == 6


def test_capture_error_is_cut_at_300_characters(fake, monkeypatch):
    class LongError(FakeGraph):
        def capture(self, fn):
            raise ValueError("x" * 1000)

    monkeypatch.setattr(CAP, "_new_graph", LongError)
    w = Owner()
    with pytest.warns(RuntimeWarning, match="hipGraph capture unavailable"):
        for _ in range(3):
            w._run(torch.ones(3))
    assert w.capture_error == "ValueError: " + "x" * 300


def test_disabled_path_is_always_eager(fake):
    w = Owner(use_graph=False)
    for _ in range(5):
        w._run(torch.ones(3))
    assert FakeGraph.made == 0 and not w.graph_active and w.launch_mode == "eager" and len(w.calls) == 5


def test_graph_enabled_reads_gcl_no_graph(monkeypatch):
    monkeypatch.delenv("GCL_NO_GRAPH", raising=False)
    assert CAP.graph_enabled(None) and CAP.graph_enabled(True) and not CAP.graph_enabled(False)
    monkeypatch.setenv("GCL_NO_GRAPH", "1")
    assert not CAP.graph_enabled(None) and CAP.graph_enabled(True)
    monkeypatch.setenv("GCL_NO_GRAPH", "0")
    assert CAP.graph_enabled(None)
