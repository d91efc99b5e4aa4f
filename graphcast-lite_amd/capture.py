"""hipGraph capture and replay of the captured paths (`TrainStep`, `DualMeshCachedStep`, `CapturedRollout`,
`CapturedAssimilatedRollout`): a few hundred kernel launches cost the host one graph launch."""
import os
import warnings

import torch

from . import models


def graph_enabled(use_graph) -> bool:
    """The steps' `use_graph` argument: True / False as given, None = on unless GCL_NO_GRAPH is set (to non-0)."""
    if use_graph is None:
        return os.environ.get("GCL_NO_GRAPH", "0") in ("0", "")
    return bool(use_graph)


class _HipGraph(torch.cuda.CUDAGraph):
    def capture(self, fn):
        # thread_local: other threads of the process (the RCCL watchdog) may touch the runtime meanwhile
        with torch.cuda.graph(self, capture_error_mode="thread_local"):
            return fn()


_new_graph = _HipGraph  # the one place a graph is made


class Captured:
    """Base of the captured paths.  A subclass defines `_work(*args, **kw)` and calls `self._run(*args, **kw)`.

    `_work` runs eagerly for the first `warmup` calls (workspaces, CSR handles, kernel attributes, allocator pools and
    the RCCL communicator get set up outside the capture).  The next call captures `_work` into a hipGraph over static
    copies of `args` (tensors or None; `kw` reach the eager calls only), and later calls copy their `args` into those
    buffers (not when they are the buffers themselves) and replay.  A replay returns what `_work` returned at the
    capture.

    After the capture a call whose argument shapes differ from the captured ones runs eagerly and keeps the graph; with
    `recapture` any change of the argument shapes drops the graph and restarts the warm-up.  A failed capture raises
    when the graph is `required`, else warns once and stays eager for good (`use_graph` turns False)."""

    warmup = 2

    def __init__(self, use_graph: bool = True, required: bool = False, recapture: bool = False):
        self.use_graph, self._graph_required, self._recapture = use_graph, required, recapture
        self.capture_error, self._sig = None, None
        self.reset_graph()

    def reset_graph(self):
        """Drop the graph: the next `warmup` calls run eagerly, the one after captures again."""
        self._graph = self._static = self._result = self._pinned = None
        self._calls = 0

    @property
    def graph_active(self) -> bool:
        """True while calls are replayed from a captured hipGraph."""
        return self._graph is not None

    @property
    def launch_mode(self) -> str:
        if self.graph_active:
            return "hipGraph replay"
        return "eager" + (f" (capture failed: {self.capture_error})" if self.capture_error else "")

    def _capture(self, *args):
        self._static = [None if a is None else a.clone() for a in args]
        graph = _new_graph()
        with models._graphs.pinning() as pinned:  # the CSR handles the captured kernels point into
            self._result = graph.capture(lambda: self._work(*self._static))
        self._graph, self._pinned = graph, pinned

    def _run(self, *args, **kw):
        if not self.use_graph:
            return self._work(*args, **kw)
        sig = [None if a is None else a.shape for a in args]
        if self._recapture and sig != self._sig:
            self.reset_graph()
        if self._graph is None:
            self._sig = sig
            if self._calls < self.warmup:
                self._calls += 1
                return self._work(*args, **kw)
            try:
                self._capture(*args)
            except Exception as e:
                self.use_graph, self.capture_error = False, f"{type(e).__name__}: {str(e)[:300]}"
                self.reset_graph()
                torch.cuda.synchronize()
                owner = type(self).__name__
                if self._graph_required:  # the caller asked for the graph path explicitly: no silent degradation
                    raise RuntimeError(f"{owner}(use_graph=True): hipGraph capture failed ({self.capture_error})") from e
                warnings.warn(f"[{owner}] hipGraph capture unavailable ({self.capture_error}); staying eager "
                              f"(see .launch_mode / .graph_active)", RuntimeWarning)
                return self._work(*args, **kw)
            # the capture only records: the replay below performs this call
        elif sig != self._sig:
            return self._work(*args, **kw)
        else:
            for a, s in zip(args, self._static):
                if a is not None and a.data_ptr() != s.data_ptr():
                    s.copy_(a)
        self._graph.replay()
        return self._result
