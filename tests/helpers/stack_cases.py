"""One eager training step of a model with every library entry it calls written down, and the cases whose entry lists
tests/golden/stack_launches.json holds (tests/test_stack_plan.py).

`recording()` puts a proxy around the loaded library (`hip._lib`) that appends the name of every `gcl_*` entry called
through it.  Left out: queries (`*_ok`, `*_ws_bytes`), counters (`*_launches`), `gcl_last_error`, `gcl_version`, and the
host-side graph set-up and getters (`gcl_graph_*`: a graph's `__del__` calls one whenever the collector runs, so they
come at no fixed place).  Nothing here looks at functional.py's internals, so the same code records a commit from before
the stack plan existed."""
import contextlib
import os

import torch

DEV = "cuda:0"
ENV_SWITCHES = ("GCL_FUSED_GCN", "GCL_NO_ROW_SKIP", "GCL_NO_SPLIT_OUT", "GCL_NO_SPLIT_GRAD", "GCL_NO_COMPACT_STORE",
                "GCL_NO_LOSS_GRAD_INPLACE")


def _case(name, levels, B, nlat=32, nlon=64, env=None, functional=None, model=None):
    return dict(name=name, levels=levels, B=B, nlat=nlat, nlon=nlon, env=env or {}, functional=functional or {},
                model=model or {})


# id -> case.  env: variables set for the step; functional / model: attributes set on the module / on the model.
CASES = {
    "baseline_12_B3": _case("baseline", [1, 2], 3),
    "baseline_35_B3": _case("baseline", [3, 5], 3),
    "attention_12_B3": _case("attention", [1, 2], 3),
    "baseline_12_grid63x31": _case("baseline", [1, 2], 3, nlat=31, nlon=63),
    "baseline_12_B1": _case("baseline", [1, 2], 1),
    "wb2_19f_ar_12_B2": _case("wb2_512x256_19f_ar", [1, 2], 2),
    "off_fused_gcn": _case("baseline", [1, 2], 3, env={"GCL_FUSED_GCN": "0"}),
    "off_row_skip": _case("baseline", [1, 2], 3, env={"GCL_NO_ROW_SKIP": "1"}),
    "off_split_out": _case("baseline", [1, 2], 3, env={"GCL_NO_SPLIT_OUT": "1"}),
    "off_split_grad": _case("baseline", [1, 2], 3, env={"GCL_NO_SPLIT_GRAD": "1"}),
    "off_compact_store": _case("baseline", [1, 2], 3, env={"GCL_NO_COMPACT_STORE": "1"}),
    "off_loss_grad_inplace": _case("baseline", [1, 2], 3, env={"GCL_NO_LOSS_GRAD_INPLACE": "1"}),
    "off_ln_colsum": _case("baseline", [1, 2], 3, functional={"_LN_COLSUM": False}),
    "off_rows_out": _case("baseline", [1, 2], 3, functional={"_ROWS_OUT": False}),
    "off_row_skip_35": _case("baseline", [3, 5], 3, env={"GCL_NO_ROW_SKIP": "1"}),  # (at [1, 2] every mesh row has a reader)
    "off_ln_colsum_35": _case("baseline", [3, 5], 3, functional={"_LN_COLSUM": False}),
    "off_lat_table": _case("baseline", [1, 2], 3, model={"_lat_through_table": False}),
    "off_grad_landing": _case("baseline", [1, 2], 3, model={"_grad_landing": False}),
}


def is_launch(name: str) -> bool:
    return name.startswith("gcl_") and not (name.endswith(("_ok", "_ws_bytes", "_launches")) or name.startswith("gcl_graph_")
                                            or name in ("gcl_last_error", "gcl_version"))


class _Recorder:
    def __init__(self, lib, names):
        self._lib, self._names, self._wrapped = lib, names, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not is_launch(name):
            return fn
        w = self._wrapped.get(name)
        if w is None:
            def w(*a, _fn=fn, _name=name):
                self._names.append(_name)
                return _fn(*a)
            self._wrapped[name] = w
        return w


@contextlib.contextmanager
def recording():
    """-> the list that the entry names are appended to while the block runs."""
    from graphcast_lite_amd import hip

    real, names = hip.lib(), []
    hip._lib = _Recorder(real, names)
    try:
        yield names
    finally:
        hip._lib = real


@contextlib.contextmanager
def switched(case, model):
    """The case's switches set, every other one of ENV_SWITCHES unset; all put back afterwards."""
    from graphcast_lite_amd import functional

    env0 = {k: os.environ.pop(k, None) for k in ENV_SWITCHES}
    os.environ.update(case["env"])
    old = [(obj, k, getattr(obj, k), k in vars(obj)) for obj, attrs in ((functional, case["functional"]), (model, case["model"]))
           for k in attrs]
    for obj, attrs in ((functional, case["functional"]), (model, case["model"])):
        for k, v in attrs.items():
            assert hasattr(obj, k), k
            setattr(obj, k, v)
    try:
        yield
    finally:
        for obj, k, v, own in old:
            setattr(obj, k, v) if own else delattr(obj, k)
        for k, v in env0.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def build(case):
    """(model, X, y) of a case on the device, seeded as tests/test_hip_model.py seeds its pairs."""
    from test_hip_model import data, make_pair

    cfg, m, _ = make_pair(case["name"], case["levels"], nlat=case["nlat"], nlon=case["nlon"])
    X, y = data(cfg, m._num_grid_nodes, case["B"])
    return m, X.to(DEV), y.to(DEV)


def step(m, X, y):
    """Two forwards and one backward, as tests/test_encoder_output_split.py::_step: (prediction, loss, gradients)."""
    from graphcast_lite_amd.train import batch_loss

    m.zero_grad()
    out = m(X).detach().clone()
    loss = batch_loss(m, X, y)
    loss.backward()
    torch.cuda.synchronize()
    return out, loss.detach().clone(), {n_: p.grad.clone() for n_, p in m.named_parameters()}


def run_case(case):
    """-> ((prediction, loss, gradients), entry names) of one step of a fresh model."""
    m, X, y = build(case)
    with switched(case, m), recording() as names:
        res = step(m, X, y)
    return res, names
