"""A GCNConv stack decides its path once (stack_plan.plan_gcn_stack) and its backward reads the decision.

On the GPU: one eager training step per case of helpers/stack_cases.py calls the library's entries in the order recorded
from the commit before the plan existed (golden/stack_launches.json), every stack's forward calls exactly the entries its
plan names, and together the cases reach every ConvStep kind, every LayerNorm form and every form of incoming gradient.
Without a GPU: the plan's answers on stand-in layouts, where no library query is needed."""
import json
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import stack_cases as SC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_launches.json")
CONV_ENTRIES = {"tab": ["gcl_gcn_layer_fwd_tab"], "split": ["gcl_gcn_layer_fwd_split"],
                "two_kernel_padded": ["gcl_dense_fwd", "gcl_aggregate"], "two_kernel": ["gcl_dense_fwd", "gcl_aggregate"]}
LN_ENTRIES = {None: [], "dense": ["gcl_layernorm_fwd"], "mapped": ["gcl_layernorm_fwd_map"],
              "mapped_skip": ["gcl_layernorm_fwd_map_skip"]}


def forward_entries(plan):
    """The entries a stack's forward calls, as its plan names them."""
    names = []
    for st in plan.convs:
        names += CONV_ENTRIES.get(st.kind) or ["gcl_gcn_layer_fwd_present" if st.present else "gcl_gcn_layer_fwd_rows"]
    return names + LN_ENTRIES[plan.ln]


@pytest.fixture(scope="module")
def runs(lib_built):
    """case id -> (entry names of the step, [(plan, entries of that stack's forward)], [kind of incoming gradient]): every
    case runs once, with GCNStackFn.forward and the backward's classifier watched."""
    from graphcast_lite_amd import functional as F

    fwd0, inc0, out = F.GCNStackFn.forward, F._incoming_grad, {}
    for cid, case in SC.CASES.items():
        stacks, kinds, cur = [], [], []

        def fwd(ctx, *a):
            i0 = len(cur[0])
            res = fwd0(ctx, *a)
            stacks.append((ctx.plan, cur[0][i0:]))
            return res

        def inc(*a):
            g = inc0(*a)
            kinds.append(g.kind)
            return g

        F.GCNStackFn.forward, F._incoming_grad = staticmethod(fwd), inc
        try:
            m, X, y = SC.build(case)
            with SC.switched(case, m), SC.recording() as names:
                cur.append(names)
                SC.step(m, X, y)
        finally:
            F.GCNStackFn.forward, F._incoming_grad = staticmethod(fwd0), inc0
        out[cid] = (names, stacks, kinds)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(SC.CASES))
def test_step_calls_the_recorded_entries(runs, cid):
    with open(GOLDEN) as fh:
        want = json.load(fh)[cid]
    assert runs[cid][0] == want


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(SC.CASES))
def test_each_stack_calls_what_its_plan_names(runs, cid):
    _, stacks, kinds = runs[cid]
    assert len(stacks) == 2 * len(kinds) >= 4  # encoder and decoder at least: two forwards and one backward each
    for plan, names in stacks:
        assert names == forward_entries(plan), plan


@pytest.mark.gpu
def test_cases_reach_every_branch(runs):
    plans = [p for _, stacks, _ in runs.values() for p, _ in stacks]
    assert {st.kind for p in plans for st in p.convs} == {"tab", "split", "fused", "two_kernel_padded", "two_kernel"}
    assert {p.ln for p in plans} == {None, "dense", "mapped", "mapped_skip"}
    assert {k for _, _, kinds in runs.values() for k in kinds} == {"dense", "mapped", "parts", "wide"}
    assert any(p.split_reader and not p.split_store for p in plans) and any(p.split_store and not p.split_reader for p in plans)
    assert any(st.rows_out for p in plans for st in p.convs) and any(p.enc_shape is not None for p in plans)


# ------------------------------------------------------------------------------------------------------------------
# the plan alone (no GPU): a stand-in graph inside the one-kernel layer's range, so no library query is asked
# ------------------------------------------------------------------------------------------------------------------
def _plan(widths, Fin=64, B=3, n=96, has_ln=False, out_rows=0, land=None, lat=None, squeeze=False, sw=None):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd.stack_plan import Layout, Switches, plan_gcn_stack

    graph = types.SimpleNamespace(max_in_degree=8, kind=hip.GRAPH_GCN, n=n)
    shapes = [(Fo, Fi) for Fi, Fo in zip([Fin] + widths[:-1], widths)]
    x = Layout.dense(B, n if lat is None else 40, Fin)
    return plan_gcn_stack(x, None, squeeze, shapes, graph, has_ln, out_rows, land, lat, None, sw or Switches(True, True, True, True))


class _Land:
    """GradLanding's ln_plan for a decoder input 64 wide that reads `readers` of the rows."""

    def __init__(self, readers):
        self.readers, self.table = readers, torch.zeros(1, dtype=torch.int32)

    def ln_plan(self, n, F, may_skip):
        return (True, self.table if may_skip and self.readers < n else None) if F == 64 else (False, None)


@pytest.fixture
def fused_on(monkeypatch):
    monkeypatch.delenv("GCL_FUSED_GCN", raising=False)


def test_plan_kinds_follow_the_layouts_between_the_layers(fused_on, monkeypatch):
    kinds = lambda p: [st.kind for st in p.convs]  # noqa: E731
    plan, out_head, present = _plan([64, 64, 64])
    assert kinds(plan) == ["fused"] * 3 and plan.ln is None and plan.padded_last is None and out_head is None and present is None
    assert not any(st.dense_after or st.present or st.rows_out for st in plan.convs)
    # a width past the one-kernel layer's range; an odd width in the middle is copied dense and refused by the next gate
    assert kinds(_plan([128, 64])[0]) == ["two_kernel", "two_kernel"]
    plan = _plan([64, 33, 64])[0]
    assert kinds(plan) == ["fused", "fused", "two_kernel"] and [st.dense_after for st in plan.convs] == [False, True, False]
    # an odd last width stays padded when nothing follows it, in either implementation; a LayerNorm reads dense rows
    plan = _plan([64, 19], out_rows=32)[0]
    assert kinds(plan) == ["fused", "fused"] and plan.padded_last == (20, 19, False) and plan.out_rows == 32
    assert plan.convs[1].rows_out == 32 and not plan.convs[1].dense_after
    assert _plan([64, 19], out_rows=32, sw=_sw(rows_out=False))[0].convs[1].rows_out is None
    assert _plan([64, 19], out_rows=96)[0].out_rows == 0  # (all rows: no slice)
    plan = _plan([64, 19], has_ln=True)[0]
    assert plan.padded_last is None and plan.convs[1].dense_after and plan.ln == "dense"
    monkeypatch.setenv("GCL_FUSED_GCN", "0")
    plan = _plan([64, 19])[0]
    assert kinds(plan) == ["two_kernel", "two_kernel_padded"] and plan.padded_last == (20, 19, True)
    lat = types.SimpleNamespace(M=96, tail=None)
    plan = _plan([64, 64], lat=lat)[0]  # (the row-table layer has no two-kernel form: the switch leaves it)
    assert kinds(plan) == ["tab", "two_kernel"] and plan.n == 96


def _sw(**kw):
    from graphcast_lite_amd.stack_plan import Switches

    return Switches(True, True, True, True)._replace(**kw)


def test_plan_layernorm_forms(fused_on):
    plan, _, present = _plan([64, 64], has_ln=True, land=_Land(readers=50))
    assert plan.ln == "mapped_skip" and plan.landing and plan.convs[-1].present and present is not None
    assert not plan.convs[0].present
    for sw in (_sw(row_skip=False), _sw(ln_colsum=False)):
        plan, _, present = _plan([64, 64], has_ln=True, land=_Land(readers=50), sw=sw)
        assert plan.ln == "mapped" and present is None and not plan.convs[-1].present and plan.ln_colsum == sw.ln_colsum
    assert _plan([64, 64], has_ln=True, land=_Land(readers=96))[0].ln == "mapped"
    plan = _plan([64, 48], has_ln=True, land=_Land(readers=50))[0]
    assert plan.ln == "dense" and plan.landing  # (another width than the decoder's input: announced, not mapped)
    for kw in (dict(squeeze=True), dict(out_rows=32)):  # the landing serves whole batched outputs only
        plan = _plan([64, 64], has_ln=True, land=_Land(readers=50), **kw)[0]
        assert plan.ln == "dense" and not plan.landing
    assert _plan([64, 64], land=_Land(readers=50))[0].ln is None


def test_a_step_refuses_a_layout_its_plan_did_not_assume():
    from graphcast_lite_amd import functional as F

    t = torch.zeros(2, 8, 12)
    F._expect_dense(t, 2, 8, 12)
    for bad in (t[:, :, :8], t[:, :4], t.transpose(0, 1), t.view(-1)[1:1 + 2 * 8 * 8].view(2, 8, 8)):
        with pytest.raises(RuntimeError, match="plan assumed"):
            F._expect_dense(bad, *bad.shape)
    F._expect_dense(t.view(-1)[1:1 + 2 * 8 * 8].view(2, 8, 8), 2, 8, 8, aligned=False)
