"""linear_x3_bwd_lean_kernel: the fused dense backward without the code of what the caller did not ask for (activation
and slope gradient, db, column sums of dX, the masks of a partial last float4).  It shares its body with
linear_x3_bwd_kernel, which tests every request at run time and serves GCL_X3_BWD_LEAN=0: every output of every reachable
combination must be torch.equal between the two, and a call that asks for both column sums (with an activation: for
everything) must still launch linear_x3_bwd_kernel."""
import itertools

import pytest
import torch

from helpers.layouts import SENT, Guarded, has, launched, randn, targs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NUM_CU = 256
SWITCH = "GCL_X3_BWD_LEAN"
SHAPES = {"64x64": (64, 64, 64), "36x16": (36, 16, 16), "64x33_ld36": (64, 33, 36)}  # Fin, Fout, row stride of dy
ROWS = [1, 63, 65, 2 * NUM_CU * 64 + 65]
# (activation, slope gradient, db, column sums): the slope gradient needs the activation
COMBOS = [c for c in itertools.product([False, True], repeat=4) if c[0] or not c[1]]


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


@pytest.fixture(autouse=True)
def _defaults(monkeypatch):
    for k in (SWITCH, "GCL_X3", "GCL_NO_FUSED64", "GCL_NO_FUSED_BWD"):
        monkeypatch.delenv(k, raising=False)


def _operands(rows, Fin, Fout, ldy, seed):
    dyw = randn(rows, ldy, seed=seed)  # (the padding columns of dy hold finite junk)
    return dyw[:, :Fout], randn(Fout, Fin, seed=seed + 1) / 8, randn(rows, Fin, seed=seed + 2), torch.tensor([0.25], device=DEV)


def _call(hip, ops, combo, acc=False, init=None):
    """One hip.linear_bwd_all -> {name: tensor} of dx and every destination (Guarded: a sentinel frame around each)."""
    dy, W, x, slope = ops
    act, want_slope, want_db, want_cs = combo
    Fout, Fin = W.shape
    init = init or {}
    dst = {"dW": Guarded((Fout, Fin), init=init.get("dW")), "dsl": Guarded((1,), init=init.get("dsl")),
           "db": Guarded((Fout,), init=init.get("db")), "cs": Guarded((Fin,), init=init.get("cs"))}
    for k, g in dst.items():
        if k not in init:
            g.view.fill_(SENT)
    # a slope destination without an activation is passed on purpose: nothing may be written to it
    dx = hip.linear_bwd_all(dy, W, x, slope if act else None, dst["dsl"].view if (want_slope or not act) else None,
                            dst["dW"].view, dst["db"].view if want_db else None, dst["cs"].view if want_cs else None, acc,
                            act=hip.ACT_PRELU if act else hip.ACT_NONE)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in dst.values()), "written outside a destination"
    out = {k: g.view.clone() for k, g in dst.items()}
    out["dx"] = dx
    return out, {"dsl": want_slope, "db": want_db, "cs": want_cs, "dW": True, "dx": True}


def _compare(hip, monkeypatch, ops, combo, what, acc=False, init=None):
    new, wanted = _call(hip, ops, combo, acc, init)
    monkeypatch.setenv(SWITCH, "0")
    old, _ = _call(hip, ops, combo, acc, init)
    monkeypatch.delenv(SWITCH)
    for k, want in wanted.items():
        if want:
            assert bool(torch.isfinite(new[k]).all()) and torch.equal(new[k], old[k]), f"{what}: {k} differs from the full kernel"
        else:
            kept = init[k] if (init and k in init) else torch.full_like(new[k], SENT)
            assert torch.equal(new[k], kept), f"{what}: {k} was not requested but written"


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_combination_equals_the_full_kernel(hip, monkeypatch, shape, rows):
    Fin, Fout, ldy = SHAPES[shape]
    ops = _operands(rows, Fin, Fout, ldy, seed=rows % 97 + Fin)
    for combo in COMBOS:
        _compare(hip, monkeypatch, ops, combo, f"{shape} rows={rows} act/slope/db/cs={combo}")


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_kernel_that_ran(hip, monkeypatch, shape):
    Fin, Fout, ldy = SHAPES[shape]
    NO = "2" if Fout > 32 else "1"
    ops = _operands(65, Fin, Fout, ldy, seed=3)
    b = lambda v: "true" if v else "false"  # noqa: E731
    for combo in COMBOS:
        act, _, want_db, want_cs = combo
        _, names = launched(lambda: _call(hip, ops, combo))
        lean = targs(names, "linear_x3_bwd_lean_kernel")
        if want_db and want_cs:  # both column sums: the full kernel, with or without an activation
            assert lean == [] and targs(names, "linear_x3_bwd_kernel") == [[NO]], (combo, names)
        else:
            assert lean == [[NO, b(act), b(want_db), b(want_cs), b(Fout % 4 != 0)]], (combo, names)
            assert not has(names, "linear_x3_bwd_kernel<"), (combo, names)
        monkeypatch.setenv(SWITCH, "0")
        _, names = launched(lambda: _call(hip, ops, combo))
        monkeypatch.delenv(SWITCH)
        assert targs(names, "linear_x3_bwd_kernel") == [[NO]] and not has(names, "linear_x3_bwd_lean_kernel"), (combo, names)


@pytest.mark.parametrize("gate", ["GCL_X3", "GCL_NO_FUSED64", "GCL_NO_FUSED_BWD"])
def test_the_gates_of_the_full_kernel_hold_for_the_lean_one(hip, monkeypatch, gate):
    monkeypatch.setenv(gate, "0" if gate == "GCL_X3" else "1")
    _, names = launched(lambda: _call(hip, _operands(65, 64, 64, 64, seed=4), (False, False, False, False)))
    assert not has(names, "linear_x3_bwd"), names


@pytest.mark.parametrize("which", ["dW", "db", "cs", "dsl"])
def test_accumulate_bits(hip, monkeypatch, which):
    """Each destination's accumulate flag, against the full kernel (hip.linear_bwd_all gives all three the flag of dW)."""
    combo = {"dW": (False, False, False, False), "db": (False, False, True, False), "cs": (False, False, False, True),
             "dsl": (True, True, False, False)}[which]
    ops = _operands(193, 64, 64, 64, seed=8)
    init = {"dW": randn(64, 64, seed=1), "db": randn(64, seed=2), "cs": randn(64, seed=3), "dsl": randn(1, seed=4)}
    _compare(hip, monkeypatch, ops, combo, f"accumulate into {which}", acc=True, init=init)
    new, _ = _call(hip, ops, combo, True, init)
    fresh, _ = _call(hip, ops, combo, False)
    assert not torch.equal(new[which], fresh[which]), "the accumulate flag changed nothing"
