"""The epoch functions of `graphcast_lite_amd.regional_train` against the reference's OWN `train_dual_epoch` /
`eval_dual` (scripts/train_dual_mesh.py) and `train_epoch` / `eval_epoch` (scripts/train_roi_residual.py), recorded in
tests/golden/regional_train_vectors.npz by tests/golden/make_regional_train_golden.py: two epochs over three samples
with torch's Adam around the reference's `DualMeshModel` / `ROIResidualModel` and the linear stub global model of
tests/helpers/regional_case.py (5-degree box, hidden 32).

Tolerance: 1e-4 relative on the losses and on the parameter norms, the bar tests/test_dual_mesh.py applies to these same
steps against torch Adam; the correction skill is a difference of two such losses relative to one of them: 2e-4 absolute."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from regional_case import LinearStubGlobal  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_Z = None


def _fx():
    global _Z
    if _Z is None:
        _Z = np.load(os.path.join(GOLDEN, "regional_train_vectors.npz"))
    return _Z


def _model(z):
    from graphcast_lite_amd.dual_mesh import DualMeshModel

    C, obs, D, hidden, steps, k, level = (int(v) for v in z["dims"])
    stub = LinearStubGlobal(C, obs, D, z["global_lats"], z["global_lons"])
    m = DualMeshModel(stub, tuple(z["roi"]), z["grid_lats"], z["grid_lons"], torch.device(DEV), reg_mesh_level=level,
                      reg_mesh_buffer=float(z["buffer"]), reg_processor_steps=steps, cross_k=k, hidden_dim=hidden)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if not n.startswith("global_model."):
                p.copy_(torch.from_numpy(z["w0:" + n]))
    return m


def _data(z, split, n):
    return [(torch.from_numpy(z[f"{split}_X{i}"]), torch.from_numpy(z[f"{split}_y{i}"])) for i in range(n)]


def _close(got, want, rel=1e-4):
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("name,cached,residual,ar", [("cached", True, True, 1), ("std_ar1", False, False, 1),
                                                     ("std_ar2", False, True, 2)])
def test_epochs_match_the_reference_run(name, cached, residual, ar):
    from graphcast_lite_amd.regional_train import DualMeshCacheStep, GlobalOutputCache, eval_dual, train_dual_epoch
    from graphcast_lite_amd.train import TrainStep

    z = _fx()
    m = _model(z)
    train, val = _data(z, "train", 3), _data(z, "val", 2)
    lr = float(z["lr"])
    tc = vc = None
    if cached:
        tc = GlobalOutputCache.build(m, train, "train", log=lambda s: None)
        vc = GlobalOutputCache.build(m, val, "val", log=lambda s: None)
        step = DualMeshCacheStep(m, tc, lr=lr, use_residual=residual)
    else:
        step = TrainStep(m, lr=lr, spatial_mask=m.roi_mask.view(1, -1, 1).float(), use_residual=residual, ar_steps=ar)
    for epoch in range(2):
        tl = train_dual_epoch(m, train, step, DEV, use_residual=residual, current_ar_steps=ar, cache=tc, say=lambda s: None)
        vl, skill = eval_dual(m, val, DEV, use_residual=residual, current_ar_steps=ar, cache=vc)
        want_t, (want_v, want_s) = float(z[f"{name}:train_loss"][epoch]), z[f"{name}:eval"][epoch]
        print(f"{name} epoch {epoch}: train {tl!r} / {want_t!r}, val {vl!r} / {want_v!r}, skill {skill!r} / {want_s!r}")
        assert _close(tl, want_t) and _close(vl, want_v) and abs(skill - want_s) <= 2e-4, (epoch, tl, vl, skill)
    for n, p in m.named_parameters():
        if not n.startswith("global_model."):
            ref = torch.from_numpy(z[f"{name}:w:{n}"]).double()
            err = (p.detach().cpu().double() - ref).norm().item()
            assert err <= 1e-4 * ref.norm().item(), (n, err, ref.norm().item())
    if name == "std_ar2":  # the final weights scored with one static and one forcing channel
        vl, skill = eval_dual(m, val, DEV, use_residual=True, current_ar_steps=2, static_channels=[1], forcing_channels=[3])
        want_v, want_s = z["eval_special"]
        assert _close(vl, want_v) and abs(skill - want_s) <= 2e-4, (vl, skill, want_v, want_s)


def test_roi_epochs_match_the_reference_run():
    """`train_epoch` / `eval_epoch` of scripts/train_roi_residual.py; the ACC is a correlation, held to 1e-4 absolute, and
    the `[Correction]` line to the recorded print within its printed precision."""
    import re

    from graphcast_lite_amd.regional_train import eval_roi_epoch, train_roi_epoch
    from graphcast_lite_amd.roi_residual import ROIResidualModel
    from graphcast_lite_amd.train import TrainStep

    z = _fx()
    C, obs, D, hidden = (int(v) for v in z["dims"][:4])
    steps, k = (int(v) for v in z["roi:dims"])
    stub = LinearStubGlobal(C, obs, D, z["global_lats"], z["global_lons"])
    m = ROIResidualModel(stub, tuple(z["roi"]), z["grid_lats"], z["grid_lons"], torch.device(DEV), hidden_dim=hidden,
                         processor_steps=steps, roi_k=k)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if not n.startswith("global_model."):
                p.copy_(torch.from_numpy(z["roi:w0:" + n]))
    train, val = _data(z, "train", 3), _data(z, "val", 2)
    step = TrainStep(m, lr=float(z["roi:lr"]), spatial_mask=m.roi_mask.view(1, -1, 1).float(), use_residual=False)
    num = re.compile(r"mean_abs=(\S+), max_abs=(\S+), baseline_mse=(\S+)$")
    for epoch in range(2):
        said = []
        tl = train_roi_epoch(m, train, step, DEV, say=said.append)
        vl, acc = eval_roi_epoch(m, val, DEV)
        want_t, (want_v, want_a) = float(z["roi:train_loss"][epoch]), z["roi:eval"][epoch]
        print(f"roi epoch {epoch}: train {tl!r} / {want_t!r}, val {vl!r} / {want_v!r}, ACC {acc!r} / {want_a!r}; {said[-1]}")
        assert _close(tl, want_t) and _close(vl, want_v) and abs(acc - want_a) <= 1e-4, (epoch, tl, vl, acc)
        got = [float(v) for v in num.search(said[-1]).groups()]
        want = [float(v) for v in num.search(str(z["roi:correction_lines"][epoch])).groups()]
        for a, b, digit in zip(got, want, (1e-6, 1e-4, 1e-6)):
            assert abs(a - b) <= 1.01 * digit + 1e-4 * abs(b), (said[-1], z["roi:correction_lines"][epoch])
    for n, p in m.named_parameters():
        if not n.startswith("global_model."):
            ref = torch.from_numpy(z["roi:w:" + n]).double()
            err = (p.detach().cpu().double() - ref).norm().item()
            assert err <= 1e-4 * ref.norm().item(), (n, err, ref.norm().item())


# ------------------------------------------------------------------------------------------------------------------
# the scripts' main() as recorded (tests/golden/regional_main_vectors.npz)
# ------------------------------------------------------------------------------------------------------------------
_NUM = r"-?\d+\.\d+"


def _main_fx():
    return np.load(os.path.join(GOLDEN, "regional_main_vectors.npz"))


def _main_model(z, weights):
    from graphcast_lite_amd.dual_mesh import DualMeshModel

    C, obs, D, hidden, steps, k, level = (int(v) for v in z["dims"])
    stub = LinearStubGlobal(C, obs, D, z["global_lats"], z["global_lons"])
    m = DualMeshModel(stub, tuple(float(v) for v in z["roi"]), z["grid_lats"], z["grid_lons"], torch.device(DEV),
                      reg_mesh_level=level, reg_mesh_buffer=float(z["buffer"]), reg_processor_steps=steps, cross_k=k,
                      hidden_dim=hidden)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if not n.startswith("global_model."):
                p.copy_(torch.from_numpy(z[f"dual:{weights}:{n}"]))
    return m


def _split(z, name):
    X, y = torch.from_numpy(z[f"{name}_X"]), torch.from_numpy(z[f"{name}_y"])
    return [(X[i:i + 1], y[i:i + 1]) for i in range(X.shape[0])]


def _same_lines(got, want, rel, what):
    """The same text once the numbers are masked, and every number within rel (plus one unit of its last printed digit;
    percentages, which are differences of two losses over one of them, within 0.02 points + that)."""
    import re

    assert re.sub(_NUM, "#", got) == re.sub(_NUM, "#", want), (what, got, want)
    for a, b in zip(re.finditer(_NUM + "%?", got), re.finditer(_NUM + "%?", want)):
        digit = 10.0 ** -len(b.group().rstrip("%").split(".")[1])
        x, y = float(a.group().rstrip("%")), float(b.group().rstrip("%"))
        tol = 1.01 * digit + (0.02 if b.group().endswith("%") else rel * abs(y))
        assert abs(x - y) <= tol, (what, got, want)


def test_fit_dual_mesh_reproduces_the_recorded_script_run(tmp_path, capsys):
    """`scripts/train_dual_mesh.py` from its overfit test to its results: two epochs with two AR steps, the residual, a
    static and a forcing channel (the standard mode scores after the overwrite).  Losses within 1e-4, the gradient
    norms of the report within 1e-3 (they are printed to 1e-6 at sizes of 1e-3), the trained weights within 1e-4; of
    the overfit lines, which follow 200 steps at lr 0.01, the first one at 1e-4 and the text of all."""
    import json
    import re

    from graphcast_lite_amd.regional_train import fit_dual_mesh

    z = _main_fx()
    m = _main_model(z, "w0")
    out = str(tmp_path / "results")
    res = fit_dual_mesh(m, _split(z, "train"), _split(z, "val"), _split(z, "test"), out, num_epochs=2, lr=5e-4, ar_steps=2,
                        use_residual=True, static_channels=[1], forcing_channels=[3], reg_mesh_level=7)
    assert sorted(os.listdir(out)) == [str(f) for f in z["dual:files"]]
    got, want = open(os.path.join(out, "training_log.txt")).read().split("\n"), str(z["dual:log"]).split("\n")
    assert len(got) == len(want)
    for a, b in zip(got[:7], want[:7]):
        print(a, "|", b)
        _same_lines(a, b, 1e-4, "training_log.txt")
    ref = json.loads(str(z["dual:results_json"]))
    assert list(res) == list(ref)
    for k, v in ref.items():
        if isinstance(v, float):
            assert abs(res[k] - v) <= (2e-4 if "skill" in k else 1e-4 * abs(v)), (k, res[k], v)
        else:
            assert res[k] == v, k
    printed, ref_out = capsys.readouterr().out.split("\n"), str(z["dual:stdout"]).split("\n")
    pick = lambda lines, pre: [ln for ln in lines if ln.startswith(pre)]  # noqa: E731
    steps_got, steps_want = pick(printed, "    step"), pick(ref_out, "    step")
    assert len(steps_got) == len(steps_want) == 11
    _same_lines(steps_got[0], steps_want[0], 1e-4, "overfit step 0")
    for a, b in zip(steps_got, steps_want):
        assert re.sub(_NUM, "#", a) == re.sub(_NUM, "#", b)
    for pre in ("[OverfitTest]", "=" * 60, "[GradCheck]"):
        assert pick(printed, pre)[:3] == pick(ref_out, pre)[:3], pre
    for a, b in zip(pick(printed, "  ["), pick(ref_out, "  [")):
        _same_lines(a, b, 1e-3, "gradient report")
    assert len(pick(printed, "  [")) == len(pick(ref_out, "  [")) == 5
    best = torch.load(os.path.join(out, "best_regional.pth"), weights_only=True)
    assert sorted(best) == [str(k) for k in z["dual:regional_keys"]]
    for n, p in m.named_parameters():
        if not n.startswith("global_model."):
            refw = torch.from_numpy(z["dual:w:" + n]).double()
            err = (best[n].cpu().double() - refw).norm().item()
            assert err <= 1e-4 * refw.norm().item(), (n, err, refw.norm().item())


def test_predict_dual_mesh_matches_the_recorded_script_run(tmp_path):
    """`scripts/predict_dual_mesh.py --per-channel --ar-steps 2` on the weights the recorded training run saved: scores
    within 1e-4 of the script's `StreamingMetrics` objects, the printed tables the same text with numbers within that,
    and the per-horizon state equal to `verify.StreamingMetrics` fed sample by sample."""
    import json

    from graphcast_lite_amd.predict import rollout
    from graphcast_lite_amd.regional_train import predict_dual_mesh
    from graphcast_lite_amd.verify import Persistence, StreamingMetrics

    z = _main_fx()
    m = _main_model(z, "w")
    test = _split(z, "test")
    variables, std = [str(v) for v in z["variables"]], z["std"]
    said = []
    path = str(tmp_path / "results" / "predict_results.json")
    res = predict_dual_mesh(m, test, max_samples=200, ar_steps=2, use_residual=True, per_channel=True, variables=variables,
                            std=std, results_path=path, say=said.append)
    ref = json.loads(str(z["predict:results_json"]))
    assert json.load(open(path)) == json.loads(json.dumps(res)) and list(res) == list(ref)
    assert res["n_samples"] == ref["n_samples"] == 6 and res["ar_steps"] == 2 and res["roi"] == ref["roi"]
    sc, rpc, apc = z["predict:scores"], z["predict:rmse_per_channel"], z["predict:acc_per_channel"]
    objs = [res.overall[0], res.overall[1]] + [h[0] for h in res.horizons] + [h[1] for h in res.horizons]
    assert len(objs) == len(sc) == 6
    for i, o in enumerate(objs):
        assert o.n == int(sc[i][0])
        assert abs(o.rmse - sc[i][1]) <= 1e-4 * sc[i][1] and abs(o.mae - sc[i][2]) <= 1e-4 * sc[i][2], (i, o.rmse, sc[i])
        assert abs(o.acc - sc[i][3]) <= 1e-4
        assert np.all(np.abs(o.rmse_per_channel - rpc[i]) <= 1e-4 * rpc[i]) and np.all(np.abs(o.acc_per_channel - apc[i]) <= 1e-4)
    want = str(z["predict:stdout"])
    want = want[want.index("\n[predict]"):want.index("\nSaved to")].rstrip("\n").split("\n")
    assert len(said) >= 2 and len("\n".join(said[:-1]).split("\n")) == len(want)
    for a, b in zip("\n".join(said[:-1]).split("\n"), want):
        _same_lines(a, b, 1e-4, "predict tables")
    assert said[-1] == f"\nSaved to {path}"
    # the per-horizon objects against StreamingMetrics fed sample by sample
    C, rows = m.n_features, m._roi_rows.long()
    sm = [[StreamingMetrics(C), StreamingMetrics(C)] for _ in range(2)]
    with torch.no_grad():
        for X, y in test:
            X, y = X.to(DEV), y.to(DEV)
            outs = rollout(m, X, 2, use_residual=True)
            for p in range(2):
                y_p = y[0][rows][:, p * C:(p + 1) * C].contiguous()
                sm[p][0].update(y_p, outs[0][rows][:, p * C:(p + 1) * C].contiguous())
                sm[p][1].update(y_p, Persistence(X[0][rows].contiguous(), C))
    for p in range(2):
        for q in range(2):
            a, b = res.horizons[p][q], sm[p][q]
            assert a.n == b.n == 3
            for f in ("rmse", "mae", "acc"):
                assert abs(getattr(a, f) - getattr(b, f)) <= 1e-10 * max(1.0, abs(getattr(b, f))), (p, q, f)
            assert np.allclose(a.rmse_per_channel, b.rmse_per_channel, rtol=1e-10, atol=0)
            assert np.allclose(a.acc_per_channel, b.acc_per_channel, rtol=0, atol=1e-10)
