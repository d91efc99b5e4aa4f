"""Generate tests/golden/regional_train_vectors.npz by RUNNING the reference's own epoch functions
(`scripts/train_dual_mesh.py`: `train_dual_epoch`, `eval_dual`; `scripts/train_roi_residual.py`: `train_epoch`,
`eval_epoch`) around the reference's `DualMeshModel` and `ROIResidualModel`.

Run from the repo root, only where the reference tree (`make_golden.REF`) exists:

    python tests/golden/make_regional_train_golden.py

Placeholders and stand-ins are those of `make_dual_mesh_golden.py` (imported from there, not copied); the global model
is `tests/helpers/regional_case.py`'s `LinearStubGlobal`.  Every case runs two epochs over three training samples with
torch's Adam (lr 5e-4), evaluating two validation samples after each epoch:
  cached      `--precompute` mode (cache of `precompute_global`), residual on
  std_ar1     standard mode, ar_steps 1, residual off
  std_ar2     standard mode, ar_steps 2, residual on
Evaluation of the final weights with one static and one forcing channel (`eval_special`, ar_steps 2) is recorded as well.
The ROI head (`roi:` keys) runs the same two epochs with lr 1e-3 (hidden 32, 2 processor steps, roi_k 4); its printed
`[Correction]` lines are kept as strings.
Outputs (data only): the grid, the samples, the initial regional parameters, and per case the per-epoch training losses,
(validation loss, correction skill) pairs and the final regional parameters.
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_dual_mesh_golden as base  # noqa: E402
import make_golden  # noqa: E402
from make_roi_golden import _LayerNorm  # noqa: E402
from regional_case import LinearStubGlobal  # noqa: E402

C, OBS, D, HIDDEN, STEPS, K, LR = 5, 2, 11, 32, 2, 3, 5e-4
ROI_STEPS, ROI_K, ROI_LR = 2, 4, 1e-3
CASES = {"cached": dict(cached=True, residual=True, ar=1), "std_ar1": dict(cached=False, residual=False, ar=1),
         "std_ar2": dict(cached=False, residual=True, ar=2)}


def _main_runs(dm, script, roi_script, glats, glons, lats, lons, g):
    """tests/golden/regional_main_vectors.npz: the three scripts' `main()` run as they are, on a temporary experiment
    directory, with only their inputs replaced (the configuration object, the data sets, the global model, and a
    `DataLoader` without workers or shuffling), and everything they print, log and write kept as data:
      dual     train_dual_mesh.py, two epochs, ar_steps 2, residual, static channel 1 and forcing channel 3
      roi      train_roi_residual.py, two epochs
      predict  predict_dual_mesh.py --per-channel --ar-steps 2 with the weights the dual run saved
    plus the values the epoch functions returned, the regional parameters before and after the dual run, and the state
    of every `StreamingMetrics` object of the predict run."""
    import contextlib
    import io
    import json
    import tempfile
    import types

    import predict_dual_mesh as pred_script
    from torch.utils.data import DataLoader as TorchLoader

    G = lats.shape[0]
    mk = lambda n: [(torch.randn(G, C * OBS, generator=g), torch.randn(G, 2 * C, generator=g)) for _ in range(n)]  # noqa: E731
    train, val, test = mk(3), mk(2), mk(3)
    variables = ["t2m", "10u", "msl", "z@500", "q@850"]
    std = np.asarray([12.5, 3.25, 850.0, 2900.0, 0.002], np.float64)
    tmp = tempfile.mkdtemp()
    exp, data_dir = os.path.join(tmp, "exp"), os.path.join(tmp, "data")
    os.makedirs(exp), os.makedirs(data_dir)
    open(os.path.join(exp, "config.json"), "w").write("{}")
    json.dump(variables, open(os.path.join(data_dir, "variables.json"), "w"))
    np.savez(os.path.join(data_dir, "scalers.npz"), std=std, mean=np.zeros(C))
    torch.save({}, os.path.join(tmp, "global.pth"))
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(obs_window_used=OBS, num_features_used=C,
                                                           dataset_name=types.SimpleNamespace(value="fixture")),
                                batch_size=1, num_epochs=2, max_ar_steps=2, use_residual=True, static_channels=[1],
                                forcing_channels=[3], use_latitude_weighting=False)
    meta = types.SimpleNamespace(cordinates=(lats, lons), flat_grid=True)
    out = {"variables": np.asarray(variables), "std": std, "grid_lats": lats, "grid_lons": lons, "global_lats": glats,
           "global_lons": glons, "dims": np.asarray([C, OBS, D, HIDDEN, STEPS, K, base.LEVEL], np.int64),
           "roi": np.asarray(base.ROI, np.float64), "buffer": np.float64(2.0)}
    for name, ds in (("train", train), ("val", val), ("test", test)):
        out[f"{name}_X"] = torch.stack([x for x, _ in ds]).numpy()
        out[f"{name}_y"] = torch.stack([y for _, y in ds]).numpy()
    roi_args = [str(v) for v in base.ROI]
    calls = {}

    def patch(mod):
        mod.ExperimentConfig = lambda **kw: cfg
        mod.load_from_json_file = lambda path: {}
        mod.load_chunked_datasets = lambda **kw: (train, val, test, meta)
        mod.load_model_from_experiment_config = lambda *a, **k: LinearStubGlobal(C, OBS, D, glats, glons)
        if hasattr(mod, "DataLoader"):
            mod.DataLoader = lambda ds, batch_size=1, shuffle=False, **kw: TorchLoader(ds, batch_size=batch_size)

    def recording(mod, fn, key):
        inner = getattr(mod, fn)

        def wrapped(*a, **k):
            r = inner(*a, **k)
            calls.setdefault(key, []).append(r)
            return r

        setattr(mod, fn, wrapped)

    def run(mod, argv):
        said, old = io.StringIO(), sys.argv
        sys.argv = ["x"] + argv
        try:
            with contextlib.redirect_stdout(said):
                mod.main()
        finally:
            sys.argv = old
        return said.getvalue()

    own = lambda m: {n: p.detach().clone() for n, p in m.named_parameters() if not n.startswith("global_model.")}  # noqa: E731
    # --- dual
    patch(script)
    recording(script, "train_dual_epoch", "dual:train")
    recording(script, "eval_dual", "dual:eval")
    inner_overfit = script.overfit_test

    def overfit(model, *a, **k):
        for n, v in own(model).items():
            out["dual:w0:" + n] = v.numpy()
        return inner_overfit(model, *a, **k)

    script.overfit_test = overfit
    out["dual:stdout"] = np.asarray(run(script, [exp, "--pretrained", os.path.join(tmp, "global.pth"), "--data-dir", data_dir,
                                                 "--roi", *roi_args, "--reg-mesh-level", str(base.LEVEL), "--reg-steps",
                                                 str(STEPS), "--cross-k", str(K), "--hidden-dim", str(HIDDEN)]
                                        ).replace(tmp, "<tmp>"))  # (the scripts' default mesh buffer, 2 degrees)
    res_dir = os.path.join(exp, "results")
    out["dual:log"] = np.asarray(open(os.path.join(res_dir, "training_log.txt")).read().replace(tmp, "<tmp>"))
    out["dual:results_json"] = np.asarray(open(os.path.join(res_dir, "results.json")).read())
    out["dual:files"] = np.asarray(sorted(os.listdir(res_dir)))
    out["dual:train"] = np.asarray(calls["dual:train"], np.float64)
    out["dual:eval"] = np.asarray(calls["dual:eval"], np.float64)  # two validation passes, then the test pass
    best = torch.load(os.path.join(res_dir, "best_regional.pth"))
    out["dual:regional_keys"] = np.asarray(sorted(best))
    for n in [k for k in out if k.startswith("dual:w0:")]:
        out["dual:w:" + n[len("dual:w0:"):]] = best[n[len("dual:w0:"):]].numpy()
    # --- predict (reads the best_regional.pth of the dual run; its default mesh buffer is the model's 2.0)
    patch(pred_script)
    made = []

    class Recorded(pred_script.StreamingMetrics):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    pred_script.StreamingMetrics = Recorded
    out["predict:stdout"] = np.asarray(run(pred_script, [exp, "--pretrained", os.path.join(tmp, "global.pth"), "--data-dir",
                                                         data_dir, "--roi", *roi_args, "--reg-mesh-level", str(base.LEVEL),
                                                         "--reg-steps", str(STEPS), "--cross-k", str(K), "--hidden-dim",
                                                         str(HIDDEN), "--per-channel", "--ar-steps", "2"]
                                           ).replace(tmp, "<tmp>"))
    out["predict:results_json"] = np.asarray(open(os.path.join(res_dir, "predict_results.json")).read())
    # order of construction: overall pred, overall base, pred per horizon, base per horizon
    out["predict:scores"] = np.asarray([[m.n, m.rmse, m.mae, m.acc] for m in made], np.float64)
    out["predict:rmse_per_channel"] = np.asarray([m.rmse_per_channel for m in made], np.float64)
    out["predict:acc_per_channel"] = np.asarray([m.acc_per_channel for m in made], np.float64)
    # --- roi
    patch(roi_script)
    recording(roi_script, "train_epoch", "roi:train")
    recording(roi_script, "eval_epoch", "roi:eval")
    roi_exp = os.path.join(tmp, "roi_exp")
    os.makedirs(roi_exp)
    open(os.path.join(roi_exp, "config.json"), "w").write("{}")
    out["roi:stdout"] = np.asarray(run(roi_script, [roi_exp, "--pretrained", os.path.join(tmp, "global.pth"), "--data-dir",
                                                    data_dir, "--roi", *roi_args, "--hidden-dim", str(HIDDEN),
                                                    "--processor-steps", str(ROI_STEPS), "--roi-k", str(ROI_K)]
                                       ).replace(tmp, "<tmp>"))
    roi_res = os.path.join(roi_exp, "results")
    out["roi:log"] = np.asarray(open(os.path.join(roi_res, "training_log.txt")).read().replace(tmp, "<tmp>"))
    out["roi:results_json"] = np.asarray(open(os.path.join(roi_res, "results.json")).read().replace(tmp, "<tmp>"))
    out["roi:files"] = np.asarray(sorted(os.listdir(roi_res)))
    out["roi:train"] = np.asarray(calls["roi:train"], np.float64)
    out["roi:eval"] = np.asarray(calls["roi:eval"], np.float64)
    path = os.path.join(HERE, "regional_main_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote regional_main_vectors.npz", os.path.getsize(path), "bytes")
    print(str(out["dual:log"]))
    print(str(out["predict:stdout"])[-2500:])
    print(str(out["roi:log"]))


def main():
    if not os.path.isdir(make_golden.REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    make_golden._placeholders()
    sys.modules["torch_geometric.nn"].LayerNorm = _LayerNorm
    sys.modules["torch_geometric.utils"].scatter = base._scatter
    sys.path.insert(0, make_golden.REF)
    sys.path.insert(0, os.path.join(make_golden.REF, "scripts"))
    import src.dual_mesh as dm
    import train_dual_mesh as script

    glats, glons = base._global_mesh()
    lats, lons = base._grid()
    G = lats.shape[0]
    g = torch.Generator().manual_seed(33)
    train = [(torch.randn(1, G, C * OBS, generator=g), torch.randn(1, G, 2 * C, generator=g)) for _ in range(3)]
    val = [(torch.randn(1, G, C * OBS, generator=g), torch.randn(1, G, 2 * C, generator=g)) for _ in range(2)]
    torch.manual_seed(9)
    m0 = dm.DualMeshModel(LinearStubGlobal(C, OBS, D, glats, glons), base.ROI, lats, lons, torch.device("cpu"),
                          reg_mesh_level=base.LEVEL, reg_mesh_buffer=base.BUFFER, reg_processor_steps=STEPS, cross_k=K,
                          hidden_dim=HIDDEN)
    for p in m0.global_model.parameters():
        p.requires_grad = False
    with torch.no_grad():  # off the decoder's near-zero start, so that the correction matters from the first step
        m0.reg_decoder.mlp[2].weight.normal_(0.0, 0.2, generator=g)
        m0.reg_decoder.mlp[2].bias.normal_(0.0, 0.1, generator=g)
    own = lambda m: {n: p.detach().clone() for n, p in m.named_parameters() if not n.startswith("global_model.")}  # noqa: E731
    out = {"grid_lats": lats, "grid_lons": lons, "global_lats": glats, "global_lons": glons,
           "roi": np.asarray(base.ROI, np.float64), "buffer": np.float64(base.BUFFER),
           "dims": np.asarray([C, OBS, D, HIDDEN, STEPS, K, base.LEVEL], np.int64), "lr": np.float64(LR),
           "cases": np.asarray(sorted(CASES))}
    for i, (X, y) in enumerate(train):
        out[f"train_X{i}"], out[f"train_y{i}"] = X.numpy(), y.numpy()
    for i, (X, y) in enumerate(val):
        out[f"val_X{i}"], out[f"val_y{i}"] = X.numpy(), y.numpy()
    for k, v in own(m0).items():
        out["w0:" + k] = v.numpy()
    for name, case in CASES.items():
        m = copy.deepcopy(m0)
        opt = torch.optim.Adam([p for n, p in m.named_parameters() if not n.startswith("global_model.") and p.requires_grad],
                               lr=LR)
        tc = vc = None
        if case["cached"]:
            m.eval()
            tc = [m.precompute_global(X) for X, _ in train]
            vc = [m.precompute_global(X) for X, _ in val]
        tl, ev = [], []
        for epoch in range(2):
            tl.append(script.train_dual_epoch(m, train, opt, torch.device("cpu"), use_residual=case["residual"],
                                              current_ar_steps=case["ar"], cache=tc))
            ev.append(script.eval_dual(m, val, torch.device("cpu"), use_residual=case["residual"],
                                       current_ar_steps=case["ar"], cache=vc))
        out[f"{name}:train_loss"], out[f"{name}:eval"] = np.asarray(tl, np.float64), np.asarray(ev, np.float64)
        for k, v in own(m).items():
            out[f"{name}:w:" + k] = v.numpy()
        if name == "std_ar2":
            out["eval_special"] = np.asarray(script.eval_dual(m, val, torch.device("cpu"), use_residual=True,
                                                              current_ar_steps=2, static_channels=[1],
                                                              forcing_channels=[3]), np.float64)
    # scripts/train_roi_residual.py: train_epoch / eval_epoch around the reference's ROIResidualModel, lr 1e-3
    import contextlib
    import io

    import src.roi_residual as rr
    import train_roi_residual as roi_script

    torch.manual_seed(11)
    r = rr.ROIResidualModel(LinearStubGlobal(C, OBS, D, glats, glons), base.ROI, lats, lons, torch.device("cpu"),
                            hidden_dim=HIDDEN, processor_steps=ROI_STEPS, roi_k=ROI_K)
    for p in r.global_model.parameters():
        p.requires_grad = False
    with torch.no_grad():
        r.decoder.mlp[-1].weight.normal_(0.0, 0.2, generator=g)
    for k, v in own(r).items():
        out["roi:w0:" + k] = v.numpy()
    opt = torch.optim.Adam([p for n, p in r.named_parameters() if not n.startswith("global_model.") and p.requires_grad],
                           lr=ROI_LR)
    tl, ev, said = [], [], io.StringIO()
    for epoch in range(2):
        with contextlib.redirect_stdout(said):
            tl.append(roi_script.train_epoch(r, train, opt, torch.device("cpu")))
        ev.append(roi_script.eval_epoch(r, val, torch.device("cpu")))
    out["roi:train_loss"], out["roi:eval"] = np.asarray(tl, np.float64), np.asarray(ev, np.float64)
    out["roi:correction_lines"] = np.asarray([ln for ln in said.getvalue().split("\n") if "[Correction]" in ln])
    out["roi:dims"] = np.asarray([ROI_STEPS, ROI_K], np.int64)
    out["roi:lr"] = np.float64(ROI_LR)
    for k, v in own(r).items():
        out["roi:w:" + k] = v.numpy()
    print("roi", out["roi:train_loss"], out["roi:eval"].tolist(), out["roi:correction_lines"])
    _main_runs(dm, script, roi_script, glats, glons, lats, lons, g)
    path = os.path.join(HERE, "regional_train_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote regional_train_vectors.npz", os.path.getsize(path), "bytes")
    for name in CASES:
        print(name, out[f"{name}:train_loss"], out[f"{name}:eval"].tolist())
    print("eval_special", out["eval_special"])


if __name__ == "__main__":
    main()
