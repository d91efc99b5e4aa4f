"""`graphcast_lite_amd.predict` (the loop and the entry point), `observations.create_obs` and
`verify.interpolate_to_region` on the GPU against the reference's own `main()` runs recorded in
tests/golden/predict_vectors.npz (tests/golden/make_predict_golden.py).

Tolerances.  The forecasts are float32 rollouts of a tanh stub model, the reference's on the CPU: 1e-4 relative on every
float attribute of a `StreamingMetrics` object (1e-4 absolute on the ACC sums) and on the saved tensors, and the rule of
`_same_lines` with 1e-4 on the printed block - both numbers and that helper's rule are those of
test_regional_train_golden.py for the same kind of comparison.  The regional scoring of a bundle is float64 arithmetic
on identical inputs: 1e-10 on the scores, `_same_lines` with 1e-9 on the lines, and the two stored fields bit for bit
(single float64 -> float32 roundings of IEEE-exact arithmetic)."""
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, experiment

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import predict_case as pc  # noqa: E402
import runner_case as RC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOATS = ("sum_se", "sum_ae", "sum_se_per_ch")
COUNTS = ("n", "total_elem", "elem_per_ch", "acc_count")


def _said():
    buf = io.StringIO()
    return buf, (lambda s="": buf.write(str(s) + "\n"))


def _fields(sm):
    return {f: np.asarray(getattr(sm, f), np.float64) for f in FLOATS + COUNTS + ("sum_acc",)}


@pytest.mark.parametrize("name", pc.set_names())
def test_recorded_option_set(name, tmp_path, lib_built):
    from graphcast_lite_amd.predict import inference_tables

    z = pc.fixture()
    _, quiet = _said()
    run, args, (variables, std) = pc.run_set(z, name, tmp_path, DEV, batch_size=8, say=quiet)
    ver = run.verifier
    want = pc.recorded_objects(z, name)
    order = pc.creation_order(run.ar_steps, run.region is not None)
    assert len(order) == len(want) == len(ver._objects), "object count"
    worst = 0.0
    for rec, (kind, method, p) in zip(want, order):
        got = _fields(pc.verifier_object(ver, kind, method, p))
        for f in COUNTS:
            assert np.array_equal(got[f], rec[f]), (name, kind, method, p, f)
        for f in FLOATS:
            e = np.abs(got[f] - rec[f]) / np.maximum(np.abs(rec[f]), 1e-30)
            e = np.where(rec[f] == 0, np.abs(got[f]), e)
            worst = max(worst, float(np.max(e)))
            assert np.all(e <= 1e-4), (name, kind, method, p, f, got[f], rec[f])
        assert np.all(np.abs(got["sum_acc"] - rec["sum_acc"]) <= 1e-4 * np.maximum(1.0, rec["acc_count"])), (name, kind, p)
    print(f"{name}: worst relative error of a sum {worst:.2e}")
    buf, say = _said()
    inference_tables(run, per_channel=args.per_channel, variables=variables, std=std, say=say)
    pc.same_lines(pc.summary_block(buf.getvalue()), pc.summary_block(str(z[f"{name}:stdout"])), 1e-4, name)
    if name == "offline":
        from graphcast_lite_amd.predict import PREDICTION_KEYS, load_predictions, save_predictions

        n_lon, n_lat, C, obs, ns = (int(v) for v in z["dims"])
        path = str(tmp_path / "saved.pt")
        save_predictions(path, run.predictions, run.ground_truth, C, run.ar_steps, obs, n_lon, n_lat,
                         sample_offsets=run.sample_offsets, data_dir="<tmp>/data_plain")
        b = load_predictions(path)
        assert list(b) == [str(k) for k in z["offline:bundle_keys"]] == list(PREDICTION_KEYS)
        assert [b[k] for k in ("n_features", "ar_steps", "obs_window", "n_lon", "n_lat")] == z["offline:bundle:ints"].tolist()
        assert b["sample_offsets"] == z["offline:bundle:sample_offsets"].tolist()
        assert b["data_dir"] == str(z["offline:bundle:data_dir"])
        assert torch.equal(b["ground_truth"], torch.from_numpy(z["offline:bundle:ground_truth"]))
        want_p = torch.from_numpy(z["offline:bundle:predictions"])
        assert b["predictions"].shape == want_p.shape
        assert float((b["predictions"] - want_p).abs().max()) <= 1e-4 * float(want_p.abs().max())


@pytest.mark.parametrize("name", ["plain", "seqnudge", "oi"])
def test_batch_size_does_not_change_a_bit(name, tmp_path, lib_built):
    """Batches of 1 and of 3 (3 + 1) over the 4 samples: equal verifier states and kept forecasts, and the states of
    `verify.StreamingMetrics` fed sample by sample (at 1e-10: another order of the same float64 sums)."""
    from graphcast_lite_amd.verify import Persistence, StreamingMetrics

    z = pc.fixture()
    _, quiet = _said()
    dirs = pc.write_dirs(tmp_path, z)
    argv_key = f"{name}:argv"
    runs = {}
    for bs in (1, 3):
        # keep the forecasts as well: the same options plus --save
        zz = {k: z[k] for k in z.files}
        zz[argv_key] = np.asarray([str(a) for a in z[argv_key]] + ["--save", "x.pt"])
        runs[bs], _, _ = pc.run_set(zz, name, tmp_path, DEV, batch_size=bs, per_sample=True, say=quiet, dirs=dirs)
    a, b = runs[1], runs[3]
    assert torch.equal(a.verifier._states, b.verifier._states)
    assert torch.equal(a.predictions, b.predictions) and torch.equal(a.ground_truth, b.ground_truth)
    assert a.sample_offsets == b.sample_offsets == [0, 1, 2, 3]
    # sample by sample through single objects
    n_lon, n_lat, C, obs, ns = (int(v) for v in z["dims"])
    X, y = torch.from_numpy(z["s3_X"]).to(DEV), torch.from_numpy(z["s3_y"]).to(DEV)
    pred = a.predictions.to(DEV)
    sm = {"pred": StreamingMetrics(C, [1, 3]), "base": StreamingMetrics(C, [1, 3])}
    rows = None if a.rows is None else torch.from_numpy(a.rows).to(DEV)
    sm_r = {"pred": StreamingMetrics(C, [1, 3]), "base": StreamingMetrics(C, [1, 3])}
    for i in range(ns):
        sm["pred"].update(y[i], pred[i])
        sm["base"].update(y[i], Persistence(X[i], C))
        if rows is not None:
            sm_r["pred"].update(y[i][rows], pred[i][rows])
            sm_r["base"].update(y[i][rows], X[i][rows][:, -C:].repeat(1, 3))
    for m in ("pred", "base"):
        pairs = [(a.verifier.overall[m], sm[m])] + ([(a.verifier.region[m], sm_r[m])] if rows is not None else [])
        for got, want in pairs:
            g, w = got._host(), want._host()
            assert np.all(np.abs(g - w) <= 1e-10 * np.maximum(1.0, np.abs(w))), (name, m, g, w)


def _experiment_dir(path, data_dir):
    cfg = experiment("demo_low", [1]).model_dump(mode="json")
    cfg.update(wandb_log=False, data_dir=data_dir)
    cfg["data"]["dataset_name"] = "demo_era5_small"
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(cfg, fh)
    return path


@pytest.mark.parametrize("use_graph", [True, False])
def test_main_end_to_end_on_a_real_model(use_graph, tmp_path, lib_built, capsys):
    """`main([...])` on a `WeatherPrediction` (the smallest configuration of the suite) over a chunked directory: it
    returns, writes the bundle, and its scores are those of `rollout` + `ForecastVerifier` called by hand on the same
    batches, bit for bit."""
    from graphcast_lite_amd import main as M
    from graphcast_lite_amd import predict as P
    from graphcast_lite_amd.config import ExperimentConfig
    from graphcast_lite_amd.data import load_chunked_datasets
    from graphcast_lite_amd.verify import ForecastVerifier, Persistence

    LON, LAT, FEAT, T = 16, 8, 3, 41
    rng = np.random.default_rng(0)
    zc = dict(reg_series=rng.standard_normal((T, LON, LAT, FEAT)).astype(np.float16), reg_mean=np.zeros(FEAT, np.float32),
              reg_std=np.ones(FEAT, np.float32), reg_lon=np.linspace(0, 360, LON, endpoint=False),
              reg_lat=np.linspace(-90, 90, LAT))
    data_dir = RC.write_chunked(str(tmp_path / "series"), zc)
    exp = _experiment_dir(str(tmp_path / "exp"), data_dir)
    with open(os.path.join(exp, "config.json")) as fh:
        cfg = ExperimentConfig(**json.load(fh))
    dev = torch.device(DEV)
    _, _, test_ds, meta = load_chunked_datasets(data_path=data_dir, obs_window=2, pred_steps=2, n_features=FEAT,
                                                test_split="test", device=dev)
    torch.manual_seed(3)
    model = M.load_model_from_experiment_config(cfg, dev, meta).to(dev).eval()
    torch.save(model.state_dict(), os.path.join(exp, "best_model.pth"))
    saved = str(tmp_path / "predictions.pt")
    run = P.main([exp, "--ar-steps", "2", "--split", "test", "--batch-size", "2", "--region", "-40", "40", "80", "200",
                  "--save", saved, "--per-channel"], device=DEV, use_graph=use_graph)
    said = capsys.readouterr().out
    assert "=== Inference summary (8 samples) ===" in said and "--- Region [-40.0,40.0]N x [80.0,200.0]E (" in said
    assert len(test_ds) == 8 and run.n_samples == 8
    rows, _ = P.scored_rows([-40.0, 40.0, 80.0, 200.0], 0, meta, data_dir, LON * LAT, say=lambda s: None)
    ver = ForecastVerifier(FEAT, 2, region_idxs=rows, device=dev)
    outs = []
    for i0 in range(0, 8, 2):
        X, y = test_ds.batch([i0, i0 + 1])
        out = P.rollout(model, X, 2)
        ver.update(y, pred=out, base=Persistence(X, FEAT))
        outs.append(out)
    assert torch.equal(run.verifier._states, ver._states)
    b = P.load_predictions(saved)
    assert torch.equal(b["predictions"], torch.cat(outs).cpu())
    assert b["sample_offsets"] == [t for _, t in test_ds._sample_indices] and b["n_lon"] == LON and b["ar_steps"] == 2
    assert run.overall[0].rmse == ver.overall["pred"].rmse and run.region[1].acc == ver.region["base"].acc


# ----------------------------------------------------------------------------------------------------------------------
# observations.create_obs
# ----------------------------------------------------------------------------------------------------------------------
def test_create_obs_writes_the_recorded_tensor(tmp_path, lib_built):
    from graphcast_lite_amd.observations import main

    z = pc.fixture()
    n_lon, n_lat, C, obs, ns = (int(v) for v in z["dims"])
    y = torch.from_numpy(z["obs:y"])
    layouts = {"flat": y, "spatial": y.view(6, n_lon, n_lat, 2 * C), "full": y.view(6, n_lon, n_lat, 2, C)}
    (tmp_path / "variables.json").write_text(json.dumps([str(v) for v in z["variables"]]))
    np.savez(tmp_path / "coords_axes.npz", latitude=z["obs:coords_axes_lats"], longitude=z["obs:coords_axes_lons"])
    np.savez(tmp_path / "coords_nodes.npz", latitude=z["obs:coords_nodes_lats"], longitude=z["obs:coords_nodes_lons"])
    for run in (str(r) for r in z["obs:runs"]):  # with --roi (axes and per-node coordinates) and without
        layout = str(z[f"obs:{run}:layout"])
        torch.save(layouts[layout].clone(), tmp_path / f"y_{layout}.pt")
        save = tmp_path / run / "obs.pt"
        argv = [str(a).replace("<d>", str(tmp_path)) for a in z[f"obs:{run}:argv"]]
        got = main(["create", "--y-path", str(tmp_path / f"y_{layout}.pt"), "--vars-path", str(tmp_path / "variables.json"),
                    "--save-path", str(save)] + argv, device=DEV)
        on_disk = torch.load(save, weights_only=True)
        assert on_disk.shape == (3, n_lon * n_lat, 2 * C) and not on_disk.is_cuda
        assert np.array_equal(on_disk.numpy().view(np.int32), z[f"obs:{run}:bits"]), run
        assert np.array_equal(got.numpy().view(np.int32), z[f"obs:{run}:bits"]), run
    assert main(["create", "--y-path", str(tmp_path / "y_flat.pt"), "--vars-path", str(tmp_path / "variables.json"),
                 "--save-path", str(tmp_path / "none.pt"), "--roi", "1", "2", "3", "4"], device=DEV) is None


# ----------------------------------------------------------------------------------------------------------------------
# verify.interpolate_to_region
# ----------------------------------------------------------------------------------------------------------------------
def test_interpolate_to_region_reproduces_the_recorded_run(tmp_path, lib_built):
    from graphcast_lite_amd.verify import main

    z = pc.fixture()
    f = pc.interp_inputs(z)
    bundle, gd, rd = pc.write_interp_dirs(tmp_path, z)
    out = str(tmp_path / "interp_out.pt")
    buf = io.StringIO()
    import contextlib

    with contextlib.redirect_stdout(buf):
        res = main(["--predictions", bundle, "--global-data", gd, "--region-data", rd, "--per-channel", "--out", out],
                   device=DEV)
    got, want = buf.getvalue().replace(str(tmp_path), "<tmp>"), str(z["interp:stdout"])
    pc.same_lines(got.rstrip("\n"), want.rstrip("\n"), 1e-9, "interpolate_to_region")
    # the scores against the restatement of the recorded run's inputs at 1e-10
    from graphcast_lite_amd.verify import RegionBundleScores, match_regional_steps, regrid_tables

    t0 = match_regional_steps(f["offsets"], f["obs"], 4, f["P"], f["nt"])
    cell, w = regrid_tables(f["g_lats"], f["g_lons"], f["r_lats"], f["r_lons"])
    v, t, b = pc.region_fields(f["pred"], f["ntg"], cell, w, f["series"], t0, f["mean"][:f["C"]], f["std"][:f["C"]],
                               f["P"], f["C"])
    ref = RegionBundleScores(pc.region_sums(v, t, b, t0, f["nt"]), 3, 5, f["nlr"] * f["ntr"])
    assert (res.n_matched, res.n_samples, res.n_nodes) == (3, 5, 35)
    pairs = [(res.overall, ref.overall)] + [(res.horizon(p), ref.horizon(p)) for p in range(f["P"])]
    pairs += [(res.channel(p, c), ref.channel(p, c)) for p in range(f["P"]) for c in range(f["C"])]
    for x, y in pairs:
        for key in ("rmse", "base", "mae", "skill", "acc"):
            assert abs(x[key] - y[key]) <= 1e-10 * max(1.0, abs(y[key])), (key, x, y)
    saved = torch.load(out, weights_only=False)
    assert list(saved) == [str(k) for k in z["interp:out_keys"]]
    assert torch.equal(saved["interpolated_predictions"], torch.from_numpy(z["interp:out:interpolated_predictions"]))
    assert torch.equal(saved["regional_ground_truth"], torch.from_numpy(z["interp:out:regional_ground_truth"]))
    assert saved["interpolated_predictions"].dtype == torch.float32
    assert saved["variables"] == [str(v) for v in z["interp:out:variables"]] and saved["n_matched"] == 3
    for key in ("region_lats", "region_lons", "scalers_mean", "scalers_std"):
        assert np.array_equal(saved[key], z[f"interp:out:{key}"]) and saved[key].dtype == np.float64, key
    # the legacy form of the bundle: the bare tensor (grid and channel count from the global data set, offsets 0..N-1)
    bare = str(tmp_path / "bare.pt")
    torch.save(torch.from_numpy(f["pred"]), bare)
    with contextlib.redirect_stdout(io.StringIO()):
        res2 = main(["--predictions", bare, "--global-data", gd, "--region-data", rd], device=DEV)
    assert res2.n_samples == 5 and res2.n_matched == 5  # steps 6 .. 10 of the 12
