"""Generate tests/golden/predict_vectors.npz by RUNNING the reference's own `main()` of `scripts/predict.py`,
`scripts/create_obs.py`, `scripts/generate_assim_dataset.py` and `scripts/interpolate_to_region.py` with only their
inputs replaced.

Run from the repo root, only where the reference tree (`make_golden.REF`) exists:

    python tests/golden/make_predict_golden.py

predict.py: `ExperimentConfig`, `load_from_json_file`, the two dataset loaders and `load_model_from_experiment_config` are
patched (the pattern of `make_regional_train_golden._main_runs` with `make_golden._placeholders()`); the model is the
tanh `StubModel` of `tests/helpers/stub_model.py`; `StreamingMetrics` is wrapped so that every instance is recorded in
creation order; `ArgumentParser.parse_args` is wrapped so that each option's flags, default, type name, nargs and choices
are recorded.  Grid 12 x 8 (longitude-major), C 5, obs 2, 4 samples, static [1], forcing [3].  Option sets (`SETS`):
  plain        AR 3, --per-channel --region 50 60 83 98 over a directory with coords.npz axes
  seqnudge     sequential nudging, --obs-sparsity 0.2 --obs-channels t2m,msl,nope --nudge-first-k 2
  oi           OI, --region on the linspace axes, --oi-corr-len 300000, a 25 % network
  oi_dense     OI against the whole truth on the region rows
  offline      offline nudging with --save
  blend        --boundary-blending --background-path
  onestep      AR = P_model = 1 (static channel 1 is NOT carried), --per-channel
  onestep_nores  the same with --no-residual
  multistep    AR = P_model = 3: the model's output as it is
  flat         a flat-grid dataset with is_regional, roi-only stations, sequential nudging
  bmw          boundary_mask_width = 1
  prune        --prune-mesh --mesh-buffer 7.5 over the coords.npz directory
  short        AR 3 over targets of one step: the truth's width decides what is scored
  legacy       the legacy loader (y is the observation source), OI with --obs-path absent, --max-samples 3
For each set: stdout, every recorded object's attributes, what the patched hooks saw, and the saved bundle.

The other three scripts run on small files written to a temporary directory; what they print and write is kept.
Everything stored is data (inputs, recorded results, printed text).
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402
from stub_model import StubModel  # noqa: E402

N_LON, N_LAT, C, OBS, NS = 12, 8, 5, 2, 4
G = N_LON * N_LAT
VARIABLES = ["t2m", "10u", "msl", "z@500", "q@850"]
STD = np.asarray([12.5, 3.25, 850.0, 2900.0, 0.002], np.float64)
REGION_C = ["50", "60", "83", "98"]        # on the coords.npz axes
REGION_L = ["-40", "40", "80", "200"]      # on the linspace axes
SM_FIELDS = ("n", "total_elem", "sum_se", "sum_ae", "sum_se_per_ch", "elem_per_ch", "sum_acc", "acc_count")

SETS = {
    "plain": dict(argv=["--ar-steps", "3", "--per-channel", "--region", *REGION_C], data="coords"),
    "seqnudge": dict(argv=["--ar-steps", "3", "--assim-method", "nudging", "--obs-sparsity", "0.2", "--obs-channels",
                           "t2m,msl,nope", "--nudge-first-k", "2"], data="plain"),
    "oi": dict(argv=["--ar-steps", "3", "--assim-method", "oi", "--region", *REGION_L, "--oi-corr-len", "300000",
                     "--obs-sparsity", "0.25", "--obs-roi-only", "--obs-seed", "5"], data="plain"),
    "oi_dense": dict(argv=["--ar-steps", "3", "--assim-method", "oi", "--region", *REGION_L, "--oi-corr-len", "300000"],
                     data="plain"),
    "offline": dict(argv=["--ar-steps", "3", "--assim-method", "nudging", "--nudging-mode", "offline", "--nudging-alpha",
                          "0.4", "--save", "<tmp>/saved.pt"], data="plain"),
    "blend": dict(argv=["--ar-steps", "3", "--boundary-blending", "--background-path", "<tmp>/background.pt",
                        "--taper-width", "2"], data="plain"),
    "onestep": dict(argv=["--per-channel"], data="plain", pred_model=1, targets=1),
    "onestep_nores": dict(argv=["--no-residual"], data="plain", pred_model=1, targets=1),
    "multistep": dict(argv=[], data="plain", pred_model=3),
    "flat": dict(argv=["--ar-steps", "3", "--assim-method", "nudging", "--obs-sparsity", "0.3", "--obs-roi-only"],
                 data="flat", flat=True),
    "bmw": dict(argv=["--ar-steps", "3"], data="plain", bmw=1),
    "short": dict(argv=["--ar-steps", "3"], data="plain", targets=1),
    "prune": dict(argv=["--ar-steps", "3", "--prune-mesh", "--mesh-buffer", "7.5"], data="coords"),
    "legacy": dict(argv=["--ar-steps", "3", "--assim-method", "oi", "--region", *REGION_L, "--oi-corr-len", "300000",
                         "--max-samples", "3"], data="legacy", legacy=True),
}


def _samples(g, steps):
    """NS samples (X [G, OBS*C], y [G, steps*C]): y continues X smoothly enough for persistence to mean something."""
    out = []
    for _ in range(NS):
        X = torch.randn(G, OBS * C, generator=g)
        y = X[:, -C:].repeat(1, steps) + 0.3 * torch.randn(G, steps * C, generator=g)
        out.append((X, y))
    return out


class _Squeezing(StubModel):
    """A batch of one comes back without its batch axis, as the reference's model returns it: the only form the
    `AR_STEPS <= P_model` branch of predict.py can score."""

    def forward(self, X, attention_threshold=0.0, **kw):
        out = super().forward(X)
        return out.squeeze(0) if out.dim() == 3 and out.shape[0] == 1 else out


def _run(mod, argv):
    said, old = io.StringIO(), sys.argv
    sys.argv = ["x"] + argv
    try:
        with contextlib.redirect_stdout(said):
            try:
                mod.main()
            except SystemExit:
                pass
    finally:
        sys.argv = old
    return said.getvalue()


def _parser_table(ap):
    rows = []
    for a in ap._actions:
        if isinstance(a, type(ap._actions[0])) and a.dest == "help":
            continue
        rows.append({"flags": list(a.option_strings), "dest": a.dest, "default": a.default,
                     "type": getattr(a.type, "__name__", None) if a.type is not None else None,
                     "nargs": a.nargs, "choices": list(a.choices) if a.choices is not None else None,
                     "action": type(a).__name__, "required": bool(a.required),
                     "metavar": list(a.metavar) if isinstance(a.metavar, tuple) else a.metavar})
    return rows


def _predict_runs(out, tmp):
    import argparse

    import predict as script
    from src.assimilation import optimal_interpolation as oi_mod

    g = torch.Generator().manual_seed(2024)
    W0 = 0.4 * torch.randn(C, OBS * C, generator=g)
    b0 = 0.1 * torch.randn(C, generator=g)
    W3 = 0.4 * torch.randn(3 * C, OBS * C, generator=g)
    b3 = 0.1 * torch.randn(3 * C, generator=g)
    samples3, samples1 = _samples(g, 3), _samples(g, 1)
    background = torch.randn(NS, G, 3 * C, generator=g)
    out.update({"W0": W0.numpy(), "b0": b0.numpy(), "W3": W3.numpy(), "b3": b3.numpy(), "background": background.numpy(),
                "variables": np.asarray(VARIABLES), "std": STD,
                "dims": np.asarray([N_LON, N_LAT, C, OBS, NS], np.int64)})
    for tag, ds in (("s3", samples3), ("s1", samples1)):
        out[f"{tag}_X"] = torch.stack([x for x, _ in ds]).numpy()
        out[f"{tag}_y"] = torch.stack([y for _, y in ds]).numpy()
    torch.save(background, os.path.join(tmp, "background.pt"))

    # --- data directories
    lats_c, lons_c = np.linspace(40, 68, N_LAT), np.linspace(75, 108, N_LON)
    rng = np.random.RandomState(3)
    flat_lats, flat_lons = rng.uniform(30, 70, G), rng.uniform(60, 120, G)
    is_regional = (flat_lats > 45) & (flat_lats < 62) & (flat_lons > 80) & (flat_lons < 105)
    out.update({"coords_lats": lats_c, "coords_lons": lons_c, "flat_lats": flat_lats, "flat_lons": flat_lons,
                "is_regional": is_regional})
    dirs = {}
    for name in ("plain", "coords", "flat", "legacy"):
        d = os.path.join(tmp, "data_" + name)
        os.makedirs(d)
        json.dump(VARIABLES, open(os.path.join(d, "variables.json"), "w"))
        np.savez(os.path.join(d, "scalers.npz"), std=STD, mean=np.zeros(C))
        if name != "legacy":
            open(os.path.join(d, "dataset_info.json"), "w").write("{}")  # what marks a directory as chunked
        dirs[name] = d
    np.savez(os.path.join(dirs["coords"], "coords.npz"), latitude=lats_c, longitude=lons_c)
    np.savez(os.path.join(dirs["flat"], "coords.npz"), latitude=flat_lats, longitude=flat_lons)
    exp = os.path.join(tmp, "exp")
    os.makedirs(exp)
    open(os.path.join(exp, "config.json"), "w").write("{}")
    torch.save({}, os.path.join(exp, "best_model.pth"))

    made, hooks = [], {}

    class Recorded(script.StreamingMetrics):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

    script.StreamingMetrics = Recorded
    inner_region = script.region_node_indices

    def region_node_indices(*a):
        r = inner_region(*a)
        hooks["region_node_indices"] = r
        return r

    script.region_node_indices = region_node_indices
    inner_oi = oi_mod.OptimalInterpolation.__init__

    def oi_init(self, lats, lons, sb, so, L, device, flat_grid=False, roi_idx=None):
        hooks["oi_roi_idx"] = np.asarray([] if roi_idx is None else roi_idx, np.int64)
        hooks["oi_args"] = np.asarray([sb, so, L], np.float64)
        inner_oi(self, lats, lons, sb, so, L, device, flat_grid=flat_grid, roi_idx=roi_idx)

    oi_mod.OptimalInterpolation.__init__ = oi_init
    inner_apply = oi_mod.OptimalInterpolation.apply

    def oi_apply(self, forecast, observations):
        hooks.setdefault("obs_rows", np.nonzero(torch.isfinite(observations).any(-1).numpy())[0])
        hooks.setdefault("obs_chans", np.nonzero(torch.isfinite(observations).any(0).numpy())[0])
        return inner_apply(self, forecast, observations)

    oi_mod.OptimalInterpolation.apply = oi_apply
    inner_seq = script.sequential_nudged_rollout

    def seq(model, x0, y_obs, p, alpha, k, device):
        hooks.setdefault("obs_rows", np.nonzero(torch.isfinite(y_obs[0]).any(-1).numpy())[0])
        hooks.setdefault("obs_chans", np.nonzero(torch.isfinite(y_obs[0]).any(0).numpy())[0] % C)
        hooks["nudge_args"] = np.asarray([p, alpha, -1 if k is None else k], np.float64)
        return inner_seq(model=model, x0=x0, y_obs=y_obs, p=p, alpha=alpha, k=k, device=device)

    script.sequential_nudged_rollout = seq
    inner_parse = argparse.ArgumentParser.parse_args

    def parse_args(self, *a, **k):
        hooks["parser"] = _parser_table(self)
        return inner_parse(self, *a, **k)

    argparse.ArgumentParser.parse_args = parse_args
    try:
        for name, s in SETS.items():
            made.clear()
            hooks.clear()
            p_model = s.get("pred_model", 1)
            targets = s.get("targets", 3)
            data = samples1 if targets == 1 else samples3
            cfg = types.SimpleNamespace(
                data=types.SimpleNamespace(obs_window_used=OBS, num_features_used=C, pred_window_used=p_model,
                                           dataset_name=types.SimpleNamespace(value="fixture")),
                static_channels=[1], forcing_channels=[3])
            if "bmw" in s:
                cfg.boundary_mask_width = s["bmw"]
            meta = types.SimpleNamespace(num_latitudes=N_LAT, num_longitudes=N_LON)
            if s.get("flat"):
                meta = types.SimpleNamespace(num_latitudes=0, num_longitudes=0, flat_grid=True, num_grid_nodes=G,
                                             is_regional=is_regional,
                                             cordinates=(flat_lats.astype(np.float32), flat_lons.astype(np.float32)))

            class Legacy(list):
                y = torch.stack([y for _, y in data])

            def chunked(**kw):
                hooks["loader"] = json.dumps({k: (v if not isinstance(v, str) else v.replace(tmp, "<tmp>"))
                                              for k, v in kw.items()}, sort_keys=True)
                return None, None, list(data), meta

            def legacy(path, data_cfg):
                hooks["loader"] = json.dumps({"legacy": path.replace(tmp, "<tmp>")})
                return None, None, Legacy(data), meta

            def model_of(exp_cfg, device, md, **kw):
                rb = kw.get("region_bounds")
                hooks["model_kwargs"] = json.dumps({"coordinates": kw.get("coordinates") is not None,
                                                    "region_bounds": None if rb is None else [float(v) for v in rb],
                                                    "mesh_buffer": float(kw.get("mesh_buffer")),
                                                    "flat_grid": bool(kw.get("flat_grid"))}, sort_keys=True)
                return _Squeezing(OBS, W3, b3) if p_model == 3 else StubModel(OBS, W0, b0)

            script.ExperimentConfig = lambda **kw: cfg
            script.load_from_json_file = lambda path: {}
            script.load_chunked_datasets = chunked
            script.load_train_and_test_datasets = legacy
            script.load_model_from_experiment_config = model_of
            argv = [exp, "--data-dir", dirs[s["data"]]] + [a.replace("<tmp>", tmp) for a in s["argv"]]
            text = _run(script, argv).replace(tmp, "<tmp>")
            out[f"{name}:argv"] = np.asarray(s["argv"] or [""])
            out[f"{name}:stdout"] = np.asarray(text)
            out[f"{name}:n_objects"] = np.int64(len(made))
            for f in SM_FIELDS:
                out[f"{name}:sm:{f}"] = np.asarray([np.asarray(getattr(m, f), np.float64) for m in made], np.float64)
            out[f"{name}:sm:exclude"] = np.asarray(sorted(made[0].exclude_channels), np.int64)
            for k, v in hooks.items():
                if k != "parser":
                    out[f"{name}:hook:{k}"] = np.asarray(v)
            if name == "plain":
                out["parser"] = np.asarray(json.dumps(hooks["parser"]))
            if name == "offline":
                b = torch.load(os.path.join(tmp, "saved.pt"), weights_only=False)
                out["offline:bundle_keys"] = np.asarray(list(b))
                out["offline:bundle:predictions"] = b["predictions"].numpy()
                out["offline:bundle:ground_truth"] = b["ground_truth"].numpy()
                out["offline:bundle:ints"] = np.asarray([b[k] for k in ("n_features", "ar_steps", "obs_window", "n_lon",
                                                                        "n_lat")], np.int64)
                out["offline:bundle:sample_offsets"] = np.asarray(b["sample_offsets"], np.int64)
                out["offline:bundle:data_dir"] = np.asarray(str(b["data_dir"]).replace(tmp, "<tmp>"))
            print(f"--- {name}: {len(made)} objects")
            print(text[text.find("=" * 60):] if "=" * 60 in text else text)
    finally:
        argparse.ArgumentParser.parse_args = inner_parse
        oi_mod.OptimalInterpolation.__init__ = inner_oi
        oi_mod.OptimalInterpolation.apply = inner_apply


def _create_obs_runs(out, tmp):
    import create_obs as script

    g = torch.Generator().manual_seed(77)
    y = torch.randn(6, G, 2 * C, generator=g)
    d = os.path.join(tmp, "obs")
    os.makedirs(d)
    json.dump(VARIABLES, open(os.path.join(d, "variables.json"), "w"))
    lats_c, lons_c = np.linspace(40, 68, N_LAT), np.linspace(75, 108, N_LON)
    # create_obs.py meshes (lons, lats) latitude-major for axis coordinates: its grid is G = n_lat x n_lon nodes
    np.savez(os.path.join(d, "coords_axes.npz"), latitude=lats_c, longitude=lons_c)
    rng = np.random.RandomState(3)
    flat_lats, flat_lons = rng.uniform(30, 70, G), rng.uniform(60, 120, G)
    np.savez(os.path.join(d, "coords_nodes.npz"), latitude=flat_lats, longitude=flat_lons)
    out["obs:y"] = y.numpy()
    # (the script's fourth layout, [N, G, P, C'] with C' no multiple of the variable count, cannot reach its final reshape)
    layouts = {"flat": y, "spatial": y.view(6, N_LON, N_LAT, 2 * C), "full": y.view(6, N_LON, N_LAT, 2, C)}
    runs = {"flat_all": ("flat", ["--sparsity", "0.1"]),
            "spatial_vars": ("spatial", ["--sparsity", "0.2", "--vars", "t2m, msl,nope", "--seed", "7"]),
            "full_roi_axes": ("full", ["--sparsity", "0.5", "--roi", "50", "60", "83", "98", "--coords-path",
                                       os.path.join(d, "coords_axes.npz"), "--vars", "10u"]),
            "flat_roi_nodes": ("flat", ["--sparsity", "0.3", "--roi", "45", "62", "80", "105", "--coords-path",
                                          os.path.join(d, "coords_nodes.npz"), "--seed", "1"]),
            "tiny": ("flat", ["--sparsity", "0.001", "--vars", "z@500"])}
    out["obs:runs"] = np.asarray(list(runs))
    for name, (layout, extra) in runs.items():
        torch.save(layouts[layout].clone(), os.path.join(d, f"y_{layout}.pt"))
        save = os.path.join(d, name, "obs.pt")
        text = _run(script, ["--y-path", os.path.join(d, f"y_{layout}.pt"), "--vars-path", os.path.join(d, "variables.json"),
                             "--save-path", save] + extra)
        res = torch.load(save)
        out[f"obs:{name}:layout"] = np.asarray(layout)
        out[f"obs:{name}:argv"] = np.asarray([a.replace(d, "<d>") for a in extra])
        out[f"obs:{name}:bits"] = res.numpy().view(np.int32)
        print(f"--- create_obs {name}: {tuple(res.shape)}, {int(torch.isfinite(res).sum())} finite")
        print(text.replace(tmp, "<tmp>").strip().split("\n")[-3])
    out["obs:coords_axes_lats"], out["obs:coords_axes_lons"] = lats_c, lons_c
    out["obs:coords_nodes_lats"], out["obs:coords_nodes_lons"] = flat_lats, flat_lons


def _assim_dataset_runs(out, tmp):
    import generate_assim_dataset as script

    g = torch.Generator().manual_seed(78)
    y5 = torch.randn(3, 4, 3, 2, C, generator=g)
    y3 = torch.randn(3, 12, 2 * C, generator=g)
    out["assim:y5"], out["assim:y3"] = y5.numpy(), y3.numpy()
    runs = {"names": (y5, ["--vars", "t2m,msl,nope"], VARIABLES, None),
            "indices": (y3, ["--indices", "0,3,9", "--out-name", "da"], None, {"data": {"pred_window_used": 2}}),
            "all": (y3, [], None, {"data": {"pred_window": 2}}),
            "names_no_list": (y5, ["--vars", "t2m"], None, None)}
    out["assim:runs"] = np.asarray(list(runs))
    for name, (y, extra, features, cfg) in runs.items():
        exp = os.path.join(tmp, "assim_" + name)
        os.makedirs(exp)
        torch.save(y.clone(), os.path.join(exp, "y_test.pt"))
        if features is not None:
            json.dump(features, open(os.path.join(exp, "features.json"), "w"))
        if cfg is not None:
            json.dump(cfg, open(os.path.join(exp, "config.json"), "w"))
        text = _run(script, [exp] + extra)
        sub = os.path.join(exp, extra[extra.index("--out-name") + 1] if "--out-name" in extra else "assimilation")
        out[f"assim:{name}:argv"] = np.asarray(extra or [""])
        out[f"assim:{name}:y_obs"] = torch.load(os.path.join(sub, "y_obs.pt")).numpy()
        out[f"assim:{name}:mask_flat"] = torch.load(os.path.join(sub, "mask_flat.pt")).numpy()
        out[f"assim:{name}:meta"] = np.asarray(open(os.path.join(sub, "meta.json")).read())
        out[f"assim:{name}:stdout"] = np.asarray(text.replace(exp, "<exp>"))
        print(f"--- generate_assim_dataset {name}: mask {out[f'assim:{name}:mask_flat'].astype(int).tolist()}")


def _interp_runs(out, tmp):
    import interpolate_to_region as script

    NLG, NTG, NLR, NTR, Cr, P, NF, NT = 16, 8, 7, 5, 3, 2, 4, 12
    g = torch.Generator().manual_seed(79)
    gd, rd = os.path.join(tmp, "glob"), os.path.join(tmp, "reg")
    os.makedirs(gd), os.makedirs(rd)
    g_lats, g_lons = np.linspace(-90, 90, NTG), np.linspace(0, 360, NLG, endpoint=False)
    r_lats, r_lons = np.linspace(60, 40, NTR), np.linspace(320, 350, NLR)  # descending; past the last global longitude
    np.savez(os.path.join(gd, "coords.npz"), latitude=g_lats, longitude=g_lons)
    np.savez(os.path.join(rd, "coords.npz"), latitude=r_lats, longitude=r_lons)
    names = ["t2m", "msl", "10u"]
    json.dump(names, open(os.path.join(gd, "variables.json"), "w"))
    json.dump({"time_start": "2023-01-02", "time_end": "2023-01-31"}, open(os.path.join(gd, "dataset_info.json"), "w"))
    json.dump({"time_start": "2023-01-01", "time_end": "2023-01-03", "n_time": NT, "n_lon": NLR, "n_lat": NTR, "n_feat": NF},
              open(os.path.join(rd, "dataset_info.json"), "w"))
    mean = np.asarray([280.0, 1013.0, 1.5, 0.3], np.float64)   # msl in hPa-sized numbers: the fp16 series stays finite
    std = np.asarray([11.0, 9.0, 4.0, 0.2], np.float64)
    np.savez(os.path.join(rd, "scalers.npz"), mean=mean, std=std)
    series = (torch.randn(NT, NLR, NTR, NF, generator=g).numpy() * std + mean).astype(np.float16)
    series.tofile(os.path.join(rd, "data.npy"))
    N = 5
    preds = torch.randn(N, NLG * NTG, P * Cr, generator=g)
    truth = torch.randn(N, NLG * NTG, P * Cr, generator=g)
    offsets = [-6, -4, 30, -1, 2]  # global starts 4 steps after regional: base step -1 (skipped), 1, past the end, 4, 7
    bundle = {"predictions": preds, "ground_truth": truth, "n_features": Cr, "ar_steps": P, "obs_window": 2, "n_lon": NLG,
              "n_lat": NTG, "sample_offsets": offsets, "data_dir": "x"}
    torch.save(bundle, os.path.join(tmp, "pred_bundle.pt"))
    outp = os.path.join(tmp, "interp_out.pt")
    text = _run(script, ["--predictions", os.path.join(tmp, "pred_bundle.pt"), "--global-data", gd, "--region-data", rd,
                         "--per-channel", "--out", outp])
    res = torch.load(outp, weights_only=False)
    out.update({"interp:g_lats": g_lats, "interp:g_lons": g_lons, "interp:r_lats": r_lats, "interp:r_lons": r_lons,
                "interp:mean": mean, "interp:std": std, "interp:series_bits": series.view(np.uint16),
                "interp:predictions": preds.numpy(), "interp:ground_truth": truth.numpy(),
                "interp:sample_offsets": np.asarray(offsets, np.int64), "interp:names": np.asarray(names),
                "interp:dims": np.asarray([NLG, NTG, NLR, NTR, Cr, P, NF, NT, 2], np.int64),
                "interp:global_info": np.asarray(open(os.path.join(gd, "dataset_info.json")).read()),
                "interp:region_info": np.asarray(open(os.path.join(rd, "dataset_info.json")).read()),
                "interp:stdout": np.asarray(text.replace(tmp, "<tmp>")),
                "interp:out_keys": np.asarray(list(res)),
                "interp:out:interpolated_predictions": res["interpolated_predictions"].numpy(),
                "interp:out:regional_ground_truth": res["regional_ground_truth"].numpy(),
                "interp:out:variables": np.asarray(res["variables"]),
                "interp:out:region_lats": res["region_lats"], "interp:out:region_lons": res["region_lons"],
                "interp:out:n_matched": np.int64(res["n_matched"]),
                "interp:out:scalers_mean": res["scalers_mean"], "interp:out:scalers_std": res["scalers_std"]})
    print(text.replace(tmp, "<tmp>"))


def main():
    if not os.path.isdir(make_golden.REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    make_golden._placeholders()
    sys.path.insert(0, make_golden.REF)
    sys.path.insert(0, os.path.join(make_golden.REF, "scripts"))
    out = {"sets": np.asarray(list(SETS)), "sm_fields": np.asarray(SM_FIELDS)}
    tmp = tempfile.mkdtemp()
    _predict_runs(out, tmp)
    _create_obs_runs(out, tmp)
    _assim_dataset_runs(out, tmp)
    _interp_runs(out, tmp)
    path = os.path.join(HERE, "predict_vectors.npz")
    np.savez_compressed(path, **out)
    print("wrote predict_vectors.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
