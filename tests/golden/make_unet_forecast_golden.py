"""Generate the regional U-Net forecaster's fixture by RUNNING the reference's own scripts (src/unet/predict.py and
src/unet/predict_v2.py) with CPU torch.

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_unet_forecast_golden.py

The case is tests/helpers/unet_forecast_case.py.  Output (data only):

    unet_forecast_data/         data.npy (raw fp16 [48, 12, 9, 7]), dataset_info.json, scalers.npz, variables.json: smooth
                                travelling waves plus noise, six channels used of seven stored; channel 5 constant in time
    unet_forecast_data_const/   the same but channel 4 is constant in space too ("lsm")
    unet_forecast_v1.pt         state dict of the reference's WeatherUNet(12, 6, 8), random (unet_case.randomise_)
    unet_forecast_v2.pt         state dict of the reference's WeatherUNetV2(12, 6, 8, 2, 2), random (unet_v2_case.randomise_);
                                in both the output convolution is scaled down, so the forecast stays near persistence, and
                                the weights are rounded to float16 and stored as float16 (load_state_dict casts them back
                                exactly), which keeps the V2 file at 0.6 MB instead of 1.2 MB
    unet_forecast_exp_<case>/config.json   the experiment configs of unet_forecast_case.CASES
    unet_forecast_ref.npz       <case>.ref32.<name>: the accumulators the reference script held when its main() returned
                                (read from that frame's locals by a profile hook); <case>.f64.<name>: the float64
                                restatement of the same loop (unet_forecast_case.forecast_loop)
    unet_forecast_ref.json      per case the tables the script printed (its stdout from the rule of '=' on: the lines
                                before it name the run's paths) and the distance between ref32 and f64 per family

The generator asserts, per case: the float32 restatement of the loop over the reference's module reproduces the script's
accumulators bit for bit (so the restatement is the script's loop); no dynamic channel comes near the ACC gate in float32
(pn, tn > 1e-3); the tables printed from the float64 accumulators equal the script's stdout character for character
except the cells unet_forecast_case.UNSTABLE lists, and so do the tables printed from the float64 accumulators moved by
unet_forecast_case.MARGIN times the float32 / float64 distance either way (so every other printed digit is stable under the
tolerance the GPU test grants); and `forecast_tables` reproduces the stdout from the recorded accumulators.
"""
import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.path.insert(0, ROOT)
import make_golden  # noqa: E402  (where the reference checkout lives)
import unet_case as UC  # noqa: E402
import unet_forecast_case as FC  # noqa: E402
import unet_v2_case as VC  # noqa: E402

REF = make_golden.REF
NAMES = ["t2m", "u10", "z@500", "toa", "msl", "z_sfc", "tp"]
_ACC_LOCALS = {"sum_se": "sum_se_h", "sum_se_base": "sum_se_base_h", "sum_nse": "sum_nse_h", "sum_nse_base": "sum_nse_base_h",
               "sum_acc": "sum_acc_h", "acc_count": "acc_count_h", "count": "count_h"}


def _series(const_channel_4: bool):
    rng = np.random.default_rng(FC.SEED)
    t = np.arange(FC.T)[:, None, None]
    lon = np.arange(FC.N_LON)[None, :, None] / FC.N_LON
    lat = np.arange(FC.N_LAT)[None, None, :] / (FC.N_LAT - 1)

    def wave(k, speed, phase):
        return np.sin(2 * np.pi * (k * lon + speed * t) + phase) * np.cos(np.pi * (lat - 0.5) * 0.9) + 0.4 * np.cos(
            2 * np.pi * (lon - 2 * lat + 0.5 * speed * t) + 2 * phase)

    def noise(s):
        return s * rng.standard_normal((FC.T, FC.N_LON, FC.N_LAT))

    f = np.zeros((FC.T, FC.N_LON, FC.N_LAT, FC.CT))
    f[..., 0] = 280.0 + 8.0 * wave(1, 0.031, 0.3) + noise(0.8)
    f[..., 1] = 5.0 * wave(2, 0.043, 1.1) + noise(0.6)
    f[..., 2] = 55.0 + 1.2 * wave(1, 0.027, 2.0) + noise(0.1)
    f[..., 3] = 30.0 + 2.0 * wave(1, 0.125, 0.0)
    f[..., 4] = 101.0 + 1.2 * wave(2, 0.037, 0.7) + noise(0.1)
    f[..., 5] = (8.0 * (wave(1, 0.0, 0.5) + 1.5)) * np.ones((FC.T, 1, 1))
    f[..., 6] = np.abs(noise(1.0))
    if const_channel_4:
        f[..., 4] = 0.3
    return f.astype(np.float16)


def _write_dataset(path, series, names):
    os.makedirs(path, exist_ok=True)
    series.tofile(os.path.join(path, "data.npy"))
    with open(os.path.join(path, "dataset_info.json"), "w") as fh:
        json.dump({"n_time": FC.T, "n_lon": FC.N_LON, "n_lat": FC.N_LAT, "n_feat": FC.CT}, fh)
    x = series.astype(np.float64).reshape(-1, FC.CT)
    mean, std = x.mean(0), x.std(0)
    mean[std < 1e-6], std[std < 1e-6] = 0.1, 0.7  # the constant channel: normalised to a constant that is no short binary fraction
    np.savez(os.path.join(path, "scalers.npz"), mean=mean.astype(np.float32), std=std.astype(np.float32))
    with open(os.path.join(path, "variables.json"), "w") as fh:
        json.dump(names, fh)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run_script(mod, argv):
    """(stdout, the accumulators main() held when it returned) of one run of a reference script."""
    held = {}

    def hook(frame, event, arg):
        if event == "return" and frame.f_code.co_name == "main" and frame.f_code.co_filename == mod.__file__:
            held.update({k: np.array(frame.f_locals[v]) for k, v in _ACC_LOCALS.items()})

    out, old = io.StringIO(), sys.argv
    sys.argv = ["predict"] + argv
    sys.setprofile(hook)
    try:
        with contextlib.redirect_stdout(out):
            mod.main()
    finally:
        sys.setprofile(None)
        sys.argv = old
    assert held, "the profile hook did not see main() return"
    return out.getvalue(), held


def _tail(stdout):
    return stdout[stdout.index("\n" + "=" * 70):]


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    from graphcast_lite_amd.unet_predict import forecast_tables

    _write_dataset(FC.DATA, _series(False), NAMES)
    _write_dataset(FC.DATA_CONST, _series(True), NAMES[:4] + ["lsm"] + NAMES[5:])

    sys.path.insert(0, REF)
    scripts = {"v1": _load("_ref_unet_predict", os.path.join(REF, "src", "unet", "predict.py")),
               "v2": _load("_ref_unet_predict_v2", os.path.join(REF, "src", "unet", "predict_v2.py"))}
    torch.manual_seed(0)
    models = {"v1": UC.randomise_(scripts["v1"].WeatherUNet(FC.OBS * FC.C, FC.C, FC.BASE), FC.SEED).eval(),
              "v2": VC.randomise_(scripts["v2"].WeatherUNetV2(FC.OBS * FC.C, FC.C, FC.BASE, FC.HEADS, FC.MODES), FC.SEED + 1).eval()}
    for arch, m in models.items():
        with torch.no_grad():
            m.out_conv.weight.mul_(0.15)
            m.out_conv.bias.mul_(0.15)
            for t in m.state_dict().values():  # values a float16 file holds exactly: the checkpoints stay small
                if t.is_floating_point():
                    t.copy_(t.half().float())
        torch.save({k: v.half() if v.is_floating_point() else v for k, v in m.state_dict().items()}, FC.CKPT[arch])
        print(f"{FC.CKPT[arch]}: {os.path.getsize(FC.CKPT[arch]) / 1e3:.1f} kB, {m.num_params} parameters")

    arrays, text = {}, {}
    starts = FC.split_starts()
    for case, (arch, data, static, forcing, ar) in FC.CASES.items():
        os.makedirs(FC.exp_dir(case), exist_ok=True)
        with open(os.path.join(FC.exp_dir(case), "config.json"), "w") as fh:
            json.dump(FC.case_config(case), fh, indent=2)
        argv = [FC.exp_dir(case), "--ckpt", FC.CKPT[arch], "--data-dir", data] + (["--ar-steps", str(ar)] if ar else [])
        stdout, ref32 = _run_script(scripts[arch], argv)
        ar_steps = ar or FC.PRED
        series, mean, std, names = FC.load_dataset(data)
        sd = {k: v.clone() for k, v in models[arch].state_dict().items()}
        rf = ((FC.OBS - 1) * FC.C, FC.OBS * FC.C)
        loop32, min_norm = FC.forecast_loop(lambda x, m=models[arch]: x[:, rf[0]:rf[1]] + m(x), series, starts, mean, std,
                                            static, forcing, ar_steps, dtype=torch.float32)
        for k in ref32:
            assert np.array_equal(loop32[k], ref32[k]), f"{case}: the float32 restatement of the loop misses the script's {k}"
        assert min_norm > 1e-3, f"{case}: a dynamic channel's centred norm is {min_norm:.3e}: too near the ACC gate"
        f64, _ = FC.forecast_loop(FC.network(arch, sd), series, starts, mean, std, static, forcing, ar_steps)
        d = FC.distance(ref32, f64)
        H, W = FC.N_LAT, FC.N_LON
        t32 = forecast_tables(ref32, names, static, forcing, H, W, len(starts))
        t64 = forecast_tables(f64, names, static, forcing, H, W, len(starts))
        assert t32 == _tail(stdout), f"{case}: forecast_tables misses the script's stdout:\n{t32}\n---\n{_tail(stdout)}"
        assert FC.mask_unstable(case, t64) == FC.mask_unstable(case, t32), \
            f"{case}: a printed digit is not stable under float32 -> float64:\n{t32}\n---\n{t64}"
        for sign in (-1.0, 1.0):  # and under the whole tolerance the GPU test grants: MARGIN times the distance, either way
            tp = forecast_tables(FC.perturbed(f64, d, sign), names, static, forcing, H, W, len(starts))
            assert FC.mask_unstable(case, tp) == FC.mask_unstable(case, t32), \
                f"{case}: a printed digit moves within {FC.MARGIN} x the distance:\n{t32}\n---\n{tp}"
        for which, acc in (("ref32", ref32), ("f64", f64)):
            for k, v in acc.items():
                arrays[f"{case}.{which}.{k}"] = np.asarray(v)
        text[case] = {"tables": _tail(stdout), "distance": d, "n_samples": len(starts), "min_norm": min_norm}
        print(f"{case}: distance(ref32, f64) = " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()) + f"; min norm {min_norm:.3e}")
        print(_tail(stdout))
    np.savez(FC.REF_NPZ, **arrays)
    with open(FC.REF_JSON, "w") as fh:
        json.dump(text, fh, indent=1, ensure_ascii=False)
    for p in (FC.REF_NPZ, FC.REF_JSON, os.path.join(FC.DATA, "data.npy")):
        print(f"wrote {p} ({os.path.getsize(p) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
