"""The regional U-Net forecaster's test case: the fixture of tests/golden/make_unet_forecast_golden.py (a tiny dataset in
two variants, two checkpoints, four experiment cases with the reference scripts' recorded accumulators and stdout), numpy
restatements of the loader + Grid2DDataset and of one autoregressive step's arithmetic, and the float64 restatement of
the whole loop of src/unet/predict_v2.py:113-180 (network included, through unet_case / unet_v2_case)."""
import json
import math
import os

import numpy as np
import torch

import unet_case as UC
import unet_v2_case as VC

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
DATA = os.path.join(GOLDEN, "unet_forecast_data")              # six channels that all vary in space
DATA_CONST = os.path.join(GOLDEN, "unet_forecast_data_const")  # the same but channel 4 is constant in space ("lsm")
CKPT = {"v1": os.path.join(GOLDEN, "unet_forecast_v1.pt"), "v2": os.path.join(GOLDEN, "unet_forecast_v2.pt")}
REF_NPZ = os.path.join(GOLDEN, "unet_forecast_ref.npz")
REF_JSON = os.path.join(GOLDEN, "unet_forecast_ref.json")

T, N_LON, N_LAT, CT, C, OBS, PRED = 48, 12, 9, 7, 6, 2, 3
BASE, HEADS, MODES = 8, 2, 2
SEED = 97531
MARGIN = 4.0  # the HIP path may be this many times as far from float64 as the reference's float32 run: the suite's rule for
              # the U-Nets themselves (unet_case.check), whose summation orders differ from torch's in the same way
FAMILIES = ("sum_se", "sum_se_base", "sum_nse", "sum_nse_base", "sum_acc")

# name -> (architecture, dataset, static channels, forcing channels, ar_steps or None for the config's)
CASES = {
    "v1_carry": ("v1", DATA_CONST, [4], [3], None),   # the constant static channel: its ACC cell counts rounding noise
    "v1_plain": ("v1", DATA, [], [], None),
    "v2_plain": ("v2", DATA, [], [], None),
    "v2_long": ("v2", DATA, [5], [3], 5),             # ar_steps 5 > pred_steps 3: two horizons with count 0
}


# Printed cells that are not stable between float32 and float64, (channel, column) of the per-channel table.  The ACC of
# the spatially constant static channel: after removing the field mean the reference's float32 arithmetic is left with
# rounding noise, which it correlates and counts (predict_v2.py:168-175); in float64 the centred field is exactly zero.
UNSTABLE = {"v1_carry": [(4, "ACC")]}


def mask_unstable(case, text):
    """`text` (what forecast_tables returns) with the UNSTABLE cells of the case starred out."""
    import re

    lines = text.split("\n")
    first = next(i for i, ln in enumerate(lines) if ln.startswith("Per-channel metrics overall"))
    for c, column in UNSTABLE.get(case, []):
        assert column == "ACC"
        for i in range(first + 2, len(lines)):
            if re.match(rf"^\s+{c}\s", lines[i]):
                lines[i] = re.sub(r"^(\s+\d+\s+\S+\s+)\S+", r"\1******", lines[i])
    return "\n".join(lines)


def exp_dir(case):
    return os.path.join(GOLDEN, "unet_forecast_exp_" + case)


def case_config(case):
    arch, data, static, forcing, _ = CASES[case]
    cfg = {"data_dir": os.path.relpath(data, os.path.dirname(os.path.dirname(GOLDEN))), "num_features": C, "obs_window": OBS,
           "pred_steps": PRED, "base_filters": BASE, "static_channels": static, "forcing_channels": forcing}
    if arch == "v2":
        cfg.update(attn_heads=HEADS, spectral_modes=MODES)
    return cfg


def load_dataset(data_dir):
    """(series fp16 [T, lon, lat, Ct], mean [C], std [C], variable names) of a fixture dataset directory."""
    with open(os.path.join(data_dir, "dataset_info.json")) as fh:
        info = json.load(fh)
    shape = (info["n_time"], info["n_lon"], info["n_lat"], info["n_feat"])
    series = np.array(np.memmap(os.path.join(data_dir, "data.npy"), dtype=np.float16, mode="r", shape=shape))
    sc = np.load(os.path.join(data_dir, "scalers.npz"))
    with open(os.path.join(data_dir, "variables.json")) as fh:
        names = json.load(fh)
    return series, sc["mean"][:C].astype(np.float32), sc["std"][:C].astype(np.float32), names


def split_starts(n_time=T, obs=OBS, pred=PRED, test_fraction=0.2):
    """The window starts of the `test_only` split of a one-chunk series (dataloader_chunked.py:138-166)."""
    idx = list(range(max(0, n_time - (obs + pred) + 1)))
    test = idx[int(len(idx) * (1 - test_fraction)):]
    return test[len(test) // 2:]


def recorded():
    """(npz of the recorded accumulators, json with the tables the scripts printed and the distances)."""
    with open(REF_JSON) as fh:
        return np.load(REF_NPZ, allow_pickle=False), json.load(fh)


def recorded_acc(npz, case, which):
    """The accumulators of a case as `forecast_tables` takes them; which: "ref32" (the reference script's own run) or
    "f64" (the float64 restatement)."""
    acc = {k: npz[f"{case}.{which}.{k}"] for k in FAMILIES + ("acc_count", "count")}
    return acc


# ---------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------
def window_np(series, t0, mean, std, n_feat, first, frames):
    """Frames t0 + first .. + frames of the loader (dataloader_chunked.py:202-218) as Grid2DDataset views them
    (predict_v2.py:36-40): float32 [frames * C, H = n_lat, W = n_lon]."""
    w = series[t0 + first:t0 + first + frames, :, :, :n_feat].astype(np.float32)
    w = (w - mean) / std
    f, n_lon, n_lat, _ = w.shape
    return np.ascontiguousarray(w.transpose(0, 3, 2, 1)).reshape(frames * n_feat, n_lat, n_lon)


def kinds_of(n_feat, static, forcing):
    kind = np.zeros(n_feat, dtype=np.uint8)
    kind[list(static)] = 1
    kind[list(forcing)] = 2  # the later assignment wins (predict_v2.py:142-148)
    return kind


def step_np(out, X, series, t0, kind, mean, std, obs, step):
    """One sample's step in the kernel's arithmetic: out' (float32, exact), and per channel the ten sums
    [se_phys, se_base_phys, se_norm, se_base_norm, sum p, sum g, Spp, Stt, Spt, corr or nan] - differences and squares in
    float32 as numpy forms them (predict_v2.py:156-163), every sum over the pixels and the centred part in float64."""
    n_feat = out.shape[0]
    g = window_np(series, t0, mean, std, n_feat, obs + step, 1)
    bl = window_np(series, t0, mean, std, n_feat, obs - 1, 1)
    p = out.copy()
    for c in range(n_feat):
        if kind[c] == 1:
            p[c] = X[(obs - 1) * n_feat + c]
        elif kind[c] == 2:
            p[c] = g[c]
    sums = np.zeros((n_feat, 10), dtype=np.float64)
    for c in range(n_feat):
        pp, gp, bp = p[c] * std[c] + mean[c], g[c] * std[c] + mean[c], bl[c] * std[c] + mean[c]
        assert pp.dtype == np.float32
        sums[c, 0] = ((pp - gp) ** 2).astype(np.float64).sum()
        sums[c, 1] = ((bp - gp) ** 2).astype(np.float64).sum()
        sums[c, 2] = ((p[c] - g[c]) ** 2).astype(np.float64).sum()
        sums[c, 3] = ((bl[c] - g[c]) ** 2).astype(np.float64).sum()
        p64, g64 = p[c].astype(np.float64), g[c].astype(np.float64)
        sums[c, 4], sums[c, 5] = p64.sum(), g64.sum()
        dp, dg = p64 - p64.sum() / p64.size, g64 - g64.sum() / g64.size
        sums[c, 6], sums[c, 7], sums[c, 8] = (dp * dp).sum(), (dg * dg).sum(), (dp * dg).sum()
        pn, tn = math.sqrt(sums[c, 6]), math.sqrt(sums[c, 7])
        sums[c, 9] = sums[c, 8] / (pn * tn) if pn > 1e-8 and tn > 1e-8 else np.nan
    return p, sums


def network(arch, sd):
    """x [1, obs * C, H, W] -> out [1, C, H, W] with x_last added, in the dtype of x, from a state dict."""
    rf = ((OBS - 1) * C, OBS * C)
    if arch == "v1":
        return lambda x: UC.functional_unet(sd, x, rf)
    return lambda x: VC.functional_unet_v2(sd, x, HEADS, MODES, rf)


def forecast_loop(net, series, starts, mean, std, static, forcing, ar_steps, dtype=torch.float64, n_feat=C, obs=OBS,
                  pred=PRED):
    """predict_v2.py:113-180 with everything behind the loader in `dtype` (the loader's float32 windows are the data).
    Returns the accumulators and the smallest centred norm (pn or tn) met on a dynamic channel."""
    npdt = np.float64 if dtype == torch.float64 else np.float32
    acc = {k: np.zeros((ar_steps, n_feat), dtype=np.float64) for k in FAMILIES}
    acc["acc_count"] = np.zeros((ar_steps, n_feat), dtype=np.int64)
    acc["count"] = np.zeros(ar_steps, dtype=np.int64)
    mean_d, std_d = mean.astype(npdt), std.astype(npdt)
    no_loss = set(static) | set(forcing)
    min_norm = math.inf
    for t0 in starts:
        X = window_np(series, t0, mean, std, n_feat, 0, obs).astype(npdt)
        Y = window_np(series, t0, mean, std, n_feat, obs, pred).astype(npdt).reshape(pred, n_feat, *X.shape[1:])
        cur = X.reshape(obs, n_feat, *X.shape[1:])
        bl = cur[-1].copy()
        for s in range(min(ar_steps, pred)):
            with torch.no_grad():
                out = net(torch.from_numpy(cur.reshape(1, obs * n_feat, *X.shape[1:]).copy()).to(dtype))[0].numpy().copy()
            for ch in static:
                out[ch] = cur[-1, ch]
            for ch in forcing:
                out[ch] = Y[s, ch]
            gt = Y[s]
            for c in range(n_feat):
                pp, gp, bp = out[c] * std_d[c] + mean_d[c], gt[c] * std_d[c] + mean_d[c], bl[c] * std_d[c] + mean_d[c]
                acc["sum_se"][s, c] += ((pp - gp) ** 2).sum()
                acc["sum_se_base"][s, c] += ((bp - gp) ** 2).sum()
                acc["sum_nse"][s, c] += ((out[c] - gt[c]) ** 2).sum()
                acc["sum_nse_base"][s, c] += ((bl[c] - gt[c]) ** 2).sum()
                p, t = out[c].flatten(), gt[c].flatten()
                p, t = p - p.mean(), t - t.mean()
                pn, tn = np.sqrt((p ** 2).sum()), np.sqrt((t ** 2).sum())
                if c not in no_loss:
                    min_norm = min(min_norm, float(pn), float(tn))
                if pn > 1e-8 and tn > 1e-8:
                    acc["sum_acc"][s, c] += (p * t).sum() / (pn * tn)
                    acc["acc_count"][s, c] += 1
            acc["count"][s] += X.shape[1] * X.shape[2]
            cur = np.concatenate([cur[1:], out[None]], axis=0)
    return acc, min_norm


def distance(acc, ref):
    """Per family the largest distance of `acc` from `ref` over the cells: relative to the cell for the four squared-error
    sums (cells that are exactly zero in both - a forcing channel, a static channel against itself - count as 0),
    absolute per counted sample for acc_sum (a correlation is of order one).  Cells whose ACC counts differ are left
    out of acc_sum's distance: the caller compares the counts itself."""
    d = {}
    for k in FAMILIES[:4]:
        a, r = np.asarray(acc[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where((a == 0) & (r == 0), 0.0, np.abs(a - r) / np.abs(r))
        d[k] = float(rel.max())
    same = np.asarray(acc["acc_count"]) == np.asarray(ref["acc_count"])
    n = np.maximum(np.asarray(ref["acc_count"]), 1)
    d["sum_acc"] = float((np.abs(np.asarray(acc["sum_acc"]) - np.asarray(ref["sum_acc"])) / n)[same].max())
    return d


def perturbed(acc, d, sign, margin=MARGIN):
    """`acc` moved by margin x the distances d, the model's sums one way and the baseline's the other (the direction that
    moves skill most), acc_sum by that much per counted sample."""
    out = {k: np.array(v) for k, v in acc.items()}
    for k, s in (("sum_se", sign), ("sum_nse", sign), ("sum_se_base", -sign), ("sum_nse_base", -sign)):
        out[k] = out[k] * (1.0 + s * margin * d[k])
    out["sum_acc"] = out["sum_acc"] + sign * margin * d["sum_acc"] * out["acc_count"]
    return out
