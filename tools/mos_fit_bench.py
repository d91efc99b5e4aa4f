"""Fitting the learned MOS on the device (graphcast_lite_amd.mos.MOSFitter) next to sklearn's
HistGradientBoostingRegressor on the host, on two synthetic MOS-like tables:

  a  the reference-sized table: 61 000 x 20, 500 iterations, early stopping off
  b  a 128-station table: 7 800 000 x 20, 100 iterations, early stopping off

Device time is wall time of `MOSFitter.fit` (host thresholds, upload, binning, every tree, the forest read back);
sklearn's is `fit` with the same hyper-parameters on this machine's CPUs (OMP_NUM_THREADS).  Medians of `--runs` runs.

    python tools/mos_fit_bench.py                      # both tables -> profiles/mos_fit_bench.json
    python tools/mos_fit_bench.py --profile            # + per-kernel shares from a counters-free
                                                       #   `rocprofv3 --kernel-trace --stats` run of table b (one fit)

The histogram kernel's traffic is what one pass must move (per row and feature one bin byte; per row and wave the row
index and the gradient, 8 bytes, once per four features) against the 8 TB/s HBM peak; the kernel is bound by its
sequential float64 adds, not by that traffic.
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": dict(n=61_000, max_iter=500), "b": dict(n=7_800_000, max_iter=100)}
HBM_PEAK = 8.0e12


def table(n, seed=0):
    rng = np.random.default_rng(seed)
    hour = rng.integers(0, 24, n)
    doy = rng.integers(1, 366, n)
    t2m = rng.normal(0, 15, n)
    X = np.column_stack([
        t2m, t2m - rng.gamma(2, 2, n), rng.gamma(2, 2, n), rng.uniform(-1, 1, n), rng.uniform(-1, 1, n),
        rng.normal(990, 15, n), np.round(rng.uniform(0, 100, n)), rng.uniform(0, 600, n),
        np.where(rng.random(n) < 0.7, 0.0, rng.exponential(0.5, n)), np.sin(2 * np.pi * hour / 24),
        np.cos(2 * np.pi * hour / 24), np.sin(2 * np.pi * doy / 365.25), np.cos(2 * np.pi * doy / 365.25),
        rng.uniform(-60, 60, n), rng.gamma(2, 2, n), t2m + rng.normal(0, 3, n), rng.normal(0, 3, n),
        rng.integers(0, 128, n) * 0.05 + 53.0, rng.integers(0, 128, n) * 0.05 + 89.0, rng.uniform(90, 480, n)])
    y = (0.08 * X[:, 0] - 1.5 * X[:, 10] + 0.004 * X[:, 7] * (X[:, 13] > 0) - 0.3 * np.tanh(X[:, 16])
         + 0.5 * (X[:, 8] > 0) + rng.normal(0, 0.8, n))
    return np.ascontiguousarray(X), y


def run_case(name, runs, with_sklearn):
    import torch

    from graphcast_lite_amd import mos

    cfg = CASES[name]
    X, y = table(cfg["n"])
    kw = dict(max_iter=cfg["max_iter"], early_stopping=False)
    res = {"case": name, "rows": cfg["n"], "features": 20, "max_iter": cfg["max_iter"], "runs": runs}
    mos.fit_learned_mos(X[:5000], y[:5000], max_iter=4, early_stopping=False)  # library load, allocator warm-up
    dev_times = []
    for r in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fitter = mos.MOSFitter(**kw)
        fit = fitter.fit(X, y)
        torch.cuda.synchronize()
        dev_times.append(time.perf_counter() - t0)
        print(f"[{name}] device fit {r}: {dev_times[-1]:.3f} s ({fit.forest.num_nodes} nodes, {fitter.launch_mode})",
              flush=True)
    res["device_s"] = dev_times
    res["device_median_s"] = statistics.median(dev_times)
    res["forest_nodes"] = int(fit.forest.num_nodes)
    if with_sklearn:
        try:
            from sklearn.ensemble import HistGradientBoostingRegressor as HGB
        except ImportError:
            res["sklearn"] = "not importable on this machine: device side only"
            with_sklearn = False
    if with_sklearn:
        sk_times = []
        for r in range(runs):
            t0 = time.perf_counter()
            model = HGB(max_iter=cfg["max_iter"], max_depth=8, learning_rate=0.05, min_samples_leaf=20,
                        l2_regularization=0.1, early_stopping=False, random_state=42).fit(X, y)
            sk_times.append(time.perf_counter() - t0)
            print(f"[{name}] sklearn fit {r}: {sk_times[-1]:.3f} s", flush=True)
        res["sklearn_s"] = sk_times
        res["sklearn_median_s"] = statistics.median(sk_times)
        res["sklearn_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        res["speedup_median"] = res["sklearn_median_s"] / res["device_median_s"]
        pd, ps = fit.forest.predict_host(X[:2000]), model.predict(X[:2000])
        res["max_abs_prediction_diff_2000_rows"] = float(np.max(np.abs(pd - ps)))
    return res


def profile_case(name):
    """Per-kernel shares of one device fit of table `name` from rocprofv3's kernel stats (a run of its own)."""
    out = tempfile.mkdtemp(prefix="mos_fit_prof_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable,
           os.path.abspath(__file__), "--case", name, "--runs", "1", "--no-sklearn", "--out", ""]
    subprocess.run(cmd, check=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        return {"error": "no kernel_stats.csv written"}
    rows = list(csv.DictReader(open(files[0])))
    fit_rows = [r for r in rows if re.search(r"fit_\w+_kernel", r["Name"])]
    total = sum(float(r["TotalDurationNs"]) for r in fit_rows) or 1.0
    shares = [{"kernel": re.search(r"(fit_\w+)", r["Name"]).group(1), "calls": int(r["Calls"]),
               "total_ms": float(r["TotalDurationNs"]) / 1e6, "avg_us": float(r["AverageNs"]) / 1e3, "share": float(r["TotalDurationNs"]) / total}
              for r in sorted(fit_rows, key=lambda r: -float(r["TotalDurationNs"]))]
    res = {"case": name, "fit_kernels_total_ms": total / 1e6, "kernels": shares,
           "note": "includes the 4-tree warm-up fit"}
    cfg = CASES[name]
    hist = next((s for s in shares if "fit_hist_kernel" in s["kernel"]), None)
    if hist:
        # every launch counted at the root's bytes would overstate it: the slowest launches are the root passes, so take
        # the maximum launch time from the trace when it is there, else report the root-pass bytes only
        root_bytes = cfg["n"] * 20 + cfg["n"] * 8 * 5
        res["hist_root_pass_bytes"] = root_bytes
        trace = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if trace:
            d = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in csv.DictReader(open(trace[0]))
                 if "fit_hist_kernel" in r["Kernel_Name"]]
            if d:
                root_ns = statistics.median(sorted(d)[-cfg["max_iter"]:])  # the max_iter longest: the root passes
                res["hist_root_pass_us"] = root_ns / 1e3
                res["hist_root_pass_bytes_per_s"] = root_bytes / (root_ns * 1e-9)
                res["hist_root_pass_fraction_of_8TBps"] = res["hist_root_pass_bytes_per_s"] / HBM_PEAK
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["a", "b", "both"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mos_fit_bench.json"))
    args = ap.parse_args()
    names = ["a", "b"] if args.case == "both" else [args.case]
    result = {"tool": "tools/mos_fit_bench.py", "cases": [run_case(n, args.runs, not args.no_sklearn) for n in names]}
    if args.profile:
        result["profile"] = profile_case("b" if "b" in names else names[0])
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
