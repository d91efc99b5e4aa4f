"""The host side of `graphcast_lite_amd.regional_train`, without a GPU: log, table and result lines character for character
against what the reference's three scripts printed and wrote in a recorded run (tests/golden/regional_main_vectors.npz,
written by tests/golden/make_regional_train_golden.py), the epoch loop's files and patience, the `--precompute` argument rules, the record-size arithmetic and the argument
validation of the three entry points (which returns before any HIP call)."""
import ctypes as C
import json
import os
import re
import types

import numpy as np

import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN


def _main_fx():
    return np.load(os.path.join(GOLDEN, "regional_main_vectors.npz"))


def test_dual_log_lines_equal_the_reference_prints():
    """Every line `scripts/train_dual_mesh.py` logged in its recorded run, rebuilt from the values its epoch functions
    returned in that run."""
    from graphcast_lite_amd.regional_train import DUAL_HEADER, ar_line, dual_line, dual_test_line, overfit_line

    z = _main_fx()
    log = str(z["dual:log"]).split("\n")
    train, ev = z["dual:train"], z["dual:eval"]
    assert log[0] == ar_line(2) and log[1] == DUAL_HEADER and log[2] == "-" * 59
    best = float("inf")
    for e in range(2):
        mark = " *" if ev[e][0] < best else ""
        best = min(best, float(ev[e][0]))
        assert log[3 + e] == dual_line(e, float(train[e]), float(ev[e][0]), float(ev[e][1]), best, mark), log[3 + e]
    assert "\n".join(log[5:7]) == dual_test_line(float(ev[2][0]), float(ev[2][1]))
    assert log[7] == "Results saved to <tmp>/exp/results" and log[8:] == [""]
    # the overfit lines: the recorded text re-formatted from its own numbers comes out the same
    lines = [ln for ln in str(z["dual:stdout"]).split("\n") if ln.startswith("    step")]
    assert len(lines) == 11
    for ln in lines:
        step, loss, mean_abs, max_abs = re.match(r"    step +(\d+): loss=(\S+)  \|correction\|=(\S+)  max=(\S+)$", ln).groups()
        assert overfit_line(int(step), float(loss), float(mean_abs), float(max_abs)) == ln
    assert [str(f) for f in z["dual:files"]] == ["best_model.pth", "best_regional.pth", "results.json", "training_log.txt"]
    assert list(json.loads(str(z["dual:results_json"]))) == ["best_val_loss", "test_loss", "test_correction_skill", "roi",
                                                             "reg_mesh_level", "reg_steps", "cross_k", "hidden_dim",
                                                             "ar_steps"]
    assert not any(str(k).startswith("global_model.") for k in z["dual:regional_keys"])


def test_roi_log_lines_equal_the_reference_prints():
    from graphcast_lite_amd.regional_train import ROI_HEADER, correction_line, roi_line, roi_test_line

    z = _main_fx()
    log = str(z["roi:log"]).split("\n")
    train, ev = z["roi:train"], z["roi:eval"]
    assert log[0] == ROI_HEADER and log[1] == "-" * 55
    best = float("inf")
    for e in range(2):
        mark = " *" if ev[e][0] < best else ""
        best = min(best, float(ev[e][0]))
        assert log[2 + e] == roi_line(e, float(train[e]), float(ev[e][0]), float(ev[e][1]), best, mark), log[2 + e]
    assert "\n".join(log[4:6]) == roi_test_line(float(ev[2][0]), float(ev[2][1]))
    assert log[6] == "Results saved to <tmp>/roi_exp/results"
    for ln in [ln for ln in str(z["roi:stdout"]).split("\n") if "[Correction]" in ln]:
        vals = re.match(r"  \[Correction\] mean_abs=(\S+), max_abs=(\S+), baseline_mse=(\S+)$", ln).groups()
        assert correction_line(*(float(v) for v in vals)) == ln
    assert [str(f) for f in z["roi:files"]] == ["best_head.pth", "best_model.pth", "results.json", "training_log.txt"]
    assert list(json.loads(str(z["roi:results_json"]))) == ["best_val_loss", "test_loss", "test_regional_acc", "roi",
                                                            "hidden_dim", "processor_steps", "roi_k", "lr", "pretrained",
                                                            "data_dir"]


def test_regional_tables_equal_the_reference_prints():
    """`regional_tables` and `predict_results` fed the state of the reference's own `StreamingMetrics` objects: the
    summary, the per-horizon lines, the three per-horizon per-channel tables, the overall table and the JSON keys."""
    from graphcast_lite_amd.regional_train import UNITS, RegionScores, predict_results, regional_tables

    z = _main_fx()
    sc, rpc, apc = z["predict:scores"], z["predict:rmse_per_channel"], z["predict:acc_per_channel"]
    obj = [RegionScores(sc[i][0], sc[i][1], sc[i][2], sc[i][3], rpc[i], apc[i]) for i in range(len(sc))]
    AR = (len(obj) - 2) // 2
    horizons = [(obj[2 + p], obj[2 + AR + p]) for p in range(AR)]
    variables = [str(v) for v in z["variables"]]
    res = predict_results((obj[0], obj[1]), horizons, AR, tuple(z["roi"]), 961, 5, 121, variables)
    said = []
    regional_tables(res, variables, z["std"], say=said.append)
    want = str(z["predict:stdout"])
    want = want[want.index("\n" + "=" * 60):want.index("\nSaved to")]
    assert "\n".join(said) + "\n" == want, "\n".join(said)
    ref = json.loads(str(z["predict:results_json"]))
    assert list(res) == list(ref) and json.loads(json.dumps(res)) == ref
    assert [list(h) for h in res["per_horizon"]] == [list(h) for h in ref["per_horizon"]]
    assert list(res["regional_overall"]) == list(ref["regional_overall"]) and list(res["per_channel"]) == list(ref["per_channel"])
    assert UNITS["tcwv"] == "kg/m²" and len(UNITS) == 19
    # without --per-channel: the summary only, and no per_channel entry
    short = []
    res2 = predict_results((obj[0], obj[1]), horizons, AR, tuple(z["roi"]), 961, 5, 121)
    regional_tables(res2, None, None, say=short.append)
    assert short == said[:len(short)] and short[-1] == "=" * 60 and "per_channel" not in res2


class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.global_model = nn.Linear(2, 2)
        self.head = nn.Linear(2, 1)
        self.register_buffer("roi_mask", torch.tensor([True, False]))


def test_fit_loop_files_patience_and_best_weights(tmp_path, capsys):
    from graphcast_lite_amd.regional_train import MAX_PATIENCE, DUAL_HEADER, dual_line, fit_loop

    m = _Tiny()
    vals = [3.0, 2.0] + [2.5] * 30  # the best epoch is the second; ten worse ones follow
    seen = []

    def run_train(epoch):
        with torch.no_grad():
            m.head.weight.fill_(float(epoch))  # the weights of epoch 1 are the best ones
        seen.append(epoch)
        return 1.0 / (epoch + 1)

    out = str(tmp_path)
    best = fit_loop(m, run_train, lambda: (vals[len(seen) - 1], 0.25), out, 40, DUAL_HEADER, "-" * 59, dual_line,
                    "best_regional.pth")
    assert best == 2.0 and MAX_PATIENCE == 10 and seen == list(range(12))
    assert sorted(os.listdir(out)) == ["best_model.pth", "best_regional.pth", "training_log.txt"]
    reg = torch.load(os.path.join(out, "best_regional.pth"), weights_only=True)
    assert sorted(reg) == ["head.bias", "head.weight", "roi_mask"] and not any(k.startswith("global_model.") for k in reg)
    full = torch.load(os.path.join(out, "best_model.pth"), weights_only=True)
    assert "global_model.weight" in full and float(full["head.weight"][0, 0]) == 1.0
    assert float(m.head.weight.detach()[0, 0]) == 1.0  # the best weights are loaded back
    log = open(os.path.join(out, "training_log.txt")).read().split("\n")
    assert log[0] == DUAL_HEADER and log[1] == "-" * 59 and len(log) == 2 + 12 + 1 + 1
    assert log[2] == "    1    1.000000    3.000000     25.00%    3.000000 *"
    assert log[3] == "    2    0.500000    2.000000     25.00%    2.000000 *"
    assert log[4] == "    3    0.333333    2.500000     25.00%    2.000000"
    assert log[14] == "Early stopping at epoch 12" and log[15] == ""
    assert capsys.readouterr().out.split("\n")[:2] == [DUAL_HEADER, "-" * 59]


def test_precompute_argument_rules(capsys):
    from graphcast_lite_amd.regional_train import build_parser, resolve_dual_args

    cfg = types.SimpleNamespace(max_ar_steps=3, data=types.SimpleNamespace(pred_window_used=1))
    base = ["dual", "exp", "--pretrained", "g.pth", "--roi", "50", "60", "85", "100"]
    p = build_parser()
    a = p.parse_args(base)
    assert (a.lr, a.reg_mesh_level, a.reg_steps, a.cross_k, a.hidden_dim, a.reg_buffer, a.subsample) == \
        (5e-4, 7, 4, 3, 256, 2.0, 1) and a.roi == [50.0, 60.0, 85.0, 100.0]
    assert resolve_dual_args(a, cfg) == (3, 3, True)  # the horizon defaults to the configuration's, shuffled
    assert resolve_dual_args(p.parse_args(base + ["--ar-steps", "2"]), cfg) == (2, 2, True)
    assert capsys.readouterr().out == ""
    # --precompute: one step whatever was asked for, a warning, and no shuffling (the cache is walked in order)
    assert resolve_dual_args(p.parse_args(base + ["--precompute"]), cfg) == (3, 1, False)
    assert capsys.readouterr().out == "WARNING: --precompute requires --ar-steps 1, got 3. Forcing ar_steps=1.\n"
    assert resolve_dual_args(p.parse_args(base + ["--precompute", "--ar-steps", "1"]), cfg) == (1, 1, False)
    assert capsys.readouterr().out == ""
    r = p.parse_args(["roi", "exp", "--pretrained", "g.pth", "--roi", "1", "2", "3", "4"])
    assert (r.lr, r.hidden_dim, r.processor_steps, r.roi_k, r.batch_size) == (1e-3, 256, 6, 8, 1)
    with pytest.raises(SystemExit):
        p.parse_args(["dual", "exp", "--roi", "1", "2", "3", "4"])  # --pretrained is required
    q = p.parse_args(["predict", "exp", "--pretrained", "g.pth", "--roi", "1", "2", "3", "4"])
    assert (q.max_samples, q.ar_steps, q.reg_mesh_level, q.reg_steps, q.cross_k, q.hidden_dim, q.no_residual, q.per_channel,
            q.regional_ckpt) == (200, 1, 7, 4, 3, 256, False, False, None)
    from graphcast_lite_amd.regional_train import main

    with pytest.raises(SystemExit, match="--resume"):  # the script parses it and never reads it
        main(base + ["--resume"])


def test_record_size_arithmetic(lib_built):
    from graphcast_lite_amd import hip

    # the dual_mesh_krsk-like shape: 19 features, 2 steps, 256-wide latents
    rec = hip.RegionRecord(n_roi=437, half_E=3 * 1203, XF=38, D=256, Dm=256, C=19, P=1)
    assert (rec.Sp, rec.Dgp, rec.Cp, rec.Yp) == (296, 256, 20, 20)
    assert rec.sizes == (437 * 296, 3609 * 256, 437 * 20, 437 * 20) and rec.offsets == (0, 129352, 1053256, 1061996)
    assert rec.floats == 1070736 and rec.nbytes == 4 * 1070736
    assert all(o % 4 == 0 for o in rec.offsets)  # every part starts on a 16-byte boundary
    # widths that need padding, two target steps
    rec = hip.RegionRecord(1, 7, 10, 11, 6, 5, 2)
    assert (rec.Sp, rec.Dgp, rec.Cp, rec.Yp) == (24, 8, 8, 12) and rec.nbytes == 4 * (24 + 56 + 8 + 12)
    L = lib_built
    assert L.gcl_region_cache_record_bytes(1, 0, 4, 0, 0, 1, 1) == 4 * (4 + 4 + 4)  # no latents, no senders
    for bad in ((0, 7, 10, 11, 6, 5, 1), (1, 7, 10, 11, 0, 5, 1), (1, 7, 0, 11, 6, 5, 1), (1, 7, 10, 11, 6, 5, 0),
                (1, -1, 10, 11, 6, 5, 1), (1, 7, 1 << 24, 11, 6, 5, 1)):
        assert L.gcl_region_cache_record_bytes(*bad) == 0, bad
    with pytest.raises(ValueError):
        hip.RegionRecord(*bad).nbytes
    assert L.gcl_region_eval_pair_ws_bytes(2, 3, 257, 5) == 2 * 2 * 8  # 3855 elements: two chunks of 2048
    assert L.gcl_region_eval_pair_ws_bytes(1, 1, 1, 5) == 8 and L.gcl_region_eval_pair_ws_bytes(3, 1, 1, 5) == 0


def test_argument_validation_returns_before_any_hip_call(lib_built):
    """Every refusal is -1 with a message; none of these calls reaches a launch (there is no GPU here)."""
    L = lib_built
    buf = torch.zeros(4096)
    idx = torch.zeros(64, dtype=torch.int32)
    s64 = torch.zeros(4, dtype=torch.int64)
    f, i, s = buf.data_ptr(), idx.data_ptr(), s64.data_ptr()
    shape = (3, 7, 10, 11, 6, 5, 1)  # n_roi, half_E, XF, D, Dm, C, P

    def store(pred=f, ldp=5, ldx=10, cache=f, n_slots=2, shape=shape, B=1):
        return L.gcl_region_cache_store(pred, ldp, 0, f, 11, 0, f, 6, 0, f, ldx, 0, f, 5, 0, i, i, s, cache, n_slots, B, 20, 9,
                                        *shape, None)

    for kw, msg in ((dict(pred=None), b"null argument"), (dict(ldp=4), b"row stride"), (dict(ldx=9), b"row stride"),
                    (dict(cache=f + 4), b"16-byte aligned"), (dict(n_slots=0), b"bad shape"), (dict(B=0), b"bad shape"),
                    (dict(shape=(3, 7, 10, 11, 0, 5, 1)), b"bad record shape")):
        assert store(**kw) == -1 and msg in L.gcl_last_error(), (kw, L.gcl_last_error())

    def fetch(cache=f, slots=s, roi3=f, bs=3 * 24, B=2, n_slots=2):
        return L.gcl_region_cache_fetch(cache, n_slots, slots, B, *shape, roi3, bs, None, 0, None, 0, None, 0, None)

    for kw, msg in ((dict(cache=None), b"bad argument"), (dict(slots=None), b"bad argument"), (dict(roi3=None), b"no destination"),
                    (dict(bs=3 * 24 - 4), b"sample stride"), (dict(bs=3 * 24 + 2), b"sample stride"),
                    (dict(roi3=f + 8), b"16-byte aligned"), (dict(n_slots=0), b"bad argument")):
        assert fetch(**kw) == -1 and msg in L.gcl_last_error(), (kw, L.gcl_last_error())

    acc = torch.zeros(2, dtype=torch.float64).data_ptr()

    def pair(nq=1, delta=f, ldd=5, ldw=10, new_win=None, win=f, n=20, rows=i, ws=f, ws_bytes=4096, obs=2, ldo=0, out=None):
        return L.gcl_region_eval_pair(nq, delta, ldd, 0, win, ldw, 0, new_win, out, ldo, 0, None, 0, 0, None, 0, 0, None, None,
                                      0, 0, f, 5, 0, None, 1, rows, n, C.c_double(1.0), acc, 1, 20, obs, 5, ws, ws_bytes, None)

    for kw, msg in ((dict(nq=3), b"one or two predictions"), (dict(nq=2), b"null argument"), (dict(delta=None), b"null argument"),
                    (dict(ldd=4), b"row stride"), (dict(ldw=9), b"row stride"), (dict(new_win=f), b"in place"),
                    (dict(rows=None, n=21), b"identity rows"), (dict(ws_bytes=4), b"workspace"), (dict(obs=0), b"bad shape"),
                    (dict(out=f, ldo=4), b"output row stride"), (dict(out=f, ldo=5), b"may not be the delta")):
        assert pair(**kw) == -1 and msg in L.gcl_last_error(), (kw, L.gcl_last_error())
