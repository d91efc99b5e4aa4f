"""The downscaler's objective, scores and loop end to end on the GPU (graphcast_lite_amd.downscale) against the
reference's own runs (tests/golden/downscale_loss_vectors.npz, made by tests/golden/make_downscale_loss_golden.py).

Rules:
  losses       masked_mse_loss, spectral_loss, gradient_loss and downscaler_loss give the same terms (the same kernels:
               bit-equal), each within 4 * max(E(ref32), 2^-24) of the fixture's float64 value, E(x) = max |x - x64| /
               max |x64|; backward through (2.5 * loss) gives exactly 2.5 times the gradient of loss.backward().
  training     on the archives of tests/helpers/downscale_case.py (obs 2, batches of 3 in order, the stub network of
               tests/helpers/downscaler_stub.py, SGD lr 1e-2, two epochs): the per-batch loss sequence, the validation
               loss, the two RMSE columns and the skill each satisfy E(ours) <= 4 * max(E(ref32), 2^-24) against the
               reference's float64 run, E(ref32) the error of its own float32 run.
  fit          fit_downscaler writes best_model.pth, training_log.txt and results.json, stops early once the validation
               loss stops improving (lr 0 after epoch 1) and reloads the best weights before the test table.
  batches      iter_batches with the same generator seed yields the same batches twice; with shuffle every index
               appears exactly once per epoch; drop_last drops the remainder.
"""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import downscale_case as DC  # noqa: E402
import downscale_loss_case as LC  # noqa: E402
from downscaler_stub import ChannelMix  # noqa: E402

gpu = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def D(lib_built):
    from graphcast_lite_amd import downscale

    return downscale


@pytest.fixture(scope="module")
def gv():
    return LC.golden()


@pytest.fixture(scope="module")
def pairs(D):
    g = DC.golden()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    scalers = {"mean": g["sc_mean"], "std": g["sc_std"], "n": g["sc_n"]}
    return D.DownscalerPairs(up(g["coarse"]), up(g["fine"]), up(g["static_fine"]), scalers, g["lat32"].astype(np.float64),
                             g["lon32"].astype(np.float64), DC.info_of(g), json.loads(str(g["variables"])))


def dataset(D, pairs, split, **kw):
    return D.DownscalerDataset(pairs, obs_window=LC.TRAIN_OBS, split=split, device=DEV, **kw)


def static_mask():
    m = torch.ones(DC.C)
    m[DC.STATIC] = 0.0
    return m.to(DEV)


def within(ours, key, gv):
    """E(ours) <= 4 * max(E(ref32), 2^-24) against the float64 run; prints the figures."""
    x64, x32 = gv[key + "64"], gv[key + "32"]
    e, bound = LC.E(ours, x64), 4.0 * max(LC.E(x32, x64), EPS)
    print(f"{key}: E(ours) = {e:.3e}, E(ref32) = {LC.E(x32, x64):.3e}, bound {bound:.3e}")
    return e <= bound


# ---- the losses ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", [(1, 1, 1), (3, 0, 0), (2, 1, 0)], ids=lambda c: LC.case_key(*c))
def test_named_losses_and_downscaler_loss_agree(D, gv, case):
    si, r, m = case
    out, Y, x_last = (t.to(torch.float32).to(DEV) for t in LC.inputs(LC.SHAPES[si]))
    B, C, Hh, W = out.shape
    X = torch.cat([torch.zeros_like(x_last), x_last, torch.ones(B, 1, Hh, W, device=DEV)], dim=1)  # obs 2, one static
    mask = LC.mask_for(C, bool(m), torch.float32)
    mask = None if mask is None else mask.to(DEV)
    key = LC.case_key(si, r, m)
    t64, tot64, E32, Eg32 = gv[f"{key}_t64"], gv[f"{key}_tot64"], gv[f"{key}_E32"], gv[f"{key}_Eg32"]
    mc = np.ones(C) if not m else LC.mask_for(C, True).numpy()
    basis = gv[f"{LC.case_key(si, r, 0)}_g64"] * mc.reshape(1, 1, C, 1, 1)
    pred = (x_last + out if r else out).clone().requires_grad_(True)
    named = [D.masked_mse_loss(pred, Y, mask), D.spectral_loss(pred, Y, mask), D.gradient_loss(pred, Y, mask)]
    for k, v in enumerate(named):
        assert v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.requires_grad
        assert LC.E(v.item(), t64[k]) <= 4.0 * max(E32[0][k], EPS), LC.TERMS[k]
        (g,) = torch.autograd.grad(v, pred)
        assert LC.E(g.cpu().numpy(), basis[k]) <= 4.0 * max(Eg32[k], EPS), f"gradient of {LC.TERMS[k]}"
    for wi, (sw, gw) in enumerate(LC.WEIGHTS):
        leaf = out.clone().requires_grad_(True)
        loss, terms = D.downscaler_loss(leaf, Y, X=X, obs_window=2, residual=bool(r), channel_mask=mask,
                                        spectral_weight=sw, gradient_weight=gw, return_terms=True)
        assert loss.dim() == 0 and loss.dtype == torch.float32
        assert LC.E(loss.item(), tot64[wi]) <= 4.0 * max(E32[wi][3], EPS)
        assert terms[0].float().item() == named[0].item()
        assert terms[1].float().item() == (named[1].item() if sw > 0 else 0.0)
        assert terms[2].float().item() == (named[2].item() if gw > 0 else 0.0)
        loss.backward()
        g1 = leaf.grad.clone()
        assert LC.E(g1.cpu().numpy(), basis[0] + sw * basis[1] + gw * basis[2]) <= 4.0 * max(E32[wi][4], EPS)
        leaf.grad = None
        loss2 = D.downscaler_loss(leaf, Y, X=X, obs_window=2, residual=bool(r), channel_mask=mask, spectral_weight=sw,
                                  gradient_weight=gw)
        (2.5 * loss2).backward()
        assert torch.equal(leaf.grad, g1 * 2.5)
    with torch.no_grad():
        assert not D.downscaler_loss(out, Y, channel_mask=mask).requires_grad


# ---- train_epoch, validate, compute_metrics against the reference's runs ------------------------------------------------
@gpu
def test_training_case_within_the_reference_float32_error(D, gv, pairs):
    train, val, every = (dataset(D, pairs, s) for s in ("train", "val", "all"))
    assert (len(train), len(val), len(every)) == (9, 1, 11)
    model = ChannelMix(LC.TRAIN_OBS * DC.C + len(DC.STATIC), DC.C).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=LC.TRAIN_LR)
    mask, losses, means = static_mask(), [], []
    for _ in range(LC.TRAIN_EPOCHS):
        means.append(D.train_epoch(model, D.iter_batches(train, LC.TRAIN_BATCH), opt, mask, LC.TRAIN_RESIDUAL,
                                   LC.TRAIN_SW, LC.TRAIN_GW, obs_window=LC.TRAIN_OBS, per_batch=losses))
    ours = np.array([v.item() for v in losses], dtype=np.float64)
    assert len(ours) == 6 and np.allclose(means, ours.reshape(2, 3).mean(axis=1), rtol=1e-12)
    ok = [within(ours, "train_losses", gv)]
    v = D.validate(model, D.iter_batches(val, LC.TRAIN_BATCH), mask, LC.TRAIN_RESIDUAL, DC.C, LC.TRAIN_OBS)
    ok.append(within(v, "train_val", gv))
    rm, rc, sk = D.compute_metrics(model, D.iter_batches(every, LC.TRAIN_BATCH), mask, LC.TRAIN_RESIDUAL, DC.C,
                                   every.std_np, obs_window=LC.TRAIN_OBS)
    assert rm.dtype == rc.dtype == sk.dtype == np.float64 and rm.shape == (DC.C,)
    ok += [within(rm, "train_rmse_model", gv), within(rc, "train_rmse_coarse", gv), within(sk, "train_skill", gv)]
    assert all(ok), ok


# ---- fit_downscaler --------------------------------------------------------------------------------------------------
@gpu
def test_fit_downscaler_stops_early_and_reloads_the_best_weights(D, gv, pairs, tmp_path):
    train, val, test = (dataset(D, pairs, s) for s in ("train", "val", "test"))
    model = ChannelMix(LC.TRAIN_OBS * DC.C + len(DC.STATIC), DC.C).to(DEV)
    opt = torch.optim.SGD(model.parameters(), lr=LC.TRAIN_LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 if e < 1 else 0.0)  # lr 0 after epoch 1
    loaded, orig = [], model.load_state_dict

    def spy(sd, *a, **kw):
        loaded.append({k: t.clone() for k, t in sd.items()})
        return orig(sd, *a, **kw)

    model.load_state_dict = spy
    exp = str(tmp_path / "exp")
    res = D.fit_downscaler(model, opt, sched, train, val, test, exp, num_epochs=3, patience=1, batch_size=LC.TRAIN_BATCH,
                           residual=True, spectral_weight=0.1, gradient_weight=0.05,
                           generator=torch.Generator().manual_seed(3), data_dir="pairs", log=None)
    assert sorted(os.listdir(exp)) == ["best_model.pth", "results.json", "training_log.txt"]
    log = open(os.path.join(exp, "training_log.txt")).read().split("\n")
    ref = str(gv["main_log"]).split("\n")
    assert re.fullmatch(r"=== Downscaler training started: \S+ ===", log[0]) and log[1] == "data_dir=pairs  epochs=3  batch=3  lr=0.01"
    assert log[2] == ref[2] and log[3] == ref[3] and log[4] == ref[4]  # the switches, the column header, the rule
    row = r" +\d+  +\d+\.\d{6}  +\d+\.\d{6}  +\d+\.\d{6}  \d\.\de[-+]\d\d( \*)?  \(\d+s\)"
    assert all(re.fullmatch(row, ref[i]) for i in (5, 6)), "the pattern misses the reference's own rows"
    assert re.fullmatch(row, log[5]) and log[5].split("  (")[0].endswith(" *")
    assert re.fullmatch(row, log[6]) and " *" not in log[6]
    assert log[7] == "Early stopping at epoch 2"
    assert log[8:12] == ref[7:11] and log[12].startswith("[TEST] loss=")
    best = torch.load(os.path.join(exp, "best_model.pth"), map_location=DEV)
    assert len(loaded) == 1 and all(torch.equal(loaded[0][k], best[k]) for k in best)
    assert all(torch.equal(model.state_dict()[k], best[k]) for k in best)
    on_disk = json.load(open(os.path.join(exp, "results.json")))
    assert on_disk == res and list(res) == list(json.loads(str(gv["main_results_json"])))
    names = json.loads(str(DC.golden()["variables"]))
    assert list(res["per_channel_rmse"]) == names
    assert list(res["per_channel_skill"]) == [n for i, n in enumerate(names) if i not in DC.STATIC]
    mask = static_mask()
    assert res["test_loss"] == D.validate(model, D.iter_batches(test, LC.TRAIN_BATCH), mask, True, DC.C, LC.TRAIN_OBS)
    table = re.search(r"\[TEST\] loss=[^\n]*\n(.*)\n\nResults saved", "\n".join(log), flags=re.S).group(1)
    metrics = D.DownscalerMetrics(DC.C, train.std_np, DC.STATIC)
    with torch.no_grad():
        for X, Y in D.iter_batches(test, LC.TRAIN_BATCH):
            metrics.update(model(X), X, Y, True, LC.TRAIN_OBS)
    assert table == "\n".join(metrics.table(names))


# ---- iter_batches ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("gen_device", ["cpu", DEV])
def test_iter_batches_is_repeatable_and_complete(D, pairs, gen_device):
    ds = dataset(D, pairs, "train", augment_flip=True, input_noise=0.05, wind_u_channels=DC.U_CHANNELS)
    runs = []
    for _ in range(2):
        g = torch.Generator(device=gen_device).manual_seed(11)
        runs.append([(X.clone(), Y.clone()) for X, Y in D.iter_batches(ds, 4, shuffle=True, generator=g)])
    assert [len(b[0]) for b in runs[0]] == [4, 4, 1]
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(*runs))
    other = [Y for _, Y in D.iter_batches(ds, 4, shuffle=True, generator=torch.Generator(device=gen_device).manual_seed(12))]
    assert not all(torch.equal(a[1], b) for a, b in zip(runs[0], other))

    seen, orig = [], ds.batch

    def spy(idx, **kw):
        seen.append(list(idx))
        return orig(idx, **kw)

    ds.batch = spy
    g = torch.Generator(device=gen_device).manual_seed(11)
    for _ in range(2):  # two epochs from one generator: each a permutation, and not the same one
        list(D.iter_batches(ds, 4, shuffle=True, generator=g))
    flat = [i for b in seen for i in b]
    assert sorted(flat[:9]) == sorted(flat[9:]) == list(range(9)) and flat[:9] != flat[9:]
    seen.clear()
    list(D.iter_batches(ds, 4, shuffle=True, drop_last=True, generator=g))
    assert [len(b) for b in seen] == [4, 4]
    seen.clear()
    list(D.iter_batches(ds, 4))
    assert seen == [[0, 1, 2, 3], [4, 5, 6, 7], [8]]
