"""`graphcast_lite_amd.regional_train` on the GPU: the device cache against `precompute_global` (bit-equal), the cached
step against `DualMeshCachedStep` fed the same records (bit-equal at B = 1, captured and eager), and the epoch functions
against the reference's loops restated in plain torch over the same HIP model (`scripts/train_dual_mesh.py:138-368`,
`scripts/train_roi_residual.py:91-192`).

Tolerance of the restated loops: 1e-4 relative, the bar tests/test_dual_mesh.py applies to these same steps (float32
losses summed by torch against float64 sums on the device; the observed differences are printed)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from test_dual_mesh import DEV, ROI, _pair, _regular

pytestmark = pytest.mark.gpu
KEYS = ("global_pred_roi", "roi_grid_latent", "cross_sender_feat")


def _samples(cfg, G, n, P=1, seed=40):
    g = torch.Generator().manual_seed(seed)
    Fe, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    return [(torch.randn(1, G, obs * Fe, generator=g), torch.randn(1, G, P * Fe, generator=g)) for _ in range(n)]


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def test_cache_records_equal_precompute_global():
    from graphcast_lite_amd.regional_train import GlobalOutputCache

    cfg, r, _ = _pair("baseline")
    G, C = r.global_model._num_grid_nodes, cfg.data.num_features_used
    data = _samples(cfg, G, 3, P=2)
    cache = GlobalOutputCache(r, 6, pred_steps=2)
    assert cache.nbytes == 6 * cache.rec.nbytes and len(cache) == 0
    for X, y in data:  # one sample per call: like for like with precompute_global on that sample
        cache.add(X, y)
    Xb, yb = torch.cat([d[0] for d in data]), torch.cat([d[1] for d in data])
    slots = cache.add(Xb, yb)  # and the three of them as one batch
    assert slots.tolist() == [3, 4, 5] and len(cache) == 6
    mask = r.roi_mask.cpu()
    batched = r.precompute_global(Xb.to(DEV))
    for i, (X, y) in enumerate(data):
        want = r.precompute_global(X.to(DEV))
        raw, got, y_roi = cache.sample(i)
        assert sorted(got) == sorted(want) == sorted(KEYS)
        for k in KEYS:
            assert got[k].device.type == "cpu" and got[k].shape == want[k].shape
            assert torch.equal(got[k], want[k]), (i, k)
            assert torch.equal(cache.as_reference(3 + i)[k], batched[k][i]), (i, k)
        assert torch.equal(raw, X[0][mask]) and torch.equal(y_roi, y[0][mask])
    with pytest.raises(ValueError):
        cache.add(*data[0])  # full
    # the record is what forward_cached builds: roi_input with zero pad columns
    roi3 = cache.fetch(torch.tensor([1], device=DEV))[0]
    S = r.reg_enc_input_dim
    assert roi3.shape[2] == (S + 3) // 4 * 4 and bool((roi3[..., S:] == 0).all())
    assert torch.equal(roi3[0, :, :S].cpu(), torch.cat([data[1][0][0][mask], cache.as_reference(1)["roi_grid_latent"]], 1))
    assert C == cache.rec.C


@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("use_residual", [False, True])
def test_cache_step_leaves_the_bits_of_the_cached_step(use_residual, graph):
    from graphcast_lite_amd.dual_mesh import DualMeshCachedStep
    from graphcast_lite_amd.regional_train import DualMeshCacheStep, GlobalOutputCache

    cfg, r1, _ = _pair("baseline", seed=6)
    _, r2, _ = _pair("baseline", seed=6)
    G = r1.global_model._num_grid_nodes
    cache = GlobalOutputCache(r1, 2)
    for X, y in _samples(cfg, G, 2, seed=11):
        cache.add(X, y)
    fed = [cache.sample(i) for i in range(2)]
    gsnap = {"global_model." + n: p.detach().clone() for n, p in r1.global_model.named_parameters()}
    s1 = DualMeshCacheStep(r1, cache, lr=1e-3, use_residual=use_residual, use_graph=graph)
    s2 = DualMeshCachedStep(r2, lr=1e-3, use_residual=use_residual, use_graph=False)
    slots = torch.arange(2, device=DEV)
    for i in range(5):
        l1 = s1(slots[i % 2:i % 2 + 1]).clone()
        raw, c, y = fed[i % 2]
        l2 = s2(raw, *(c[k] for k in KEYS), y)
        assert torch.equal(l1, l2), (i, l1.item(), l2.item())
    assert s1.graph_active == graph and not s2.graph_active
    p2 = dict(r2.named_parameters())
    n_reg = 0
    for n, p in r1.named_parameters():
        if n.startswith("global_model."):
            assert torch.equal(p.detach(), gsnap[n]) and p.grad is None, n
        else:
            assert torch.equal(p.detach(), p2[n].detach()), n
            n_reg += 1
    assert n_reg > 10


def test_cache_step_takes_batches():
    """B > 1 (the reference's cached mode cannot): the loss is the mean of the per-sample losses."""
    from graphcast_lite_amd.regional_train import DualMeshCacheStep, GlobalOutputCache

    cfg, r, _ = _pair("baseline", seed=6)
    G, C = r.global_model._num_grid_nodes, cfg.data.num_features_used
    cache = GlobalOutputCache(r, 3)
    for X, y in _samples(cfg, G, 3, seed=21):
        cache.add(X, y)
    per = []
    with torch.no_grad():
        for i in range(3):
            raw, c, y = cache.sample(i)
            out = r.forward_cached(raw.to(DEV), *(c[k].to(DEV) for k in KEYS))
            per.append(((out.cpu().double() - y.double()) ** 2).mean().item())
    s = DualMeshCacheStep(r, cache, lr=1e-3, use_graph=False)
    loss = s(torch.tensor([2, 0, 1], device=DEV)).item()
    assert _rel(loss, sum(per) / 3) <= 1e-5, (loss, per)


# ------------------------------------------------------------------------------------------------------------------
# the reference's loops in plain torch over the HIP model
# ------------------------------------------------------------------------------------------------------------------
def _mse(a, b):
    return ((a - b) ** 2).mean()


def _ref_eval_dual(model, batches, use_residual, ar_steps, static_channels, forcing_channels):
    """scripts/train_dual_mesh.py:310-368 (standard mode)."""
    from graphcast_lite_amd.regional_train import apply_special_channels

    mask = model.roi_mask
    total = total_g = 0.0
    with torch.no_grad():
        for X, y in batches:
            X, y = X.to(DEV), y.to(DEV)
            N, G, F = X.shape
            obs = model.obs_window
            C = F // obs
            P = y.shape[-1] // C
            y_steps = y.view(N, G, P, C)
            cs, gs = X.view(N, G, obs, C), X.view(N, G, obs, C).clone()
            steps = min(ar_steps, P)
            loss = gloss = 0.0
            for s in range(steps):
                target = y_steps[:, :, s, :]
                pred = model(cs.reshape(N, G, -1))
                pred = pred.unsqueeze(0) if pred.dim() == 2 else pred
                co = cs[:, :, -1, :] + pred if use_residual else pred.clone()
                co = apply_special_channels(co, cs, target, static_channels, forcing_channels)
                gp = model.global_model(X=gs.reshape(N, G, -1), attention_threshold=0.0)
                gp = gp.unsqueeze(0) if gp.dim() == 2 else gp
                go = gs[:, :, -1, :] + gp if use_residual else gp.clone()
                go = apply_special_channels(go, gs, target, static_channels, forcing_channels)
                loss = loss + _mse(co[:, mask], target[:, mask])
                gloss = gloss + _mse(go[:, mask], target[:, mask])
                cs = torch.cat([cs[:, :, 1:, :], co.unsqueeze(2)], dim=2)
                gs = torch.cat([gs[:, :, 1:, :], go.unsqueeze(2)], dim=2)
            total += (loss / max(steps, 1)).item()
            total_g += (gloss / max(steps, 1)).item()
    n = max(len(batches), 1)
    return total / n, 1.0 - (total / n) / (total_g / n)


@pytest.mark.parametrize("use_residual,ar_steps,special", [(False, 1, False), (True, 2, False), (True, 2, True)])
def test_eval_dual_matches_the_restated_loop(use_residual, ar_steps, special):
    from graphcast_lite_amd.regional_train import GlobalOutputCache, eval_dual

    cfg, r, _ = _pair("baseline", seed=9)
    G = r.global_model._num_grid_nodes
    batches = _samples(cfg, G, 2, P=2, seed=50) + [tuple(torch.cat(t) for t in zip(*_samples(cfg, G, 2, P=2, seed=51)))]
    st, fo = ([1], [3]) if special else (None, None)
    want = _ref_eval_dual(r, batches, use_residual, ar_steps, st, fo)
    got = eval_dual(r, batches, DEV, use_residual=use_residual, current_ar_steps=ar_steps, static_channels=st,
                    forcing_channels=fo)
    print(f"eval_dual residual={use_residual} ar={ar_steps} special={special}: {got} restated {want}")
    assert _rel(got[0], want[0]) <= 1e-4 and abs(got[1] - want[1]) <= 1e-4, (got, want)
    if ar_steps == 1:  # the cached mode scores the same thing from the records
        cache = GlobalOutputCache.build(r, batches, "val", log=lambda m: None)
        assert len(cache) == 4
        got_c = eval_dual(r, None, DEV, use_residual=use_residual, cache=cache)
        want_c = _ref_eval_dual(r, [(X[b:b + 1], y[b:b + 1]) for X, y in batches for b in range(X.shape[0])],
                                use_residual, 1, None, None)
        assert _rel(got_c[0], want_c[0]) <= 1e-4 and abs(got_c[1] - want_c[1]) <= 1e-4, (got_c, want_c)


def test_train_dual_epoch_runs_the_fused_steps():
    """Both modes against the same steps driven by hand on a twin model; the gradient report; two epochs."""
    from graphcast_lite_amd.dual_mesh import DualMeshCachedStep
    from graphcast_lite_amd.regional_train import DualMeshCacheStep, GlobalOutputCache, train_dual_epoch
    from graphcast_lite_amd.train import TrainStep

    cfg, r1, _ = _pair("baseline", seed=6)
    _, r2, _ = _pair("baseline", seed=6)
    G = r1.global_model._num_grid_nodes
    data = _samples(cfg, G, 3, seed=60)
    # cached mode
    cache = GlobalOutputCache.build(r1, data, log=lambda m: None)
    s1 = DualMeshCacheStep(r1, cache, lr=1e-3, use_residual=True)
    s2 = DualMeshCachedStep(r2, lr=1e-3, use_residual=True, use_graph=False)
    said = []
    for epoch in range(2):
        got = train_dual_epoch(r1, None, s1, DEV, use_residual=True, check_grads=(epoch == 0), cache=cache, say=said.append)
        want = 0.0
        for i in range(3):
            raw, c, y = cache.sample(i)
            want += s2(raw, *(c[k] for k in KEYS), y).item()
        assert abs(got - want / 3) <= 1e-9 * abs(want), (epoch, got, want / 3)
    assert s1.graph_active
    assert said[0] == "[GradCheck] out_roi.requires_grad: True"
    mods = [m.group(1) for m in (re.match(r"  \[(\w+)\] \d+ params, max_grad=\d+\.\d{6}, mean_grad=\d+\.\d{6}$", s)
                                 for s in said) if m]
    assert mods == ["cross_edge_encoder", "cross_message", "reg_decoder", "reg_encoder", "reg_processor"]
    assert sum(s.startswith("    top: ") for s in said) == 5
    with pytest.raises(ValueError):
        train_dual_epoch(r1, None, s1, DEV, use_residual=False, cache=cache)
    # standard mode, two AR steps
    cfg, r3, _ = _pair("baseline", seed=8)
    _, r4, _ = _pair("baseline", seed=8)
    data2 = _samples(cfg, G, 3, P=2, seed=61)
    mask3 = r3.roi_mask.view(1, -1, 1).float()
    t3 = TrainStep(r3, lr=1e-3, spatial_mask=mask3, use_residual=True, ar_steps=1, use_graph=False)
    t4 = TrainStep(r4, lr=1e-3, spatial_mask=mask3, use_residual=True, ar_steps=2, use_graph=False)
    got = train_dual_epoch(r3, data2, t3, DEV, use_residual=True, current_ar_steps=2, say=said.append)
    want = sum(t4(X.to(DEV), y.to(DEV)).item() for X, y in data2) / 3
    assert t3.ar_steps == 2 and abs(got - want) <= 1e-9 * abs(want), (got, want)
    # static / forcing channels: the script scores after the overwrite, which a plain TrainStep does not
    t5 = TrainStep(r3, lr=1e-3, spatial_mask=mask3, use_residual=True, ar_steps=2, use_graph=False, static_channels=[1],
                   forcing_channels=[3])
    with pytest.raises(ValueError, match="DualTrainStep"):
        train_dual_epoch(r3, data2, t5, DEV, use_residual=True, current_ar_steps=2, static_channels=[1], forcing_channels=[3])


def _roi_model(seed=3):
    from graphcast_lite_amd.roi_residual import ROIResidualModel
    from test_hip_model import make_pair

    cfg, m, _ = make_pair("baseline", [1, 2], seed=seed)
    lats, lons = _regular(32, 64)
    torch.manual_seed(seed + 1)
    r = ROIResidualModel(m, ROI, lats, lons, torch.device(DEV), hidden_dim=32, processor_steps=2, roi_k=4)
    with torch.no_grad():
        r.decoder.mlp[-1].weight.copy_(0.2 * torch.randn(r.decoder.mlp[-1].weight.shape))
    return cfg, r


def test_roi_epochs_match_the_restated_loops():
    from graphcast_lite_amd.regional_train import eval_roi_epoch, train_roi_epoch
    from graphcast_lite_amd.train import TrainStep, spatial_corr

    cfg, r = _roi_model()
    G = r.global_model._num_grid_nodes
    C = cfg.data.num_features_used
    batches = _samples(cfg, G, 2, P=2, seed=70) + [tuple(torch.cat(t) for t in zip(*_samples(cfg, G, 2, P=2, seed=71)))]
    mask = r.roi_mask
    loss = acc = 0.0
    with torch.no_grad():
        for X, y in batches:
            pred = r(X.to(DEV))
            pred = pred.unsqueeze(0) if pred.dim() == 2 else pred
            o_roi, y_roi = pred[:, mask, :], y.to(DEV)[:, :, :C][:, mask, :]
            loss += _mse(o_roi, y_roi).item()
            acc += spatial_corr(o_roi, y_roi)
    want = (loss / 3, acc / 3)
    got = eval_roi_epoch(r, batches, DEV)
    print(f"eval_roi_epoch: {got} restated {want}")
    assert _rel(got[0], want[0]) <= 1e-4 and abs(got[1] - want[1]) <= 1e-4, (got, want)
    # training: the mean of the fused steps' losses and the [Correction] line of the last batch
    step = TrainStep(r, lr=1e-3, spatial_mask=mask.view(1, -1, 1).float(), use_residual=False, use_graph=False)
    with torch.no_grad():
        X, y = batches[-1]
        pred, glob = r(X.to(DEV)), r.global_model(X=X.to(DEV), attention_threshold=0.0)
        corr = (pred[:, mask] - glob[:, mask]).abs()
        base = _mse(glob[:, mask], y.to(DEV)[:, :, :C][:, mask]).item()
    said = []
    first = train_roi_epoch(r, batches[-1:], step, DEV, check_grads=True, say=said.append)
    assert said[0] == "[GradCheck] out.requires_grad: True"
    m = re.match(r"  \[Correction\] mean_abs=(\d+\.\d{6}), max_abs=(\d+\.\d{4}), baseline_mse=(\d+\.\d{6})$", said[-1])
    assert m, said[-1]
    for g, w, tol in zip(m.groups(), (corr.mean().item(), corr.max().item(), base), (2e-6, 2e-4, 2e-6)):
        assert abs(float(g) - w) <= tol + 1e-4 * abs(w), (said[-1], w)
    second = train_roi_epoch(r, batches[-1:], step, DEV, say=said.append)
    assert second < first  # the step trains


def test_overfit_test_reports_and_restores():
    from graphcast_lite_amd.regional_train import overfit_test

    cfg, r, _ = _pair("baseline", seed=4)
    G = r.global_model._num_grid_nodes
    before = {k: v.clone() for k, v in r.state_dict().items()}
    said = []
    overfit_test(r, _samples(cfg, G, 1, seed=80), DEV, use_residual=True, n_steps=22, lr=0.01, say=said.append)
    lines = [s for s in said if s.startswith("    step")]
    assert len(lines) == 3 and all(re.match(r"    step +\d+: loss=\d+\.\d{6}  \|correction\|=\d+\.\d{6}  max=\d+\.\d{4}$", s)
                                   for s in lines), lines
    assert said[1] == "[OverfitTest] 1 sample, 22 steps, lr=0.01..."
    assert said[-2] == "[OverfitTest] DONE. Model weights RESTORED to initial state."
    loss = [float(re.search(r"loss=(\S+)", s).group(1)) for s in lines]
    assert loss[-1] < loss[0]
    for k, v in r.state_dict().items():
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("precompute", [True, False])
def test_fit_dual_mesh_writes_the_reference_files(precompute, tmp_path, capsys):
    from graphcast_lite_amd.regional_train import fit_dual_mesh

    cfg, r, _ = _pair("baseline", seed=5)
    G = r.global_model._num_grid_nodes
    P = 2
    tr, va, te = (_samples(cfg, G, n, P=P, seed=s) for n, s in ((3, 90), (2, 91), (2, 92)))
    out = str(tmp_path / "results")
    res = fit_dual_mesh(r, tr, va, te, out, num_epochs=2, lr=5e-4, ar_steps=2, use_residual=True, precompute=precompute,
                        overfit=False, reg_mesh_level=7)
    assert sorted(os.listdir(out)) == ["best_model.pth", "best_regional.pth", "results.json", "training_log.txt"]
    assert list(res) == ["best_val_loss", "test_loss", "test_correction_skill", "roi", "reg_mesh_level", "reg_steps",
                         "cross_k", "hidden_dim", "ar_steps"]
    assert json.load(open(os.path.join(out, "results.json"))) == res
    assert res["ar_steps"] == (1 if precompute else 2) and res["cross_k"] == 3 and res["hidden_dim"] == 32
    assert res["reg_steps"] == 2 and res["roi"] == list(ROI)
    reg = torch.load(os.path.join(out, "best_regional.pth"), weights_only=True)
    full = torch.load(os.path.join(out, "best_model.pth"), weights_only=True)
    assert reg and not any(k.startswith("global_model.") for k in reg)
    assert sorted(reg) == sorted(k for k in full if not k.startswith("global_model."))
    assert any(k.startswith("global_model.") for k in full)
    log = open(os.path.join(out, "training_log.txt")).read().split("\n")
    assert log[0] == f"[AR] training/eval horizon = {res['ar_steps']} step(s) (+{res['ar_steps'] * 6}h)"
    assert log[1] == "epoch  train_loss    val_loss  corr_skill        best" and log[2] == "-" * 59
    assert re.match(r"    1 {2}[ \d]+\.\d{6} {2}[ \d]+\.\d{6} {2}[ \-\d]+\.\d\d% {2}[ \d]+\.\d{6} \*$", log[3]), log[3]
    assert re.match(r"^\[TEST\] loss=\d+\.\d{6}  correction_skill=-?\d+\.\d\d%$", log[6]), log[5:]
    assert log[5] == "" and log[7] == f"Results saved to {out}"
    printed = capsys.readouterr().out
    assert ("[Precompute] Caching global model outputs..." in printed) == precompute
    if precompute:
        assert "WARNING: --precompute requires --ar-steps 1, got 2. Forcing ar_steps=1." in printed
        assert re.search(r"  train: 3 samples cached in \d+s \(\d+ MB\)", printed)
    assert np.isfinite(res["test_loss"]) and res["best_val_loss"] < float("inf")


def test_fit_roi_residual_writes_the_reference_files(tmp_path):
    from graphcast_lite_amd.regional_train import fit_roi_residual

    cfg, r = _roi_model(seed=5)
    G = r.global_model._num_grid_nodes
    tr, va, te = (_samples(cfg, G, n, seed=s) for n, s in ((3, 95), (2, 96), (2, 97)))
    out = str(tmp_path / "results")
    res = fit_roi_residual(r, tr, va, te, out, num_epochs=2, lr=1e-3, overfit=False,
                           extra={"pretrained": "g.pth", "data_dir": "d"})
    assert sorted(os.listdir(out)) == ["best_head.pth", "best_model.pth", "results.json", "training_log.txt"]
    assert list(res) == ["best_val_loss", "test_loss", "test_regional_acc", "roi", "hidden_dim", "processor_steps", "roi_k",
                         "lr", "pretrained", "data_dir"]
    assert json.load(open(os.path.join(out, "results.json"))) == res
    assert (res["hidden_dim"], res["processor_steps"], res["roi_k"], res["pretrained"]) == (32, 2, 4, "g.pth")
    head = torch.load(os.path.join(out, "best_head.pth"), weights_only=True)
    assert head and not any(k.startswith("global_model.") for k in head)
    log = open(os.path.join(out, "training_log.txt")).read().split("\n")
    assert log[0] == "epoch  train_loss    val_loss   val_ACC        best" and log[1] == "-" * 55
    assert re.match(r"    1 {2}[ \d]+\.\d{6} {2}[ \d]+\.\d{6} {2}[ \-\d]+\.\d{4} {2}[ \d]+\.\d{6} \*$", log[2]), log[2]
    assert log[4] == "" and re.match(r"^\[TEST\] loss=\d+\.\d{6}  regional_ACC=-?\d+\.\d{4}$", log[5]), log[4:]
    assert log[6] == f"Results saved to {out}"
