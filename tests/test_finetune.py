"""Fine-tuning on the fused step (src/main.py:190-211, src/train.py:311-524): Adam parameter groups with per-parameter
step counters (`gcl_adam_step_groups`), freeze / unfreeze and AR-depth changes on a live `TrainStep`, the optimiser
state in torch's layout, and the `train()` driver against `tests/golden/finetune_vectors.npz` - a fixture produced by
running the reference's own `train()` (tests/golden/make_finetune_golden.py).  Nothing here reads the reference."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import finetune_stub as S  # noqa: E402

DEV = "cuda:0"


def _z():
    return np.load(os.path.join(GOLDEN, "finetune_vectors.npz"), allow_pickle=False)


def rel(a, b):
    """max(Frobenius relative error, max|diff| / max|ref|)"""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    fro = float((a - b).norm() / (b.norm() + 1e-30))
    mx = float((a - b).abs().max() / (b.abs().max() + 1e-30)) if b.numel() else 0.0
    return max(fro, mx)


def _stub(z, device="cpu", prefix="init"):
    m = S.FinetuneStub().to(device)
    m.load_state_dict({k: torch.tensor(z[f"{prefix}_{k}"]) for k, _ in m.named_parameters()})
    return m


def _two_groups(m, lr=1e-2, factor=0.1):
    proc = list(m.processor.parameters())
    ids = {id(p) for p in proc}
    return [{"params": [p for p in m.parameters() if id(p) not in ids], "lr": lr}, {"params": proc, "lr": lr * factor}]


def _batches(z, split, device="cpu"):
    return [(torch.tensor(x).to(device), torch.tensor(y).to(device)) for x, y in zip(z[f"X_{split}"], z[f"y_{split}"])]


def _masks(device="cpu"):
    from graphcast_lite_amd.train import get_lat_weights

    md, cfg = S.metadata(), S.config()
    lw = get_lat_weights(md.num_latitudes, md.num_longitudes, device)
    cm = torch.ones(S.C, device=device)
    cm[cfg.forcing_channels] = 0.0
    roi = torch.as_tensor(md.is_regional, dtype=torch.float32, device=device).view(1, -1, 1)
    return lw, cm, roi


def _torch_state(z, prefix):
    """The fixture's torch.optim.Adam state_dict (tensors) of `prefix` (e.g. 'a', 'c1_ckpt')."""
    state, k = {}, 0
    n = sum(len(z[f"{prefix}_opt_params{g}"]) for g in range(len(z[f"{prefix}_opt_lr"])))
    for k in range(n):
        if f"{prefix}_opt_{k}_step" in z:
            state[k] = {"step": torch.tensor(float(z[f"{prefix}_opt_{k}_step"])),
                        "exp_avg": torch.tensor(z[f"{prefix}_opt_{k}_exp_avg"]),
                        "exp_avg_sq": torch.tensor(z[f"{prefix}_opt_{k}_exp_avg_sq"])}
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()["param_groups"][0]
    groups = [dict(ref, lr=float(lr), params=[int(i) for i in z[f"{prefix}_opt_params{g}"]])
              for g, lr in enumerate(z[f"{prefix}_opt_lr"])]
    return {"state": state, "param_groups": groups}


# ------------------------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------------------------
def test_fused_adam_group_layout_matches_torch_adam():
    """Two groups over a CPU bucket, before any step: the same `param_groups` as torch.optim.Adam (indices in group
    order - the processor, declared between encoder and decoder, comes last - and lr per group)."""
    from graphcast_lite_amd.train import FlatParams, FusedAdam

    mt, mf = S.FinetuneStub(), S.FinetuneStub()
    for p in mf.processor.parameters():
        p.requires_grad = False  # frozen parameters are in the bucket all the same
    groups = _two_groups(mf, lr=3e-3, factor=0.1)
    opt = FusedAdam(FlatParams(mf, groups), param_groups=groups)
    want = torch.optim.Adam(_two_groups(mt, lr=3e-3, factor=0.1)).state_dict()
    got = opt.state_dict()
    assert got["param_groups"] == want["param_groups"] and got["state"] == want["state"] == {}
    assert got["param_groups"][1]["params"] == [4, 5]
    assert len(opt.flat.params) == 6 and opt.flat.params[4] is mf.processor.weight


def test_fused_adam_loads_per_parameter_steps_of_the_reference_run():
    """The final state of fixture run (a) - processor 9 steps, the rest 15 - loads into a two-group FusedAdam and
    comes back unchanged (the current one-counter optimiser refused it)."""
    from graphcast_lite_amd.train import FlatParams, FusedAdam

    z = _z()
    sd = _torch_state(z, "a")
    m = _stub(z)
    groups = _two_groups(m, lr=5.0)
    opt = FusedAdam(FlatParams(m, groups), param_groups=groups)
    opt.load_state_dict(sd)
    assert opt.steps() == [15, 15, 15, 15, 9, 9]  # bucket order = group order: encoder, decoder, processor
    assert [g["lr"] for g in opt.param_groups] == [0.01, 0.001]
    back = opt.state_dict()
    assert [g["params"] for g in back["param_groups"]] == [[0, 1, 2, 3], [4, 5]]
    for k, st in sd["state"].items():
        assert float(back["state"][k]["step"]) == float(st["step"])
        assert torch.equal(back["state"][k]["exp_avg"], st["exp_avg"])
        assert torch.equal(back["state"][k]["exp_avg_sq"], st["exp_avg_sq"])
    with pytest.raises(ValueError, match="number of parameter groups"):
        opt.load_state_dict(dict(sd, param_groups=sd["param_groups"][:1]))
    bad = dict(sd, param_groups=[sd["param_groups"][0], dict(sd["param_groups"][1], params=[4])])
    with pytest.raises(ValueError, match="size"):
        opt.load_state_dict(bad)
    m4 = S.FinetuneStub()
    with pytest.raises(ValueError, match="eps"):
        FusedAdam(FlatParams(m4, _two_groups(m4))).load_state_dict(
            dict(sd, param_groups=[sd["param_groups"][0], dict(sd["param_groups"][1], eps=1e-6)]))


def test_build_optimizer_is_the_reference_optimizer():
    from graphcast_lite_amd.train import build_optimizer

    z = _z()
    m = S.FinetuneStub()
    opt = build_optimizer(m, S.config(), pretrained=True)
    sd = opt.state_dict()
    assert [g["lr"] for g in sd["param_groups"]] == list(z["a_opt_lr"])
    assert [g["params"] for g in sd["param_groups"]] == [list(z["a_opt_params0"]), list(z["a_opt_params1"])]
    assert not any(p.requires_grad for p in m.processor.parameters())
    assert all(p.requires_grad for p in m.encoder.parameters())
    m2 = S.FinetuneStub()
    assert len(build_optimizer(m2, S.config(), pretrained=False).param_groups) == 1
    assert all(p.requires_grad for p in m2.parameters())


def test_train_rejects_wandb():
    from graphcast_lite_amd.train import train

    m = S.FinetuneStub()
    with pytest.raises(NotImplementedError, match="wandb"):
        train(m, [], [], None, torch.optim.Adam(m.parameters()), 1, "cpu", S.config(), ".", wandb_log=True)


def test_oracle_replays_reference_finetune_run():
    """Run (a)'s schedule - processor frozen for 2 of 5 epochs at lr x 0.1, AR 1 -> 2 - replayed with the oracle's
    loss and a two-group torch.optim.Adam reproduces the fixture: the fixture means what the GPU tests assume."""
    from oracle import train_step as T

    z = _z()
    over, epochs, _ = S.RUNS["a"]
    cfg = S.config(**over)
    m = _stub(z)
    for p in m.processor.parameters():
        p.requires_grad = False
    opt = torch.optim.Adam(_two_groups(m, cfg.learning_rate, cfg.finetune_processor_lr_factor))
    lw, cm, roi = _masks()
    kw = dict(lat_weights=lw, channel_mask=cm, spatial_mask=roi, static_channels=cfg.static_channels,
              forcing_channels=cfg.forcing_channels, use_residual=cfg.use_residual)
    train_b, val_b = _batches(z, "train"), _batches(z, "val")
    per_stage = epochs // cfg.max_ar_steps
    for ep in range(epochs):
        if ep == cfg.freeze_processor_epochs:
            for p in m.processor.parameters():
                p.requires_grad = True
        ar = min(1 + ep // per_stage, cfg.max_ar_steps)
        assert ar == z["a_ar"][ep]
        tot = 0.0
        for i, (X, y) in enumerate(train_b):
            opt.zero_grad()
            loss = T.train_step_loss(m, X, y, ar_steps=ar, epoch=ep, batch_num=i, **kw)
            loss.backward()
            opt.step()
            tot += float(loss.detach())
        assert abs(tot / len(train_b) - z["a_train_losses"][ep]) <= 2e-6 * abs(z["a_train_losses"][ep])
        vl = T.evaluate(m, val_b, lat_weights=lw, spatial_mask=roi, channel_mask=cm,
                        static_channels=cfg.static_channels, forcing_channels=cfg.forcing_channels)[0]
        assert abs(vl - z["a_val_losses"][ep]) <= 2e-6 * abs(z["a_val_losses"][ep])
    for k, p in m.named_parameters():
        assert rel(p, z[f"a_final_{k}"]) < 1e-5, k
    st = opt.state_dict()["state"]
    assert {k: int(v["step"]) for k, v in st.items()} == {0: 15, 1: 15, 2: 15, 3: 15, 4: 9, 5: 9}


# ------------------------------------------------------------------------------------------------------------------
# GPU: the kernel
# ------------------------------------------------------------------------------------------------------------------
SIZES = [37, 64, 130, 1, 200, 65]  # odd sizes that end mid-chunk


def _bucket(sizes, seed=0):
    """A padded flat bucket like FlatParams builds: (p, g, m, v, chunk map, offsets)."""
    offs, tot = [], 0
    for n in sizes:
        offs.append(tot)
        tot += (n + 63) // 64 * 64
    gen = torch.Generator().manual_seed(seed)
    p, m, v = torch.zeros(tot), torch.zeros(tot), torch.zeros(tot)
    owner = torch.empty(tot // 64, dtype=torch.int32)
    for i, (o, n) in enumerate(zip(offs, sizes)):
        p[o:o + n] = torch.randn(n, generator=gen)
        owner[o // 64:(o + (n + 63) // 64 * 64) // 64] = i
    return p, m, v, owner, offs


@pytest.mark.gpu
def test_grouped_adam_kernel_one_group_is_bit_equal_to_adam_step(lib_built):
    from graphcast_lite_amd import hip

    p, m, v, owner, offs = _bucket(SIZES)
    P = len(SIZES)
    a = [t.to(DEV) for t in (p, m, v)]
    b = [t.to(DEV) for t in (p, m, v)]
    chunk, active = owner.to(DEV), torch.ones(P, dtype=torch.int32, device=DEV)
    lr = torch.full((P,), 2e-3, device=DEV)
    step, bc = torch.zeros(P, dtype=torch.int32, device=DEV), torch.zeros(P, 2, device=DEV)
    gen = torch.Generator().manual_seed(3)
    for t in range(1, 6):
        g = torch.zeros_like(p)
        for o, n in zip(offs, SIZES):
            g[o:o + n] = torch.randn(n, generator=gen)
        g = g.to(DEV)
        hip.adam_step(a[0], g, a[1], a[2], 2e-3, 0.9, 0.999, 1e-8, 0.0, t, grad_scale=0.5)
        hip.adam_step_groups(b[0], g, b[1], b[2], chunk, active, lr, step, bc, 0.9, 0.999, 1e-8, 0.0, grad_scale=0.5)
        for x, y in zip(a, b):
            assert torch.equal(x, y), t
    assert step.cpu().tolist() == [5] * P


@pytest.mark.gpu
def test_grouped_adam_kernel_frozen_segments_and_per_parameter_steps(lib_built):
    """Two groups (lr 1e-2 and 1e-3), weight decay, parameters frozen for a while and unfrozen mid-run: frozen p, m, v
    and step bitwise untouched; active parameters match torch.optim.Adam within 1e-6, steps exactly."""
    from graphcast_lite_amd import hip

    p, m, v, owner, offs = _bucket(SIZES, seed=1)
    P = len(SIZES)
    tparams = [torch.nn.Parameter(p[o:o + n].clone()) for o, n in zip(offs, SIZES)]
    groups = [{"params": tparams[:3], "lr": 1e-2}, {"params": tparams[3:], "lr": 1e-3}]
    topt = torch.optim.Adam(groups, weight_decay=0.01)
    pd, md, vd = p.to(DEV), m.to(DEV), v.to(DEV)
    chunk = owner.to(DEV)
    lr = torch.tensor([1e-2] * 3 + [1e-3] * 3, device=DEV)
    step, bc = torch.zeros(P, dtype=torch.int32, device=DEV), torch.zeros(P, 2, device=DEV)
    frozen_until = [0, 3, 0, 2, 5, 0]  # parameter i is frozen for steps < frozen_until[i]
    gen = torch.Generator().manual_seed(4)
    for t in range(6):
        act = [int(t >= f) for f in frozen_until]
        g = torch.zeros_like(p)
        for i, (o, n) in enumerate(zip(offs, SIZES)):
            gi = torch.randn(n, generator=gen)
            g[o:o + n] = gi
            tparams[i].grad = gi.clone() if act[i] else None
        before = [x.clone() for x in (pd, md, vd)]
        st_before = step.clone()
        hip.adam_step_groups(pd, g.to(DEV), md, vd, chunk, torch.tensor(act, dtype=torch.int32, device=DEV), lr, step,
                             bc, 0.9, 0.999, 1e-8, 0.01)
        topt.step()
        for i, (o, n) in enumerate(zip(offs, SIZES)):
            if not act[i]:
                for x, y in zip((pd, md, vd), before):
                    assert torch.equal(x[o:o + (n + 63) // 64 * 64], y[o:o + (n + 63) // 64 * 64]), (t, i)
                assert int(step[i]) == int(st_before[i])
            else:
                assert rel(pd[o:o + n], tparams[i].detach()) < 1e-6, (t, i)
    want = [int(topt.state[q]["step"]) if q in topt.state else 0 for q in tparams]
    assert step.cpu().tolist() == want == [6, 3, 6, 4, 1, 6]
    for i, (o, n) in enumerate(zip(offs, SIZES)):
        # the moments carry (1 - beta) in float32 (torch: in double, 1.3e-5 apart for beta2); it cancels in the update
        assert rel(md[o:o + n], topt.state[tparams[i]]["exp_avg"]) < 1e-4
        assert rel(vd[o:o + n], topt.state[tparams[i]]["exp_avg_sq"]) < 1e-4


# ------------------------------------------------------------------------------------------------------------------
# GPU: the model step against the oracle, captured, split, checkpoints
# ------------------------------------------------------------------------------------------------------------------
def _pair(name):
    from test_hip_model import make_pair

    tweak = None
    if name == "wb2_512x256_19f_ar_v2":
        def tweak(cfg):
            cfg.pipeline.processor.gcn.num_message_passing_steps = 3  # small: the oracle runs it on the CPU
    return make_pair(name, [1, 2], tweak=tweak)


def _ar_data(cfg, G, B=2, seed=5):
    g = torch.Generator().manual_seed(seed)
    F, obs = cfg.data.num_features_used, cfg.data.obs_window_used
    X = torch.randn(B, G, obs * F, generator=g)
    y = X[..., (obs - 1) * F:].repeat(1, 1, 2) + 0.1 * torch.randn(B, G, 2 * F, generator=g)
    return X, y


# (processor frozen?, ar_steps) of each optimiser step: frozen 2, unfrozen 3, AR 1 -> 2 on the way
SCHEDULE = [(True, 1), (True, 1), (False, 1), (False, 2), (False, 2)]


def _freeze(model, frozen):
    for p in model.processor.parameters():
        p.requires_grad = not frozen


def _oracle_run(o, X, y, lw, schedule, opt=None):
    from oracle import train_step as T

    if opt is None:
        opt = torch.optim.Adam(_two_groups(o, 1e-3, 0.1))
    losses = []
    for frozen, ar in schedule:
        _freeze(o, frozen)
        opt.zero_grad()
        lo = T.train_step_loss(o, X, y, lat_weights=lw, ar_steps=ar)
        lo.backward()
        opt.step()
        losses.append(float(lo.detach()))
    return opt, losses


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["baseline", "wb2_512x256_19f_ar_v2"])
def test_grouped_train_step_matches_torch_adam_on_oracle(name, tmp_path, lib_built):
    from oracle import train_step as T
    from graphcast_lite_amd.train import TrainStep, get_lat_weights, load_checkpoint, save_checkpoint

    cfg, m, o = _pair(name)
    X, y = _ar_data(cfg, m._num_grid_nodes)
    lw, lwd = T.get_lat_weights(32, 64), get_lat_weights(32, 64, DEV)
    _freeze(m, True)
    step = TrainStep(m, lr=1e-3, lat_weights=lwd, use_graph=False, param_groups=_two_groups(m, 1e-3, 0.1))
    proc0 = {n: p.detach().clone() for n, p in m.processor.named_parameters()}
    opt, lo = _oracle_run(o, X, y, lw, SCHEDULE)
    for i, (frozen, ar) in enumerate(SCHEDULE):
        _freeze(m, frozen)
        step.ar_steps = ar
        lh = step(X.to(DEV), y.to(DEV))
        assert abs(float(lh) - lo[i]) <= 1e-4 * abs(lo[i]), (i, float(lh), lo[i])
        if frozen:
            for n, p in m.processor.named_parameters():
                assert torch.equal(p, proc0[n]), n
                assert not p.grad.any(), n  # the gradient slots of frozen parameters stay zero
    od = dict(o.named_parameters())
    for n, p in m.named_parameters():
        assert rel(p, od[n]) < 1e-4, n

    # the state in torch's layout: indices in group order, the processor's step 3, the others' 5
    sd_f, sd_t = step.opt.state_dict(), opt.state_dict()
    assert [g["params"] for g in sd_f["param_groups"]] == [g["params"] for g in sd_t["param_groups"]]
    assert [g["lr"] for g in sd_f["param_groups"]] == [g["lr"] for g in sd_t["param_groups"]]
    # a parameter no loss path reaches (the last InteractionNet step's edge norm) has no torch state; the fused step
    # updates it with zero gradients, so its moments stay zero and its weights unchanged
    assert set(sd_t["state"]) <= set(sd_f["state"])
    for i in set(sd_f["state"]) - set(sd_t["state"]):
        assert not sd_f["state"][i]["exp_avg"].any() and not sd_f["state"][i]["exp_avg_sq"].any(), i
    n_other = len(sd_t["param_groups"][0]["params"])
    for i, st in sd_t["state"].items():
        assert float(sd_f["state"][i]["step"]) == float(st["step"]) == (5.0 if i < n_other else 3.0)
        assert rel(sd_f["state"][i]["exp_avg"], st["exp_avg"]) < 1e-4
        assert rel(sd_f["state"][i]["exp_avg_sq"], st["exp_avg_sq"]) < 1e-4

    # fused -> checkpoint -> torch two-group Adam on a fresh oracle; one more step each
    path = tmp_path / "checkpoint.pth"
    save_checkpoint(path, m, step.opt, 0, 2, 1.0, 0, [], [])
    raw = torch.load(path, map_location="cpu", weights_only=True)
    _, _, o2 = _pair(name)
    o2.load_state_dict(raw["model_state_dict"], strict=True)
    opt2 = torch.optim.Adam(_two_groups(o2, 7.0, 1.0))
    opt2.load_state_dict(raw["optimizer_state_dict"])
    assert [g["lr"] for g in opt2.param_groups] == [1e-3, 1e-4]
    _oracle_run(o2, X, y, lw, [(False, 2)], opt2)
    step(X.to(DEV), y.to(DEV))
    od2 = dict(o2.named_parameters())
    for n, p in m.named_parameters():
        assert rel(p, od2[n]) < 1e-5, n

    # torch two-group state -> checkpoint -> a fresh fused step; one more step each
    torch.save({"epoch": 0, "ar_steps": 2, "best_val_loss": 1.0, "patience_counter": 0, "train_losses": [],
                "val_losses": [], "model_state_dict": o.state_dict(), "optimizer_state_dict": opt.state_dict()}, path)
    _, m3, _ = _pair(name)
    step3 = TrainStep(m3, lr=5.0, lat_weights=lwd, ar_steps=2, use_graph=False, param_groups=_two_groups(m3, 5.0, 1.0))
    load_checkpoint(path, m3, step3.opt, torch.device(DEV))
    assert [g["lr"] for g in step3.opt.param_groups] == [1e-3, 1e-4]
    _oracle_run(o, X, y, lw, [(False, 2)], opt)
    step3(X.to(DEV), y.to(DEV))
    for n, p in m3.named_parameters():
        assert rel(p, od[n]) < 1e-5, n


@pytest.mark.gpu
def test_grouped_train_step_captured_and_split_equal_eager(lib_built):
    """Captured (use_graph=True) and split_finish steps follow eager launches through freeze, unfreeze and an AR change
    on one live TrainStep; after each change the step warms up and captures a NEW graph."""
    from graphcast_lite_amd.train import TrainStep, get_lat_weights

    pairs = [_pair("baseline") for _ in range(3)]
    cfg = pairs[0][0]
    X, y = _ar_data(cfg, pairs[0][1]._num_grid_nodes)
    Xd, yd = X.to(DEV), y.to(DEV)
    lwd = get_lat_weights(32, 64, DEV)
    steps = []
    for (_, m, _), kw in zip(pairs, (dict(use_graph=False), dict(use_graph=True),
                                     dict(use_graph=True, split_finish=True))):
        _freeze(m, True)
        steps.append(TrainStep(m, lr=1e-3, lat_weights=lwd, param_groups=_two_groups(m, 1e-3, 0.1), **kw))
    phases = [(True, 1), (False, 1), (False, 2), (True, 2)]
    graphs = []  # the graphs themselves, kept alive: the id() of a freed one can come back for a new object
    for frozen, ar in phases:
        for k in range(4):  # two warm-up calls, the capture, one replay
            outs = []
            for (_, m, _), s in zip(pairs, steps):
                _freeze(m, frozen)
                s.ar_steps = ar
                outs.append(float(s(Xd * (1 + 0.01 * k), yd)))
            assert abs(outs[1] - outs[0]) <= 1e-6 * abs(outs[0]) and abs(outs[2] - outs[0]) <= 1e-6 * abs(outs[0])
        for s in steps[1:]:
            assert s.graph_active and all(s._graph is not g for g in graphs)
            graphs.append(s._graph)
    ref = dict(pairs[0][1].named_parameters())
    for _, m, _ in pairs[1:]:
        for n, p in m.named_parameters():
            assert rel(p, ref[n]) < 1e-6, n
    assert steps[0].opt.steps() == steps[1].opt.steps() == steps[2].opt.steps()


# ------------------------------------------------------------------------------------------------------------------
# GPU: the train() driver against the reference fixture
# ------------------------------------------------------------------------------------------------------------------
def _float(tok):
    try:
        return float(tok)
    except ValueError:
        return None


def _same_log(got, want):
    """Same rows; numbers in the 5 / 4 decimals of the table may differ by one unit of the last place."""
    assert len(got) == len(want), (got, want)
    for a, b in zip(got, want):
        ta, tb = a.split(), b.split()
        assert len(ta) == len(tb), (a, b)
        for x, w in zip(ta, tb):
            if "." in w and _float(w) is not None and _float(x) is not None:
                tol = 1.01 * 10.0 ** -len(w.split(".")[1])
                assert abs(_float(x) - _float(w)) <= tol, (a, b)
            else:
                assert x == w, (a, b)


def _strip(path):
    out = []
    for line in open(path).read().splitlines():
        line = re.sub(r"\s*\d{2}:\d{2}:\d{2}$", "", line)
        out.append(re.sub(r": \d{4}-\d{2}-\d{2}T[\d:.]+ ===$", " ===", line))
    return out


def _run_driver(z, run, d, epochs, model=None, resume=None, device=DEV):
    from graphcast_lite_amd.train import build_optimizer, train

    over, _, _ = S.RUNS[run]
    cfg = S.config(**over)
    m = model if model is not None else _stub(z, device)
    opt = build_optimizer(m, cfg, pretrained=True)
    res = train(m, _batches(z, "train"), _batches(z, "val"), None, opt, epochs, device, cfg, str(d),
                dataset_metadata=S.metadata(), print_losses=False, resume_checkpoint=resume)
    return m, opt, res


def _check_run(z, prefix, d, m, opt, res, log_prefix=None):
    assert len(res["train_losses"]) == len(z[f"{prefix}_train_losses"])
    for k in ("train_losses", "val_losses"):
        for a, b in zip(res[k], z[f"{prefix}_{k}"]):
            assert abs(a - b) <= 5e-6 * abs(b), (prefix, k, res[k], z[f"{prefix}_{k}"])
    with open(os.path.join(d, "results.json")) as fh:
        assert json.load(fh) == res
    log = _strip(os.path.join(d, "training_log.txt"))
    _same_log(log, list(z[f"{log_prefix or prefix}_log"]))
    rows = [line for line in log if re.match(r"^\s+\d+\s+\d+\s", line)]
    assert [int(r.split()[1]) for r in rows][-len(z[f"{prefix}_ar"]):] == list(z[f"{prefix}_ar"])
    assert [int(r.split()[6]) for r in rows] == list(z[f"{prefix}_patience"])
    stop = [line for line in log if "Early stopping" in line]
    assert (int(stop[0].split()[-1]) if stop else 0) == int(z[f"{prefix}_stop_epoch"])
    for k, p in m.named_parameters():
        assert rel(p, z[f"{prefix}_final_{k}"]) < 2e-5, (prefix, k)
    best = torch.load(os.path.join(d, "best_model.pth"), map_location="cpu", weights_only=True)
    for k, _ in m.named_parameters():
        assert rel(best[k], z[f"{prefix}_best_{k}"]) < 2e-5, (prefix, k)
    want = _torch_state(z, prefix)
    for sd in (opt.state_dict(), torch.load(os.path.join(d, "checkpoint.pth"), map_location="cpu",
                                            weights_only=True)["optimizer_state_dict"]):
        assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in want["param_groups"]]
        assert [g["lr"] for g in sd["param_groups"]] == [g["lr"] for g in want["param_groups"]]
        assert sorted(sd["state"]) == sorted(want["state"])
        for i, st in want["state"].items():
            assert float(sd["state"][i]["step"]) == float(st["step"]), (prefix, i)
            assert rel(sd["state"][i]["exp_avg"], st["exp_avg"]) < 1e-4, (prefix, i)
            assert rel(sd["state"][i]["exp_avg_sq"], st["exp_avg_sq"]) < 1e-4, (prefix, i)


@pytest.mark.gpu
@pytest.mark.parametrize("run", ["a", "b"])
def test_train_driver_reproduces_reference_run(run, tmp_path, lib_built):
    z = _z()
    _, epochs, _ = S.RUNS[run]
    m, opt, res = _run_driver(z, run, tmp_path, epochs)
    _check_run(z, run, tmp_path, m, opt, res)


@pytest.mark.gpu
def test_train_driver_resumes_its_own_and_the_reference_checkpoint(tmp_path, lib_built):
    """Run (c): 3 epochs, then a resume to 5 from checkpoint.pth - once from the checkpoint this driver wrote, once
    from the reference's (rebuilt from the fixture) - both end where the reference's resumed run ended."""
    z = _z()
    _, epochs, split = S.RUNS["c"]
    d1 = tmp_path / "own"
    d1.mkdir()
    m, opt, res = _run_driver(z, "c", d1, split)
    _check_run(z, "c1", d1, m, opt, res, log_prefix=None)
    m, opt, res = _run_driver(z, "c", d1, epochs, model=S.FinetuneStub().to(DEV),
                              resume=str(d1 / "checkpoint.pth"))
    _check_run(z, "c", d1, m, opt, res)

    d2 = tmp_path / "ref"
    d2.mkdir()
    ckpt = {k: (int(z[f"c1_ckpt_{k}"]) if k != "best_val_loss" else float(z[f"c1_ckpt_{k}"]))
            for k in ("epoch", "ar_steps", "best_val_loss", "patience_counter")}
    ckpt.update(train_losses=[float(x) for x in z["c1_train_losses"]], val_losses=[float(x) for x in z["c1_val_losses"]],
                model_state_dict={k: torch.tensor(z[f"c1_ckpt_model_{k}"]) for k, _ in S.FinetuneStub().named_parameters()},
                optimizer_state_dict=_torch_state(z, "c1_ckpt"))
    torch.save(ckpt, d2 / "checkpoint.pth")
    with open(d2 / "training_log.txt", "w") as fh:  # the reference's log of the first part
        fh.write("\n".join(z["c1_log"]) + "\n")
    m, opt, res = _run_driver(z, "c", d2, epochs, model=S.FinetuneStub().to(DEV), resume=str(d2 / "checkpoint.pth"))
    assert np.allclose(res["train_losses"][:split], z["c1_train_losses"], rtol=0, atol=0)
    for k, p in m.named_parameters():
        assert rel(p, z[f"c_final_{k}"]) < 2e-5, k
    assert [int(float(v["step"])) for _, v in sorted(opt.state_dict()["state"].items())] == [15, 15, 15, 15, 3, 3]
