"""`graphcast_lite_amd.unet.TrainableUNet`: the module tree and refusals (CPU), the entry point's parser (CPU), and one
training step and short trainings on the HIP path against the float64 functional restatement of the training forward with
torch autograd (tests/helpers/unet_train_case.py), per tensor under the rule of the unet tests:
e(hip) <= max(4 e(float32 torch CPU on the same inputs), 2^-20), e(t) = max |t - t64| / max |t64|.

The fixture tests/golden/unet_train_vectors.npz is the reference's own WeatherUNet in .train() on the CPU
(make_unet_train_golden.py): the restatement must reproduce its gradients and buffers without a GPU.

Measured on an MI355X (the ranges of the ratios e(hip) / e(cpu32) printed by the GPU tests) are in DESIGN.md 3.27."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_case as UC  # noqa: E402
import unet_train_case as TC  # noqa: E402
from layouts import same_bits  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    g = TC.golden()
    sd = UC.golden_state()
    x, go = torch.from_numpy(g["x"]), torch.from_numpy(g["go"])
    y64, g64, b64 = TC.train_step(sd, x, go, torch.float64)
    return {"g": g, "sd": sd, "x": x, "go": go, "y64": y64, "g64": g64, "b64": b64}


def _model(sd=None, cin=TC.IN, cout=TC.OUT, base=TC.BASE):
    from graphcast_lite_amd.unet import TrainableUNet

    m = TrainableUNet(cin, cout, base)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_reference_network_in_training(gold):
    """The float64 restatement against what the reference's module gave in .train(): y, 44 gradients, 28 buffers."""
    g, worst = gold["g"], 0.0
    assert UC.E(g["y"], gold["y64"]) < 2.0 ** -15
    for k, t in gold["g64"].items():
        worst = max(worst, UC.E(g["grad_" + k], t))
    for k, t in gold["b64"].items():
        worst = max(worst, UC.E(g["buf_" + k], t))
    print(f"[unet-train] fixture vs float64 restatement: worst E = {worst:.3e}")
    assert len(gold["g64"]) == 44 and len(gold["b64"]) == 28
    assert worst < 2.0 ** -15


def test_state_dict_is_the_reference_layout(gold):
    from graphcast_lite_amd.unet import WeatherUNet

    m = _model()
    keys = [str(k) for k in gold["g"]["keys"]]
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        assert tuple(sd[k].shape) == tuple(gold["sd"][k].shape), k
        assert sd[k].dtype == gold["sd"][k].dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    m.load_state_dict(gold["sd"], strict=True)
    parent = WeatherUNet(TC.IN, TC.OUT, TC.BASE)
    parent.load_state_dict(m.state_dict(), strict=True)
    m.load_state_dict(parent.state_dict(), strict=True)
    assert m.num_params == parent.num_params
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in parent.named_parameters()]
    assert isinstance(m, WeatherUNet)


def test_parser_is_the_scripts():
    from graphcast_lite_amd import downscale_train as DT

    a = DT.build_parser().parse_args(["exp", "--data-dir", "data"])
    assert (a.experiment_dir, a.data_dir, a.gnn_input, a.spectral_weight, a.gradient_weight, a.input_noise, a.augment_flip) == (
        "exp", "data", False, 0.0, 0.0, 0.0, False)
    a = DT.build_parser().parse_args(["exp", "--data-dir", "d", "--gnn-input", "--spectral-weight", "0.1", "--gradient-weight",
                                      "0.05", "--input-noise", "0.05", "--augment-flip"])
    assert (a.gnn_input, a.spectral_weight, a.gradient_weight, a.input_noise, a.augment_flip) == (True, 0.1, 0.05, 0.05, True)
    with pytest.raises(SystemExit):
        DT.build_parser().parse_args(["exp"])  # --data-dir is required
    assert DT.CONFIG_DEFAULTS == {"num_features": 19, "obs_window": 2, "batch_size": 32, "learning_rate": 1e-3,
                                  "num_epochs": 50, "patience": 15, "base_filters": 64, "static_context": True,
                                  "residual": False, "static_channels": [7, 8], "random_seed": 42}
    assert callable(DT.main)


def test_config_and_wind_channels(tmp_path):
    import json

    from graphcast_lite_amd import downscale_train as DT

    assert DT.load_config(str(tmp_path)) == DT.CONFIG_DEFAULTS
    (tmp_path / "config.json").write_text(json.dumps({"base_filters": 8, "residual": True}))
    cfg = DT.load_config(str(tmp_path))
    assert cfg["base_filters"] == 8 and cfg["residual"] is True and cfg["num_epochs"] == 50
    assert DT.wind_u_channels(str(tmp_path)) == ()
    (tmp_path / "variables.json").write_text(json.dumps(["2t", "10u", "10v", "u@850", "v@850", "u@500"]))
    assert DT.wind_u_channels(str(tmp_path)) == (1, 3, 5)


def test_refusals():
    m = _model().train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(torch.zeros(1, TC.IN, 8, 15))
    with pytest.raises(ValueError, match="residual_from"):
        m(torch.zeros(2, TC.IN, 16, 24), residual_from=(0, 3))
    with pytest.raises(ValueError, match="requires grad"):
        m(torch.zeros(2, TC.IN, 16, 24, requires_grad=True))
    with pytest.raises(ValueError, match="expected"):
        m(torch.zeros(2, TC.IN + 1, 16, 24))
    with pytest.raises(ValueError, match="at least 8 x 8"):
        m(torch.zeros(2, TC.IN, 7, 24))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m(torch.zeros(2, TC.IN, 16, 24))
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(2, TC.IN, 16, 24, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="GPU tensors"):
        m.eval()(torch.zeros(2, TC.IN, 16, 24))  # eval mode is the parent's forward


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _step(m, x, go):
    y = m(x)
    y.backward(go)
    return y.detach()


def _check_step(m, y, y32, g32, b32, y64, g64, b64, what):
    UC.check(y, y64, y32, f"{what} y")
    named = dict(m.named_parameters())
    assert set(named) == set(g64)
    for k, t64 in g64.items():
        assert named[k].grad is not None and named[k].grad.shape == named[k].shape, k
        UC.check(named[k].grad, t64, g32[k], f"{what} grad {k}")
    sd = m.state_dict()
    for k, t64 in b64.items():
        UC.check(sd[k], t64, b32[k], f"{what} buffer {k}")


@pytest.mark.gpu
def test_one_step_is_the_fixture(gold):
    g = gold["g"]
    m = _model(gold["sd"]).to(DEV).train()
    y = _step(m, gold["x"].to(DEV), gold["go"].to(DEV))
    assert y.shape == gold["y64"].shape
    g32 = {k: torch.from_numpy(g["grad_" + k]) for k in gold["g64"]}
    b32 = {k: torch.from_numpy(g["buf_" + k]) for k in gold["b64"]}
    _check_step(m, y, torch.from_numpy(g["y"]), g32, b32, gold["y64"], gold["g64"], gold["b64"], "fixture")
    nbt = [int(v) for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 14 and set(nbt) == {8} == {int(g["nbt"])}


@pytest.mark.gpu
def test_one_step_odd_sizes():
    """13 x 22 at B = 3: pools that drop a row or a column, all three pads, an upsampling from a single row; six values per
    channel at the deepest level."""
    sd = TC.random_state(99)
    gen = torch.Generator().manual_seed(5)
    x, go = torch.randn(3, TC.IN, 13, 22, generator=gen), torch.randn(3, TC.OUT, 13, 22, generator=gen)
    y64, g64, b64 = TC.train_step(sd, x, go, torch.float64)
    y32, g32, b32 = TC.train_step(sd, x, go, torch.float32)
    m = _model(sd).to(DEV).train()
    y = _step(m, x.to(DEV), go.to(DEV))
    _check_step(m, y, y32, g32, b32, y64, g64, b64, "13x22 B=3")


@pytest.mark.gpu
def test_backward_repeats_accumulates_and_eval_is_the_parents(gold):
    from graphcast_lite_amd.unet import WeatherUNet

    x, go = gold["x"].to(DEV), gold["go"].to(DEV)
    m = _model(gold["sd"]).to(DEV).train()
    y1 = _step(m, x, go)
    first = {k: p.grad.clone() for k, p in m.named_parameters()}
    # eval between two training steps: the parent's bits, no grad, and the training workspace survives it
    parent = WeatherUNet(TC.IN, TC.OUT, TC.BASE)
    parent.load_state_dict(m.state_dict(), strict=True)
    parent = parent.to(DEV).eval()
    ye = m.eval()(x)
    assert not ye.requires_grad and same_bits(ye, parent(x))
    assert same_bits(m(x, residual_from=(1, 4)), parent(x, residual_from=(1, 4)))
    m.train()
    # a second backward without zero_grad accumulates: the buffers moved, but gradients do not read running statistics
    y2 = _step(m, x, go)
    assert same_bits(y1, y2)
    for k, p in m.named_parameters():
        assert same_bits(p.grad, first[k] + first[k]), k
    m.zero_grad()
    _step(m, x, go)
    for k, p in m.named_parameters():
        assert same_bits(p.grad, first[k]), k
    # a frozen parameter gets no gradient, the others the same bits
    m.zero_grad()
    m.down2.net[1].net[0].weight.requires_grad_(False)
    m.up1.conv.net[1].bias.requires_grad_(False)
    _step(m, x, go)
    for k, p in m.named_parameters():
        if p.requires_grad:
            assert same_bits(p.grad, first[k]), k
        else:
            assert p.grad is None, k
    # a backward after another forward of the same shape is refused, not answered from the wrong activations
    ya = m(x)
    m(x)
    with pytest.raises(RuntimeError, match="another training forward"):
        ya.backward(go)


@pytest.mark.gpu
def test_three_adamw_steps():
    from graphcast_lite_amd.downscale_train import downscaler_loss
    from graphcast_lite_amd.unet import WeatherUNet

    sd = TC.random_state(123)
    gen = torch.Generator().manual_seed(17)
    x, Y = torch.randn(2, TC.IN, 16, 24, generator=gen), torch.randn(2, TC.OUT, 16, 24, generator=gen)

    def restated(dtype):
        state, losses, opt = None, [], None
        for _ in range(3):
            y, params, buffers = TC.train_forward(sd, x, dtype, state)
            if opt is None:
                state = (params, buffers)
                opt = torch.optim.AdamW(list(params.values()), lr=1e-3, weight_decay=1e-5)
            opt.zero_grad()
            loss = ((y - Y.to(dtype)) ** 2).mean()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        after = dict(sd)
        after.update({k: v.detach() for k, v in params.items()})
        after.update(buffers)
        return losses, after

    l64, sd64 = restated(torch.float64)
    l32, sd32 = restated(torch.float32)
    m = _model(sd).to(DEV).train()
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    xd, Yd = x.to(DEV), Y.to(DEV)
    for k in range(3):
        opt.zero_grad()
        loss = downscaler_loss(m(xd), Yd)
        loss.backward()
        opt.step()
        lv = float(loss.detach())
        e_hip, e_cpu = abs(lv - l64[k]) / abs(l64[k]), abs(l32[k] - l64[k]) / abs(l64[k])
        print(f"[unet-train] AdamW step {k}: loss {lv:.8f}, e(hip) = {e_hip:.3e}, e(cpu32) = {e_cpu:.3e}")
        assert e_hip <= max(4 * e_cpu, UC.FLOOR), f"step {k}"
    assert l64[2] < l64[0]
    # the updated state in a fresh inference module: both packs were rebuilt, the buffers carried over
    fresh = WeatherUNet(TC.IN, TC.OUT, TC.BASE)
    fresh.load_state_dict(m.state_dict(), strict=True)
    y_eval = fresh.to(DEV).eval()(xd)
    UC.check(y_eval, UC.functional_unet(sd64, x.double()), UC.functional_unet(sd32, x), "eval after three steps")


@pytest.mark.gpu
def test_train_epoch_and_validate_on_a_tiny_dataset():
    from graphcast_lite_amd import downscale_train as DT
    from graphcast_lite_amd.downscale import DownscalerDataset, DownscalerPairs

    T, n_lon, n_lat, C = 11, 24, 16, 3
    gen = torch.Generator().manual_seed(3)
    fine = torch.randn(T, n_lon, n_lat, C, generator=gen)
    coarse = fine + 0.3 * torch.randn(T, n_lon, n_lat, C, generator=gen)
    scalers = {"mean": np.zeros(C, dtype=np.float32), "std": np.ones(C, dtype=np.float32)}
    pairs = DownscalerPairs(coarse.half().to(DEV), fine.half().to(DEV), None, scalers, np.linspace(50, 56, n_lat),
                            np.linspace(80, 92, n_lon), {"static_channels": []}, [f"v{i}" for i in range(C)])
    train_ds = DownscalerDataset(pairs, obs_window=2, split="train", static_context=False)
    val_ds = DownscalerDataset(pairs, obs_window=2, split="val", static_context=False)
    assert len(train_ds) == 8 and len(val_ds) == 1
    torch.manual_seed(0)
    m = _model(None, cin=2 * C, cout=C, base=8).to(DEV)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-5)
    mask = torch.ones(C, device=DEV)
    per_batch = []
    tl = DT.train_epoch(m, DT.iter_batches(train_ds, 4, drop_last=True), opt, mask, True, obs_window=2, per_batch=per_batch)
    vl = DT.validate(m, DT.iter_batches(val_ds, 4), mask, True, C, 2)
    assert len(per_batch) == 2 and np.isfinite(tl) and np.isfinite(vl)
    assert not m.training
    for k, p in m.named_parameters():
        assert torch.isfinite(p).all() and not torch.equal(p.detach(), before[k]), k
    assert int(m.inc.net[1].num_batches_tracked) == 2
