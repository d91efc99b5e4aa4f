"""`graphcast_lite_amd.unet.WeatherUNet`: the reference's module tree (CPU), and its eval-mode forward on the HIP path
against a float64 functional restatement of the network (tests/helpers/unet_case.py) under the rule
e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20), e(y) = max |y - y64| / max |y64|.

The fixture tests/golden/unet_vectors.npz is the reference's own WeatherUNet on the CPU (make_unet_golden.py): the
restatement must reproduce its y without a GPU, which shows that the oracle is the reference's network."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_case as UC  # noqa: E402
from layouts import same_bits  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    g = UC.golden()
    sd = UC.golden_state(g)
    x = torch.from_numpy(g["x"])
    return {"g": g, "sd": sd, "x": x, "y": torch.from_numpy(g["y"]), "y64": UC.functional_unet(sd, x.double())}


def _model(sd=None, **kw):
    from graphcast_lite_amd.unet import WeatherUNet

    m = WeatherUNet(UC.IN, UC.OUT, UC.BASE, **kw)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.eval()


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_reference_network(gold):
    """The float64 restatement against the y the reference's module gave: float32 rounding of a 15-layer network."""
    e = UC.E(gold["y"], gold["y64"])
    y32 = UC.functional_unet(gold["sd"], gold["x"])
    print(f"[unet] fixture y vs float64 restatement: E = {e:.3e}; float32 restatement vs fixture: "
          f"{float((y32 - gold['y']).abs().max()):.3e}")
    assert e < 2.0 ** -18
    assert UC.E(y32, gold["y64"]) < 2.0 ** -18


def test_state_dict_is_the_reference_layout(gold):
    m = _model()
    keys = [str(k) for k in gold["g"]["keys"]]
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    for k in keys:
        assert tuple(sd[k].shape) == tuple(gold["g"]["sd_" + k].shape), k
        assert sd[k].dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    m.load_state_dict(gold["sd"], strict=True)
    assert int(m.inc.net[1].num_batches_tracked) == 7


def test_num_params(gold):
    m = _model()
    trainable = sum(gold["g"]["sd_" + str(k)].size for k in gold["g"]["keys"]
                    if not any(str(k).endswith(s) for s in ("running_mean", "running_var", "num_batches_tracked")))
    assert m.num_params == trainable == int(gold["g"]["num_params"])


def test_value_errors():
    from graphcast_lite_amd.unet import WeatherUNet

    for bad in (6, 0, 10):
        with pytest.raises(ValueError, match="multiple of 4"):
            WeatherUNet(7, 3, base_filters=bad)
    m = _model()
    for shape in ((1, UC.IN, 7, 22), (1, UC.IN, 13, 7)):
        with pytest.raises(ValueError, match="at least 8 x 8"):
            m(torch.zeros(shape))
    with pytest.raises(ValueError, match="input"):
        m(torch.zeros(1, UC.IN + 1, 13, 22))
    with pytest.raises(ValueError, match="residual_from"):
        m(torch.zeros(1, UC.IN, 13, 22), residual_from=(0, 2))


def test_training_mode_is_refused():
    m = _model().train()
    with pytest.raises(NotImplementedError, match="inference-only.*fit_downscaler"):
        m(torch.zeros(1, UC.IN, 13, 22))


def test_cpu_and_dtype_are_refused():
    m = _model()
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        m(torch.zeros(1, UC.IN, 13, 22))
    with pytest.raises(RuntimeError, match="float32"):
        m(torch.zeros(1, UC.IN, 13, 22, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fixture_output(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    y = m(gold["x"].to(DEV))
    assert y.shape == gold["y"].shape and not y.requires_grad and y.grad_fn is None
    UC.check(y, gold["y64"], gold["y"], "fixture 13 x 22, B = 2")
    assert same_bits(m(gold["x"].to(DEV)), y), "two calls differ"


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(1, 8, 9), (3, 13, 22)])
def test_other_shapes(gold, lib_built, B, H, W):
    x = torch.randn(B, UC.IN, H, W, generator=torch.Generator().manual_seed(7))
    m = _model(gold["sd"]).to(DEV)
    y = m(x.to(DEV))
    UC.check(y, UC.functional_unet(gold["sd"], x.double()), UC.functional_unet(gold["sd"], x), f"{H} x {W}, B = {B}")
    for b in range(B):  # a sample's bits do not depend on the batch or on its place in it
        assert same_bits(m(x[b:b + 1].to(DEV)), y[b:b + 1]), f"sample {b} alone differs from its row of B = {B}"


@pytest.mark.gpu
def test_non_contiguous_input(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    x = gold["x"].to(DEV)
    xt = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not xt.is_contiguous()
    assert same_bits(m(xt), m(x))


@pytest.mark.gpu
def test_two_state_dicts_in_turn(gold, lib_built):
    """Loading a new state dict needs no extra call: the packed weights follow the weights' versions."""
    from graphcast_lite_amd.unet import WeatherUNet

    x = gold["x"]
    sd2 = UC.randomise_(WeatherUNet(UC.IN, UC.OUT, UC.BASE), 99).state_dict()
    m = _model(gold["sd"]).to(DEV)
    y1 = m(x.to(DEV)).clone()
    m.load_state_dict(sd2, strict=True)
    y2 = m(x.to(DEV)).clone()
    UC.check(y1, gold["y64"], gold["y"], "first state dict")
    UC.check(y2, UC.functional_unet(sd2, x.double()), UC.functional_unet(sd2, x), "second state dict")
    assert UC.E(y2, y1) > 1e-2, "the second state dict did not reach the kernels"
    # new statistics alone (no weight changes): the epilogue reads the four vectors at the call
    with torch.no_grad():
        m.inc.net[1].running_mean.add_(0.25)
    sd3 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    y3 = m(x.to(DEV))
    UC.check(y3, UC.functional_unet(sd3, x.double()), UC.functional_unet(sd3, x), "new running mean")
    assert UC.E(y3, y2) > 1e-4


@pytest.mark.gpu
def test_residual_from(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    x = gold["x"]
    rf = (UC.IN - UC.OUT - 1, UC.IN - 1)
    y = m(x.to(DEV), residual_from=rf)
    UC.check(y, UC.functional_unet(gold["sd"], x.double(), rf), UC.functional_unet(gold["sd"], x, rf), "residual_from")
    # the fused add is the float32 sum of the slice and the plain output, rounded once
    assert same_bits(y, x.to(DEV)[:, rf[0]:rf[1]] + m(x.to(DEV)))


@pytest.mark.gpu
def test_captured_equals_eager(gold, lib_built):
    from graphcast_lite_amd.unet import CapturedUNet

    m = _model(gold["sd"]).to(DEV)
    x = gold["x"].to(DEV)
    want = m(x).clone()
    cap = CapturedUNet(m, use_graph=True, required=True)
    for _ in range(cap.warmup + 2):
        got = cap(x)
    assert cap.graph_active
    assert same_bits(got, want)
    x2 = torch.flip(x, dims=[0]).contiguous()
    assert same_bits(cap(x2), m(x2))


@pytest.mark.gpu
def test_forward_is_fifteen_launches(gold, lib_built):
    from graphcast_lite_amd import hip

    m = _model(gold["sd"]).to(DEV)
    x = gold["x"].to(DEV)
    n0 = hip.unet_launches()
    m(x)  # packs the 14 weights first
    assert hip.unet_launches() - n0 == 14 + 15
    n1 = hip.unet_launches()
    m(x)
    assert hip.unet_launches() - n1 == 15
    with torch.no_grad():
        m.up2.conv.net[3].weight.mul_(1.0)  # one weight touched: one pack
    n2 = hip.unet_launches()
    m(x)
    assert hip.unet_launches() - n2 == 16
