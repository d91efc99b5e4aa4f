"""`graphcast_lite_amd.unet_v2.WeatherUNetV2`: the reference's module tree (CPU), and its eval-mode forward on the HIP
path against a float64 functional restatement of the network (tests/helpers/unet_v2_case.py) under the rule
e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20), e(y) = max |y - y64| / max |y64|.

The fixture tests/golden/unet_v2_vectors.npz is the reference's own WeatherUNetV2 on the CPU (make_unet_v2_golden.py):
the restatement must reproduce its y without a GPU, which shows that the oracle is the reference's network."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_v2_case as VC  # noqa: E402
from layouts import same_bits  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    g = VC.golden()
    sd = VC.golden_state(g)
    x = torch.from_numpy(g["x"])
    return {"g": g, "sd": sd, "x": x, "y": torch.from_numpy(g["y"]),
            "y64": VC.functional_unet_v2(sd, x.double(), VC.HEADS, VC.MODES)}


def _model(sd=None, cin=VC.IN, cout=VC.OUT, f=VC.BASE, heads=VC.HEADS, modes=VC.MODES):
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    m = WeatherUNetV2(cin, cout, f, heads, modes)
    if sd is not None:
        m.load_state_dict(sd, strict=True)
    return m.eval()


def _random_case(cin, f, heads, modes, seed):
    m = VC.randomise_(_model(cin=cin, f=f, heads=heads, modes=modes), seed)
    return m, {k: v.detach().clone() for k, v in m.state_dict().items()}


def _oracle(sd, x, heads, modes, rf=None):
    return VC.functional_unet_v2(sd, x.double(), heads, modes, rf), VC.functional_unet_v2(sd, x, heads, modes, rf)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_is_the_reference_network(gold):
    """The float64 restatement against the y the reference's module gave."""
    e = VC.E(gold["y"], gold["y64"])
    y32 = VC.functional_unet_v2(gold["sd"], gold["x"], VC.HEADS, VC.MODES)
    print(f"[unet_v2] fixture y vs float64 restatement: E = {e:.3e}; float32 restatement: E = {VC.E(y32, gold['y64']):.3e}")
    assert e < 2.0 ** -18
    assert VC.E(y32, gold["y64"]) < 2.0 ** -18


def test_state_dict_is_the_reference_layout(gold):
    m = _model()
    keys = [str(k) for k in gold["g"]["keys"]]
    sd = m.state_dict()
    assert len(keys) == 97 and list(sd.keys()) == keys
    for k in keys:
        assert tuple(sd[k].shape) == tuple(gold["g"]["sd_" + k].shape), k
        assert sd[k].dtype == torch.float32, k
    m.load_state_dict(gold["sd"], strict=True)
    assert same_bits(m.bottleneck_spectral.weights_im.detach(), gold["sd"]["bottleneck_spectral.weights_im"])


def test_num_params(gold):
    m = _model()
    assert m.num_params == sum(gold["g"]["sd_" + str(k)].size for k in gold["g"]["keys"]) == int(gold["g"]["num_params"])


def test_identity_skip_has_no_key():
    m = _model(cin=8, f=8)
    sd = m.state_dict()
    assert "inc.skip.weight" not in sd and "down1.conv.skip.weight" in sd and len(sd) == 96


def test_value_errors():
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    for bad in (6, 0, 10):
        with pytest.raises(ValueError, match="multiple of 4"):
            WeatherUNetV2(6, 3, base_filters=bad)
    with pytest.raises(ValueError, match="attn_heads"):
        WeatherUNetV2(6, 3, base_filters=4, attn_heads=5)
    with pytest.raises(ValueError, match="spectral_modes"):
        WeatherUNetV2(6, 3, base_filters=4, spectral_modes=0)
    m = _model()
    for shape in ((1, VC.IN, 7, 22), (1, VC.IN, 13, 7)):
        with pytest.raises(ValueError, match="at least 8 x 8"):
            m(torch.zeros(shape))
    with pytest.raises(ValueError, match="input"):
        m(torch.zeros(1, VC.IN + 1, 13, 22))
    with pytest.raises(ValueError, match="residual_from"):
        m(torch.zeros(1, VC.IN, 13, 22), residual_from=(0, 2))


def test_training_mode_is_refused():
    m = _model().train()
    with pytest.raises(NotImplementedError, match="inference-only"):
        m(torch.zeros(1, VC.IN, 13, 22))


def test_cpu_and_dtype_are_refused():
    m = _model()
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        m(torch.zeros(1, VC.IN, 13, 22))
    with pytest.raises(RuntimeError, match="float32.*there is no CPU fallback"):
        m(torch.zeros(1, VC.IN, 13, 22, dtype=torch.float64))


@pytest.mark.parametrize("what", ["spectral", "attn_proj", "se", "skip"])
def test_oracle_sees_every_branch(gold, what):
    """Zeroing a branch's weights in the fixture's state dict moves the float64 output by E > 1e-2: no branch can be
    wrong unnoticed."""
    sd = {k: v.clone() for k, v in gold["sd"].items()}
    zero = {"spectral": ["bottleneck_spectral.weights_re", "bottleneck_spectral.weights_im"],
            "attn_proj": ["bottleneck_attn.proj.weight", "bottleneck_attn.proj.bias"],
            "se": ["up2.conv.se.fc.4.weight", "up2.conv.se.fc.4.bias"],
            "skip": ["down2.conv.skip.weight"]}[what]
    for k in zero:
        sd[k].zero_()
    e = VC.E(VC.functional_unet_v2(sd, gold["x"].double(), VC.HEADS, VC.MODES), gold["y64"])
    print(f"[unet_v2] {what} zeroed: E = {e:.3e}")
    assert e > 1e-2


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fixture_output(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    y = m(gold["x"].to(DEV))
    assert y.shape == gold["y"].shape and not y.requires_grad and y.grad_fn is None
    VC.check(y, gold["y64"], gold["y"], "v2 fixture 27 x 45, B = 2")
    assert same_bits(m(gold["x"].to(DEV)), y), "two calls differ"


# B, H, W, in, base_filters, heads, modes
SHAPES = [(1, 8, 9, 6, 8, 4, 4),       # 1 x 1 bottleneck: one token, a single mode
          (1, 13, 22, 6, 8, 4, 4),     # 1 x 2: the Nyquist column is kept (c = 1)
          (2, 41, 61, 6, 8, 4, 4),     # 5 x 7: mh = 4 < Hb, all 4 columns, odd Wb
          (1, 32, 48, 6, 12, 4, 4),    # 4 x 6: Nyquist kept, mh = Hb, GroupNorm groups of 2 channels (g = 6)
          (1, 40, 64, 6, 4, 4, 4),     # 5 x 8: mw = 4 < 5, even Wb without the Nyquist column
          (3, 16, 24, 8, 8, 4, 4),     # in = f: identity skip, no pads
          (1, 128, 160, 6, 4, 4, 4),   # 320 tokens
          (1, 13, 22, 6, 8, 1, 4), (1, 13, 22, 6, 8, 8, 4),    # heads 1 and 8
          (1, 41, 61, 6, 8, 4, 1), (1, 41, 61, 6, 8, 4, 6)]    # spectral_modes 1 and 6


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cin,f,heads,modes", SHAPES)
def test_other_shapes(lib_built, B, H, W, cin, f, heads, modes):
    m, sd = _random_case(cin, f, heads, modes, seed=100 + H + f + heads + modes)
    x = torch.randn(B, cin, H, W, generator=torch.Generator().manual_seed(7))
    m = m.to(DEV)
    y = m(x.to(DEV))
    y64, y32 = _oracle(sd, x, heads, modes)
    VC.check(y, y64, y32, f"v2 {H} x {W}, B = {B}, in {cin}, f {f}, heads {heads}, modes {modes}")
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
    """Loading a new state dict needs no extra call: the packed weights follow the weights' versions; the vectors read
    at the call follow by themselves."""
    x = gold["x"]
    _, sd2 = _random_case(VC.IN, VC.BASE, VC.HEADS, VC.MODES, seed=99)
    m = _model(gold["sd"]).to(DEV)
    y1 = m(x.to(DEV)).clone()
    m.load_state_dict(sd2, strict=True)
    y2 = m(x.to(DEV)).clone()
    VC.check(y1, gold["y64"], gold["y"], "v2 first state dict")
    VC.check(y2, *_oracle(sd2, x, VC.HEADS, VC.MODES), "v2 second state dict")
    assert VC.E(y2, y1) > 1e-2, "the second state dict did not reach the kernels"
    with torch.no_grad():
        m.down1.conv.conv[4].bias.add_(0.25)  # a GroupNorm bias alone
    sd3 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    y3 = m(x.to(DEV)).clone()
    VC.check(y3, *_oracle(sd3, x, VC.HEADS, VC.MODES), "v2 new GroupNorm bias")
    assert VC.E(y3, y2) > 1e-4
    with torch.no_grad():
        m.bottleneck_spectral.weights_im.mul_(-1.5)  # in place: the version moves, the pointer does not
    sd4 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    y4 = m(x.to(DEV))
    VC.check(y4, *_oracle(sd4, x, VC.HEADS, VC.MODES), "v2 weights_im changed in place")
    assert VC.E(y4, y3) > 1e-4


@pytest.mark.gpu
def test_residual_from(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    x = gold["x"]
    rf = (VC.IN - VC.OUT, VC.IN)  # ((obs - 1) * C, obs * C) with obs = 2, C = 3
    y = m(x.to(DEV), residual_from=rf)
    VC.check(y, *_oracle(gold["sd"], x, VC.HEADS, VC.MODES, rf), "v2 residual_from")
    assert same_bits(y, x.to(DEV)[:, rf[0]:rf[1]] + m(x.to(DEV)))


@pytest.mark.gpu
def test_nan_stays_in_its_sample(gold, lib_built):
    m = _model(gold["sd"]).to(DEV)
    x = gold["x"].to(DEV)
    clean = m(x).clone()
    bad = x.clone()
    bad[1, 2, 5, 7] = float("nan")
    got = m(bad)
    assert same_bits(got[0], clean[0]), "a NaN in sample 1 reached sample 0"
    assert bool(got[1].isnan().any())


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
    _, sd2 = _random_case(VC.IN, VC.BASE, VC.HEADS, VC.MODES, seed=98)
    m.load_state_dict(sd2, strict=True)
    got2 = cap(x).clone()
    assert cap.graph_active
    assert same_bits(got2, m(x)) and VC.E(got2, want) > 1e-2


def _launches(hip):
    return hip.unet_launches() + hip.unet_v2_launches()


@pytest.mark.gpu
def test_forward_is_seventy_two_launches(gold, lib_built):
    from graphcast_lite_amd import hip
    from graphcast_lite_amd.unet_v2 import WeatherUNetV2

    assert WeatherUNetV2.LAUNCHES == 72
    m = _model(gold["sd"]).to(DEV)
    x = gold["x"].to(DEV)
    n0 = _launches(hip)
    m(x)  # packs the 16 convolution weights and the spectral weights first
    assert _launches(hip) - n0 == 17 + 72
    u0, v0 = hip.unet_launches(), hip.unet_v2_launches()
    m(x)
    assert (hip.unet_launches() - u0, hip.unet_v2_launches() - v0) == (17, 55)
    for touched in (m.up2.conv.conv[3].weight, m.bottleneck_spectral.weights_im, m.inc.skip.weight):
        with torch.no_grad():
            touched.mul_(1.0)  # a packed weight touched: its own pack; the skip is read at the call: none
        n1 = _launches(hip)
        m(x)
        assert _launches(hip) - n1 == (72 if touched is m.inc.skip.weight else 73)
    for shape in ((1, VC.IN, 16, 24), (3, VC.IN, 16, 24)):  # another grid (2 x 2 modes: one more spectral pack), another B
        xs = torch.zeros(shape, device=DEV)
        m(xs)
        n2 = _launches(hip)
        m(xs)
        assert _launches(hip) - n2 == 72, shape
    assert sorted(m._packed_spec) == [(2, 2), (3, 3)]
