"""The kernels of csrc/unet_train.hip one by one, against float64 torch autograd on the CPU under the rule of the unet
tests: per tensor, e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20), e(t) = max |t - t64| / max |t64|.
`pool_bwd` is bit-equal to torch's CPU max_pool2d backward plus one float32 add.  The shapes are the smallest at which
each kernel can go wrong: the chunk edges of colsum.h (64 rows a chunk), one pixel tile, edge tiles, the deep level where
most taps fall on padding, every source kind, both sides of every dispatch decision of the weight gradient."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_case as UC  # noqa: E402
from layouts import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, MOM = 1e-5, 0.1
ROWS = (2, 63, 64, 65, 129)  # one chunk short, exactly one chunk, one row into the second, into the third


def _hip():
    from graphcast_lite_amd import hip

    hip.lib()
    return hip


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _planar(rows):
    """channels-last [B, H, W, C] -> [B, C, H, W]"""
    return rows.permute(0, 3, 1, 2)


def _rows(planar):
    return planar.permute(0, 2, 3, 1).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# BatchNorm statistics, BatchNorm + GELU forward and backward
# ---------------------------------------------------------------------------------------------------------------------
def _bn_case(n, C, seed):
    g = _gen(seed)
    z = torch.randn(n, C, generator=g) * 1.5 + 0.4
    z[:, 1] = 0.75  # a constant channel: var = 0, invstd = 1 / sqrt(eps)
    return {"z": z, "gamma": 0.75 + 0.5 * torch.rand(C, generator=g), "beta": 0.2 * torch.randn(C, generator=g),
            "rm": 0.3 * torch.randn(C, generator=g), "rv": 0.5 + torch.rand(C, generator=g), "dA": torch.randn(n, C, generator=g)}


def _bn_oracle(c, dtype):
    z = c["z"].to(dtype).clone().requires_grad_(True)
    gamma, beta = c["gamma"].to(dtype).clone().requires_grad_(True), c["beta"].to(dtype).clone().requires_grad_(True)
    rm, rv = c["rm"].to(dtype).clone(), c["rv"].to(dtype).clone()
    a = F.gelu(F.batch_norm(z, rm, rv, gamma, beta, training=True, momentum=MOM, eps=EPS))
    a.backward(c["dA"].to(dtype))
    zd = z.detach()
    mean, var = zd.mean(0), zd.var(0, unbiased=False)
    return {"mean": mean, "invstd": 1 / torch.sqrt(var + EPS), "rm": rm, "rv": rv, "a": a.detach(), "dZ": z.grad,
            "dgamma": gamma.grad, "dbeta": beta.grad}


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("n", ROWS)
def test_bn_stats_gelu_and_backward(n, C):
    hip = _hip()
    c = _bn_case(n, C, 100 * n + C)
    o64, o32 = _bn_oracle(c, torch.float64), _bn_oracle(c, torch.float32)
    d = {k: v.to(DEV) for k, v in c.items()}
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    nbt = torch.tensor(7, dtype=torch.int64, device=DEV)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    hip.unet_bn_stats(d["z"], EPS, MOM, mean, invstd, rm, rv, nbt)
    assert int(nbt) == 8
    for name, got in (("mean", mean), ("invstd", invstd), ("rm", rm), ("rv", rv)):
        UC.check(got, o64[name], o32[name], f"bn_stats n={n} C={C} {name}")
    assert abs(float(invstd[1]) - EPS ** -0.5) <= 2.0 ** -20 * EPS ** -0.5, "constant channel: invstd = 1 / sqrt(eps)"
    # running update without a counter, and bit-equal repeats
    mean2, invstd2 = torch.empty_like(mean), torch.empty_like(invstd)
    hip.unet_bn_stats(d["z"], EPS, MOM, mean2, invstd2)
    assert same_bits(mean, mean2) and same_bits(invstd, invstd2)

    a = torch.empty_like(d["z"])
    hip.unet_bn_gelu(d["z"], d["gamma"], d["beta"], mean, invstd, a)
    UC.check(a, o64["a"], o32["a"], f"bn_gelu n={n} C={C}")

    dZ, dgamma, dbeta = torch.empty_like(d["z"]), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    hip.unet_bn_gelu_bwd(d["z"], d["dA"], d["gamma"], d["beta"], mean, invstd, dZ, dgamma, dbeta)
    UC.check(dgamma, o64["dgamma"], o32["dgamma"], f"bn_gelu_bwd n={n} C={C} dgamma")
    UC.check(dbeta, o64["dbeta"], o32["dbeta"], f"bn_gelu_bwd n={n} C={C} dbeta")
    UC.check(dZ, o64["dZ"], o32["dZ"], f"bn_gelu_bwd n={n} C={C} dZ")
    # in place, and twice: equal bits
    dA2, dg2, db2 = d["dA"].clone(), torch.empty_like(dgamma), torch.empty_like(dbeta)
    hip.unet_bn_gelu_bwd(d["z"], dA2, d["gamma"], d["beta"], mean, invstd, dA2, dg2, db2)
    assert same_bits(dA2, dZ) and same_bits(dg2, dgamma) and same_bits(db2, dbeta)


def test_bn_stats_refuses_one_row():
    hip = _hip()
    z = torch.randn(1, 4, device=DEV)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        hip.unet_bn_stats(z, EPS, MOM, torch.empty(4, device=DEV), torch.empty(4, device=DEV))
    rc = hip.lib().gcl_unet_bn_stats(z.data_ptr(), 1, 4, EPS, MOM, z.data_ptr(), z.data_ptr(), None, None, None, z.data_ptr(), 64, None)
    assert rc != 0 and b"more than 1 value" in hip.lib().gcl_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Sources, as the kernels read them and as torch restates them
# ---------------------------------------------------------------------------------------------------------------------
def _source(kind, B, H, W, Cin, seed, low=None, C1=None):
    """(tensors, restate): `tensors` are the float32 CPU tensors the descriptor points at; restate(dtype) the planar
    input [B, Cin, H, W] torch builds from them."""
    g = _gen(seed)
    if kind == "planar":
        x = torch.randn(B, Cin, H, W, generator=g)
        return (x,), lambda dt: x.to(dt)
    if kind == "rows":
        a = torch.randn(B, H, W, Cin, generator=g)
        return (a,), lambda dt: _planar(a.to(dt))
    if kind == "pool":
        Hs, Ws = low
        a = torch.randn(B, Hs, Ws, Cin, generator=g)
        return (a,), lambda dt: F.max_pool2d(_planar(a.to(dt)), 2)
    Hs, Ws = low
    skip, lo = torch.randn(B, H, W, C1, generator=g), torch.randn(B, Hs, Ws, Cin - C1, generator=g)

    def restate(dt):
        up = F.interpolate(_planar(lo.to(dt)), scale_factor=2, mode="bilinear", align_corners=True)
        up = F.pad(up, [0, W - up.shape[3], 0, H - up.shape[2]])
        return torch.cat([_planar(skip.to(dt)), up], dim=1)

    return (skip, lo), restate


def _descriptor(hip, kind, tensors):
    dev = [t.to(DEV).contiguous() for t in tensors]
    k = {"planar": hip.UNET_PLANAR, "rows": hip.UNET_ROWS, "pool": hip.UNET_POOL, "upcat": hip.UNET_UPCAT}[kind]
    return hip.unet_src(k, *dev), dev  # (dev keeps the tensors alive)


def _wgrad_oracle(restate, dZ, Cin, Cout, dtype):
    w = torch.zeros(Cout, Cin, 3, 3, dtype=dtype, requires_grad=True)
    z = F.conv2d(restate(dtype), w, padding=1)
    z.backward(_planar(dZ.to(dtype)))
    return w.grad


# (name, kind, B, H, W, Cin, Cout, low size, C1)
WGRAD_CASES = [
    ("one tile", "rows", 1, 4, 8, 8, 4, None, None),
    ("edge tiles in both axes, 2 x 2 channel tiles", "rows", 3, 5, 9, 36, 36, None, None),
    ("planar first layer", "planar", 3, 13, 22, 7, 8, None, None),
    ("planar, one sample, one tile", "planar", 1, 4, 8, 7, 4, None, None),
    ("rows read channel by channel (Cin % 4 != 0)", "rows", 1, 5, 9, 6, 4, None, None),
    ("pool read channel by channel (Cin % 4 != 0)", "pool", 1, 5, 9, 6, 4, (11, 19), None),
    ("upcat read channel by channel (C1 % 4 != 0, C2 % 4 != 0)", "upcat", 1, 5, 9, 12, 4, (2, 4), 6),
    ("deep level from an odd pool source", "pool", 3, 1, 2, 8, 4, (3, 5), None),
    ("pool from an odd source, edge tiles", "pool", 1, 5, 9, 36, 8, (11, 19), None),
    ("pool to 13 x 22", "pool", 1, 13, 22, 8, 4, (26, 45), None),
    ("upcat, pad in h only, 64 + 32", "upcat", 1, 13, 22, 96, 68, (6, 11), 64),
    ("upcat, pad in w only", "upcat", 3, 6, 11, 12, 4, (3, 5), 8),
    ("upcat, no pad", "upcat", 1, 4, 8, 8, 36, (2, 4), 4),
    ("upcat from a single row", "upcat", 3, 3, 5, 16, 8, (1, 2), 8),
    ("long Cin at the deep level", "rows", 3, 1, 2, 260, 4, None, None),
    ("Cout 68, three channel tiles", "rows", 1, 5, 9, 8, 68, None, None),
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_wgrad(case):
    hip = _hip()
    name, kind, B, H, W, Cin, Cout, low, C1 = case
    tensors, restate = _source(kind, B, H, W, Cin, 7 + H * W + Cin, low, C1)
    dZ = torch.randn(B, H, W, Cout, generator=_gen(Cin + Cout))
    w64, w32 = _wgrad_oracle(restate, dZ, Cin, Cout, torch.float64), _wgrad_oracle(restate, dZ, Cin, Cout, torch.float32)
    src, keep = _descriptor(hip, kind, tensors)
    dZd = dZ.to(DEV)
    dW = hip.unet_conv3x3_wgrad(src, dZd, Cin)
    UC.check(dW, w64, w32, f"wgrad {name}")
    # a poisoned workspace of exactly the queried size does not reach dW, and two calls give equal bits
    ws = torch.full((hip.unet_wgrad_ws_bytes(B, H, W, Cin, Cout) // 4,), float("nan"), device=DEV)
    dW2 = hip.unet_conv3x3_wgrad(src, dZd, Cin, ws=ws)
    assert same_bits(dW, dW2)


# The pixel split: NT = B * ceil(H / 4) * ceil(W / 8) pixel tiles go into min(ceil(1024 / pairs), 256, NT) chunks at the
# most, pairs = ceil(Cout / 32) * ceil(Cin / 32); tiles per chunk = ceil(NT / that), chunks = ceil(NT / tiles per chunk).
# (name, B, H, W, Cin, Cout, expected chunks)
SPLIT_CASES = [
    ("NT = 256: the cap of 256 chunks, one tile each", 8, 16, 64, 8, 4, 256),
    ("NT = 257: past the cap, two tiles a chunk, every chunk spans two samples, the last holds one tile", 257, 4, 8, 8, 4, 129),
    ("27 channel-tile pairs: ceil(1024 / 27) = 38 < NT = 48, two tiles a chunk", 4, 13, 22, 260, 68, 24),
    ("one pair, NT = 48: below both caps, one tile a chunk", 4, 13, 22, 8, 4, 48),
    ("NT = 6: fewer tiles than the chunks wanted, one tile each", 3, 4, 16, 8, 4, 6),
]


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_wgrad_pixel_split(case):
    hip = _hip()
    name, B, H, W, Cin, Cout, chunks = case
    assert hip.unet_wgrad_chunks(B, H, W, Cin, Cout) == chunks, "the case no longer sits where its name says"
    assert hip.unet_wgrad_ws_bytes(B, H, W, Cin, Cout) == chunks * Cout * Cin * 9 * 4
    tensors, restate = _source("rows", B, H, W, Cin, 31 + B, None, None)
    dZ = torch.randn(B, H, W, Cout, generator=_gen(5 * B + Cout))
    w64, w32 = _wgrad_oracle(restate, dZ, Cin, Cout, torch.float64), _wgrad_oracle(restate, dZ, Cin, Cout, torch.float32)
    src, keep = _descriptor(hip, "rows", tensors)
    ws = torch.full((chunks * Cout * Cin * 9,), float("nan"), device=DEV)
    dW = hip.unet_conv3x3_wgrad(src, dZ.to(DEV), Cin, ws=ws)
    UC.check(dW, w64, w32, f"wgrad split: {name}")
    assert same_bits(dW, hip.unet_conv3x3_wgrad(src, dZ.to(DEV), Cin))


# ---------------------------------------------------------------------------------------------------------------------
# Data gradient: the pack plus the forward convolution
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(4, 8), (5, 9), (1, 2)])
@pytest.mark.parametrize("chan", [(8, 4), (36, 36), (96, 32), (8, 260)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_dgrad_pack_and_convolution(chan, size):
    """(8, 260): the data gradient contracts over 260 channels and takes the 8-wave side of the forward kernel."""
    hip = _hip()
    (Cin, Cout), (H, W), B = chan, size, 2
    g = _gen(Cin * Cout + H)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (1.5 / (9 * Cin) ** 0.5)
    dZ = torch.randn(B, H, W, Cout, generator=g)

    def oracle(dt):
        x = torch.zeros(B, Cin, H, W, dtype=dt, requires_grad=True)
        F.conv2d(x, w.to(dt), padding=1).backward(_planar(dZ.to(dt)))
        return _rows(x.grad)

    packed = hip.unet_pack_weights_dgrad(w.to(DEV))
    dX = torch.empty(B, H, W, Cin, device=DEV)
    hip.unet_conv3x3(hip.unet_src(hip.UNET_ROWS, dZ.to(DEV)), packed, None, EPS, dX, Cout)
    UC.check(dX, oracle(torch.float64), oracle(torch.float32), f"dgrad {Cin}->{Cout} at {H}x{W}")


# ---------------------------------------------------------------------------------------------------------------------
# Routing the data gradient: pool and upsample
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip_kind", ["none", "strided"])
@pytest.mark.parametrize("C", [4, 36])
def test_pool_bwd_is_torch_cpu_bit_for_bit(C, skip_kind):
    hip = _hip()
    B, Hs, Ws = 2, 5, 7  # odd: the last row and column are dropped by the pool
    g = _gen(C)
    act = torch.randn(B, Hs, Ws, C, generator=g)
    act[0, 0:2, 0:2, :] = 0.5                      # a window of four equal values: the first wins
    act[0, 0, 2, 0], act[0, 1, 3, 0] = 2.0, 2.0    # two equal maxima: the earlier in row-major order wins
    act[1, 2, 2, 1] = float("nan")                 # one NaN: it wins
    act[1, 0, 4, 2], act[1, 1, 5, 2] = float("nan"), float("nan")  # two NaNs: the later wins
    dP = torch.randn(B, Hs // 2, Ws // 2, C, generator=g)
    wide = torch.randn(B, Hs, Ws, C + 8, generator=g)
    leaf = _planar(act).contiguous().requires_grad_(True)
    F.max_pool2d(leaf, 2).backward(_planar(dP).contiguous())
    want = _rows(leaf.grad)
    skip = None
    if skip_kind == "strided":
        want = wide[..., :C] + want
        skip = wide.to(DEV)[..., :C]
    dA = torch.full((B, Hs, Ws, C), float("nan"), device=DEV)
    hip.unet_pool_bwd(act.to(DEV), dP.to(DEV), dA, skip=skip)
    assert same_bits(dA.cpu(), want)


@pytest.mark.parametrize("C", [4, 36])
@pytest.mark.parametrize("sizes", [((1, 2), (3, 5)), ((3, 5), (6, 11)), ((6, 11), (13, 22)), ((2, 3), (4, 6))],
                         ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_upsample_bwd(sizes, C):
    hip = _hip()
    (Hs, Ws), (H, W), B, C1 = sizes[0], sizes[1], 2, 8
    d = torch.randn(B, H, W, C1 + C, generator=_gen(H * W + C))

    def oracle(dt):
        low = torch.zeros(B, C, Hs, Ws, dtype=dt, requires_grad=True)
        up = F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True)
        F.pad(up, [0, W - up.shape[3], 0, H - up.shape[2]]).backward(_planar(d[..., C1:].to(dt)))
        return _rows(low.grad)

    dlow = torch.full((B, Hs, Ws, C), float("nan"), device=DEV)
    hip.unet_upsample_bwd(d.to(DEV), C1, dlow)
    UC.check(dlow, oracle(torch.float64), oracle(torch.float32), f"upsample_bwd {Hs}x{Ws} -> {H}x{W} C={C}")


@pytest.mark.parametrize("F_", [8, 64])
@pytest.mark.parametrize("Cout", [3, 19])
def test_conv1x1_out_bwd(Cout, F_):
    hip = _hip()
    B, H, W = 2, 5, 9
    g = _gen(Cout * F_)
    a, w = torch.randn(B, H, W, F_, generator=g), torch.randn(Cout, F_, generator=g) * (1.0 / F_ ** 0.5)
    dY = torch.randn(B, Cout, H, W, generator=g)

    def oracle(dt):
        al, wl = _planar(a.to(dt)).clone().requires_grad_(True), w.to(dt).view(Cout, F_, 1, 1).clone().requires_grad_(True)
        bl = torch.zeros(Cout, dtype=dt, requires_grad=True)
        F.conv2d(al, wl, bl).backward(dY.to(dt))
        return _rows(al.grad), wl.grad.view(Cout, F_), bl.grad

    o64, o32 = oracle(torch.float64), oracle(torch.float32)
    dA = torch.empty(B, H, W, F_, device=DEV)
    got = hip.unet_conv1x1_out_bwd(dY.to(DEV), a.to(DEV), w.to(DEV), dA)
    for name, t, t64, t32 in zip(("dA", "dW", "db"), got, o64, o32):
        UC.check(t, t64, t32, f"conv1x1_out_bwd Cout={Cout} F={F_} {name}")
    again = hip.unet_conv1x1_out_bwd(dY.to(DEV), a.to(DEV), w.to(DEV), torch.empty_like(dA))
    assert all(same_bits(p, q) for p, q in zip(got, again))


def test_launch_counter_is_its_own():
    """The training kernels count their launches apart from gcl_unet_launches."""
    hip = _hip()
    z = torch.randn(8, 4, device=DEV)
    fwd, trn = hip.unet_launches(), hip.unet_train_launches()
    hip.unet_bn_stats(z, EPS, MOM, torch.empty(4, device=DEV), torch.empty(4, device=DEV))
    assert hip.unet_launches() == fwd and hip.unet_train_launches() == trn + 2
