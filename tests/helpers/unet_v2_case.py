"""The WeatherUNetV2 test case: the fixture of tests/golden/make_unet_v2_golden.py, a functional restatement of the network
from a state dict (the oracle of the unet_v2 tests, float64 on the CPU), random state dicts in which every new branch
carries weight, and the suite's error rule for the U-Nets (unet_case.E / check / FLOOR).

In float64 the restatement's spectral layer works in complex128.  The reference module cast to double still rounds its
spectral buffer to cfloat (model_v2.py:115-116), so it is no float64 oracle; the restatement keeps the dtype of x."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from unet_case import FLOOR, E, check  # noqa: F401  (the one error rule of the U-Net tests)

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "unet_v2_vectors.npz")
IN, OUT, BASE, HEADS, MODES, B, H, W = 6, 3, 4, 4, 4, 2, 27, 45
SEED = 8642
GN_EPS = LN_EPS = 1e-5  # torch's defaults, which the reference keeps


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_state(g=None, dtype=torch.float32):
    g = golden() if g is None else g
    return {k: torch.from_numpy(g["sd_" + k]).to(dtype) for k in [str(s) for s in g["keys"]]}


def randomise_(model, seed):
    """Random weights, in place, such that every branch carries weight: non-trivial GroupNorm / LayerNorm affine vectors,
    SE biases of order one, spectral weights of standard deviation Cin^-1/2 (the default 1 / (Cin Cout) makes the branch
    invisible), convolution and linear weights that keep activations of order one."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            r = torch.randn(t.shape, generator=g)
            if "weights_re" in name or "weights_im" in name:
                t.copy_(r * t.shape[0] ** -0.5)
            elif ".se.fc." in name and t.dim() == 1:  # SE biases
                t.copy_(r)
            elif t.dim() == 1 and name.endswith("weight"):  # GroupNorm / LayerNorm gamma
                t.copy_(0.75 + 0.5 * torch.rand(t.shape, generator=g))
            elif t.dim() == 1:  # GroupNorm / LayerNorm beta, the projection's and the output's bias
                t.copy_(0.2 * r)
            elif t.dim() == 2:  # linears
                t.copy_(r * (1.5 / t.shape[1] ** 0.5))
            else:  # convolutions
                fan = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(r * (1.5 / fan ** 0.5))
    return model


def groups_of(C):
    g = min(8, C)
    while C % g != 0 and g > 1:
        g -= 1
    return g


def res_block(sd, p, x):
    """model_v2.py:59-60 and 35-37."""
    C = sd[f"{p}.conv.0.weight"].shape[0]
    g = groups_of(C)
    u = x
    for c, n in ((0, 1), (3, 4)):
        u = F.conv2d(u, sd[f"{p}.conv.{c}.weight"], padding=1)
        u = F.gelu(F.group_norm(u, g, sd[f"{p}.conv.{n}.weight"], sd[f"{p}.conv.{n}.bias"], eps=GN_EPS))
    u = u + (F.conv2d(x, sd[f"{p}.skip.weight"]) if f"{p}.skip.weight" in sd else x)
    m = u.mean(dim=(2, 3))
    hid = F.gelu(F.linear(m, sd[f"{p}.se.fc.2.weight"], sd[f"{p}.se.fc.2.bias"]))
    gate = torch.sigmoid(F.linear(hid, sd[f"{p}.se.fc.4.weight"], sd[f"{p}.se.fc.4.bias"]))
    return u * gate[:, :, None, None]


def attention(sd, p, x, heads):
    """model_v2.py:74-92; the residual goes on the normalised tokens."""
    Bn, C, Hh, Ww = x.shape
    t = x.flatten(2).transpose(1, 2)
    t = F.layer_norm(t, (C,), sd[f"{p}.norm.weight"], sd[f"{p}.norm.bias"], eps=LN_EPS)
    qkv = F.linear(t, sd[f"{p}.qkv.weight"]).reshape(Bn, Hh * Ww, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    a = ((q @ k.transpose(-2, -1)) * (C // heads) ** -0.5).softmax(dim=-1)
    out = F.linear((a @ v).transpose(1, 2).reshape(Bn, Hh * Ww, C), sd[f"{p}.proj.weight"], sd[f"{p}.proj.bias"])
    return (t + out).transpose(1, 2).reshape(Bn, C, Hh, Ww)


def spectral(w_re, w_im, x, modes_h, modes_w):
    """model_v2.py:106-122 with the complex buffer in the precision of x (complex128 for float64)."""
    Bn, _, Hh, Ww = x.shape
    x_ft = torch.fft.rfft2(x, norm="ortho")
    mh, mw = min(modes_h, Hh), min(modes_w, x_ft.shape[-1])
    out_ft = torch.zeros(Bn, w_re.shape[1], Hh, x_ft.shape[-1], dtype=x_ft.dtype, device=x.device)
    w = torch.complex(w_re[:, :, :mh, :mw], w_im[:, :, :mh, :mw])
    out_ft[:, :, :mh, :mw] = torch.einsum("bihw,iohw->bohw", x_ft[:, :, :mh, :mw], w)
    return torch.fft.irfft2(out_ft, s=(Hh, Ww), norm="ortho")


def up(sd, p, x, skip):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dh, dw = skip.shape[2] - x.shape[2], skip.shape[3] - x.shape[3]
    if dh > 0 or dw > 0:
        x = F.pad(x, [0, dw, 0, dh])
    return res_block(sd, p, torch.cat([skip, x], dim=1))


def functional_unet_v2(sd, x, heads, modes, residual_from=None):
    """model_v2.py:205-220 from a state dict, in the dtype of x (the state dict's tensors are cast to it)."""
    sd = {k: v.to(x.dtype) for k, v in sd.items()}
    x1 = res_block(sd, "inc", x)
    x2 = res_block(sd, "down1.conv", F.max_pool2d(x1, 2))
    x3 = res_block(sd, "down2.conv", F.max_pool2d(x2, 2))
    x4 = res_block(sd, "down3.conv", F.max_pool2d(x3, 2))
    b_attn = attention(sd, "bottleneck_attn", x4, heads)
    b_spec = spectral(sd["bottleneck_spectral.weights_re"], sd["bottleneck_spectral.weights_im"], x4, modes, modes)
    b = res_block(sd, "bottleneck_mix", torch.cat([b_attn, b_spec], dim=1))
    u = up(sd, "up1.conv", b, x3)
    u = up(sd, "up2.conv", u, x2)
    u = up(sd, "up3.conv", u, x1)
    y = F.conv2d(u, sd["out_conv.weight"], sd["out_conv.bias"])
    if residual_from is not None:
        y = x[:, residual_from[0]:residual_from[1]] + y
    return y
