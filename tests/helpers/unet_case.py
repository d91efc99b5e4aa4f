"""The WeatherUNet test case: the fixture of tests/golden/make_unet_golden.py, a functional restatement of the network
from a state dict (the oracle of the unet tests, float64 on the CPU), random state dicts with non-trivial BatchNorm
statistics, and the suite's error rule for this network."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "unet_vectors.npz")
IN, OUT, BASE, B, H, W = 7, 3, 8, 2, 13, 22
SEED = 4321
FLOOR = 2.0 ** -20  # 16 ulp of the largest output: layers so small that the CPU float32 result happens to be exact

BLOCKS = ("inc.net", "down1.net.1.net", "down2.net.1.net", "down3.net.1.net", "up1.conv.net", "up2.conv.net", "up3.conv.net")


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_state(g=None, dtype=torch.float32):
    g = golden() if g is None else g
    sd = {}
    for k in [str(s) for s in g["keys"]]:
        t = torch.from_numpy(g["sd_" + k])
        sd[k] = t if t.dtype == torch.int64 else t.to(dtype)
    return sd


def randomise_(model, seed):
    """Random weights with non-trivial BatchNorm statistics and affine parameters, in place: fresh ones (0, 1, 1, 0) hide
    every mistake of the epilogue."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("num_batches_tracked"):
                t.fill_(7)
            elif name.endswith("running_var"):
                t.copy_(0.5 + torch.rand(t.shape, generator=g))
            elif name.endswith("running_mean"):
                t.copy_(0.3 * torch.randn(t.shape, generator=g))
            elif t.dim() == 1 and name.endswith("weight"):  # BatchNorm gamma
                t.copy_(0.75 + 0.5 * torch.rand(t.shape, generator=g))
            elif t.dim() == 1:  # BatchNorm beta, the output bias
                t.copy_(0.2 * torch.randn(t.shape, generator=g))
            else:  # convolution weights: outputs of order one
                fan = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g) * (1.5 / fan ** 0.5))
    return model


def double_conv(sd, p, x):
    for c, n in ((0, 1), (3, 4)):
        x = F.conv2d(x, sd[f"{p}.{c}.weight"], padding=1)
        x = F.batch_norm(x, sd[f"{p}.{n}.running_mean"], sd[f"{p}.{n}.running_var"], sd[f"{p}.{n}.weight"],
                         sd[f"{p}.{n}.bias"], training=False, eps=1e-5)
        x = F.gelu(x)
    return x


def up(sd, p, x, skip):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    dh, dw = skip.shape[2] - x.shape[2], skip.shape[3] - x.shape[3]
    if dh > 0 or dw > 0:
        x = F.pad(x, [0, dw, 0, dh])
    return double_conv(sd, p, torch.cat([skip, x], dim=1))


def functional_unet(sd, x, residual_from=None):
    """model.py:87-98 from a state dict, in the dtype of x (the state dict's floating tensors are cast to it)."""
    sd = {k: (v.to(x.dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    x1 = double_conv(sd, BLOCKS[0], x)
    x2 = double_conv(sd, BLOCKS[1], F.max_pool2d(x1, 2))
    x3 = double_conv(sd, BLOCKS[2], F.max_pool2d(x2, 2))
    x4 = double_conv(sd, BLOCKS[3], F.max_pool2d(x3, 2))
    u = up(sd, BLOCKS[4], x4, x3)
    u = up(sd, BLOCKS[5], u, x2)
    u = up(sd, BLOCKS[6], u, x1)
    y = F.conv2d(u, sd["out_conv.weight"], sd["out_conv.bias"])
    if residual_from is not None:
        y = x[:, residual_from[0]:residual_from[1]] + y
    return y


def E(y, y64):
    """max |y - y64| / max |y64|."""
    y, y64 = torch.as_tensor(y).double().cpu(), torch.as_tensor(y64).double().cpu()
    return float((y - y64).abs().max() / y64.abs().max())


def check(got, y64, y32, what):
    """e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20); prints the figures first."""
    e_hip, e_cpu = E(got, y64), E(y32, y64)
    bound = max(4.0 * e_cpu, FLOOR)
    print(f"[unet] {what}: e(hip) = {e_hip:.3e}, e(cpu32) = {e_cpu:.3e}, ratio = {e_hip / max(e_cpu, 1e-300):.3f}, "
          f"bound = {bound:.3e}")
    assert e_hip <= bound, f"{what}: e(hip) = {e_hip:.3e} above max(4 * {e_cpu:.3e}, 2^-20)"
    return e_hip, e_cpu
