"""The WeatherUNet training case: the fixture of tests/golden/make_unet_train_golden.py and a functional restatement of
the training forward (BatchNorm on batch statistics, running buffers updated on clones) from a state dict, with torch
autograd on the CPU - the oracle of the training tests in float64, the yardstick in float32.  The error rule is
unet_case's: per tensor, e(hip) <= max(4 e(torch CPU float32 on the same inputs), 2^-20)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unet_case as UC  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "unet_train_vectors.npz")
IN, OUT, BASE, B, H, W = UC.IN, UC.OUT, UC.BASE, 2, 16, 24
SEED = 8765
E, check, FLOOR = UC.E, UC.check, UC.FLOOR
FLOAT_BUFFERS = ("running_mean", "running_var")


def golden():
    return np.load(GOLDEN, allow_pickle=False)


def is_param(key):
    return not key.endswith(FLOAT_BUFFERS + ("num_batches_tracked",))


def is_float_buffer(key):
    return key.endswith(FLOAT_BUFFERS)


def train_forward(sd, x, dtype=None, state=None):
    """model.py:87-98 in .train() from a state dict, in `dtype` (default: x's).  Returns (y, params, buffers): params are
    leaf copies of the 44 parameters that require grad (y hangs on them), buffers the updated clones of the 28 float
    buffers.  The state dict itself is left unchanged.  state = (params, buffers) of an earlier call: these are used
    instead of sd (the buffers are updated in place), so that an optimizer can step the same leaves again and again."""
    dtype = x.dtype if dtype is None else dtype
    x = x.to(dtype)
    if state is not None:
        params, buffers = state
    else:
        params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items() if is_param(k)}
        buffers = {k: v.detach().to(dtype).clone() for k, v in sd.items() if is_float_buffer(k)}

    def double_conv(p, t):
        for c, n in ((0, 1), (3, 4)):
            t = F.conv2d(t, params[f"{p}.{c}.weight"], padding=1)
            t = F.batch_norm(t, buffers[f"{p}.{n}.running_mean"], buffers[f"{p}.{n}.running_var"], params[f"{p}.{n}.weight"],
                             params[f"{p}.{n}.bias"], training=True, momentum=0.1, eps=1e-5)
            t = F.gelu(t)
        return t

    def up(p, t, skip):
        t = F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
        dh, dw = skip.shape[2] - t.shape[2], skip.shape[3] - t.shape[3]
        if dh > 0 or dw > 0:
            t = F.pad(t, [0, dw, 0, dh])
        return double_conv(p, torch.cat([skip, t], dim=1))

    x1 = double_conv(UC.BLOCKS[0], x)
    x2 = double_conv(UC.BLOCKS[1], F.max_pool2d(x1, 2))
    x3 = double_conv(UC.BLOCKS[2], F.max_pool2d(x2, 2))
    x4 = double_conv(UC.BLOCKS[3], F.max_pool2d(x3, 2))
    u = up(UC.BLOCKS[4], x4, x3)
    u = up(UC.BLOCKS[5], u, x2)
    u = up(UC.BLOCKS[6], u, x1)
    y = F.conv2d(u, params["out_conv.weight"], params["out_conv.bias"])
    return y, params, buffers


def train_step(sd, x, go, dtype):
    """One forward and backward with the upstream gradient go: (y, {key: grad}, {key: updated float buffer})."""
    y, params, buffers = train_forward(sd, x, dtype)
    y.backward(go.to(dtype))
    return y.detach(), {k: p.grad for k, p in params.items()}, buffers


def random_state(seed, cin=IN, cout=OUT, base=BASE):
    """A random state dict with non-trivial BatchNorm statistics (unet_case.randomise_), from the project's own module
    tree (CPU, no kernels involved)."""
    from graphcast_lite_amd.unet import WeatherUNet

    return {k: v.clone() for k, v in UC.randomise_(WeatherUNet(cin, cout, base), seed).state_dict().items()}
