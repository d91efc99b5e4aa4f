"""Generate the WeatherUNet training fixture by RUNNING the reference's own `WeatherUNet` (src/unet/model.py) in
`.train()` with CPU torch.

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_unet_train_golden.py

The case is tests/helpers/unet_train_case.py: the state of tests/golden/unet_vectors.npz (in = 7, out = 3,
base_filters = 8, random weights and BatchNorm statistics), B = 2, H x W = 16 x 24 - 12 values per channel at the deepest
level, so that BatchNorm's backward is well conditioned.  One forward in training mode and one backward with a random
upstream gradient.  Output (data only): tests/golden/unet_train_vectors.npz

    keys            the state dict's key list, in order
    x               the input, float32 [2, 7, 16, 24], standard normal
    go              the upstream gradient d loss / d y, float32 [2, 3, 16, 24], standard normal
    y               the reference module's output in training mode
    grad_<key>      the gradient of each of the 44 parameters
    buf_<key>       each of the 28 float buffers (running_mean, running_var) after the step
    nbt             num_batches_tracked after the step (8 everywhere)

The generator also asserts that the float32 functional restatement of unet_train_case gives the module's gradients and
buffers bit for bit and that the float64 one lies within 2^-15 of them.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden  # noqa: E402  (where the reference checkout lives)
import unet_case as UC  # noqa: E402
import unet_train_case as TC  # noqa: E402

REF = make_golden.REF


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    spec = importlib.util.spec_from_file_location("_ref_unet_model", os.path.join(REF, "src", "unet", "model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    sd = UC.golden_state()
    model = M.WeatherUNet(TC.IN, TC.OUT, TC.BASE)
    model.load_state_dict(sd, strict=True)
    model.train()
    gen = torch.Generator().manual_seed(TC.SEED)
    x = torch.randn(TC.B, TC.IN, TC.H, TC.W, generator=gen)
    go = torch.randn(TC.B, TC.OUT, TC.H, TC.W, generator=gen)
    y = model(x)
    y.backward(go)
    after = model.state_dict()
    res = {"keys": np.array(list(sd.keys())), "x": x.numpy(), "go": go.numpy(), "y": y.detach().numpy()}
    for k, p in model.named_parameters():
        res["grad_" + k] = p.grad.numpy()
    nbt = set()
    for k, v in after.items():
        if TC.is_float_buffer(k):
            res["buf_" + k] = v.numpy()
        elif k.endswith("num_batches_tracked"):
            nbt.add(int(v))
    assert nbt == {8}, nbt
    res["nbt"] = np.int64(8)

    y32, g32, b32 = TC.train_step(sd, x, go, torch.float32)
    y64, g64, b64 = TC.train_step(sd, x, go, torch.float64)
    assert torch.equal(y32, y.detach())
    worst = 0.0
    for k, g in g32.items():
        assert torch.equal(g, torch.from_numpy(res["grad_" + k])), k
        worst = max(worst, UC.E(res["grad_" + k], g64[k]))
    for k, b in b32.items():
        assert torch.equal(b, torch.from_numpy(res["buf_" + k])), k
        worst = max(worst, UC.E(res["buf_" + k], b64[k]))
    assert worst < 2.0 ** -15, worst
    np.savez(TC.GOLDEN, **res)
    print(f"wrote {TC.GOLDEN} ({os.path.getsize(TC.GOLDEN) / 1e3:.1f} kB, {len(res)} arrays); worst E vs float64 = {worst:.3e}")


if __name__ == "__main__":
    main()
