"""Generate the WeatherUNetV2 fixture by RUNNING the reference's own `WeatherUNetV2` (src/unet/model_v2.py) with CPU torch.

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_unet_v2_golden.py

The case is tests/helpers/unet_v2_case.py: in = 6, out = 3, base_filters = 4, heads 4, modes 4, B = 2, H x W = 27 x 45.
Levels 27x45, 13x22, 6x11, 3x5: every pool drops a row or a column, the pads occur in w only, in h only and in both, the
bottleneck has 15 tokens and an odd Wb with mh = mw = 3.  The weights are random (unet_v2_case.randomise_, seed
unet_v2_case.SEED) so that every branch carries weight.  Output (data only): tests/golden/unet_v2_vectors.npz

    keys            the state dict's key list, in order
    sd_<key>        the state dict's arrays (float32)
    x               the input, float32 [2, 6, 27, 45], standard normal
    y               the reference module's output in eval mode, float32 [2, 3, 27, 45]
    num_params      the reference's num_params

The generator also asserts that the float64 functional restatement of unet_v2_case reproduces the reference's y to
E < 2^-18, here and (without storing them) at base_filters 8 and 12 on 13 x 22, 41 x 61 and 32 x 48.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import make_golden  # noqa: E402  (where the reference checkout lives)
import unet_v2_case as VC  # noqa: E402

REF = make_golden.REF


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    spec = importlib.util.spec_from_file_location("_ref_unet_model_v2", os.path.join(REF, "src", "unet", "model_v2.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    torch.manual_seed(0)
    model = VC.randomise_(M.WeatherUNetV2(VC.IN, VC.OUT, VC.BASE, VC.HEADS, VC.MODES), VC.SEED).eval()
    x = torch.randn(VC.B, VC.IN, VC.H, VC.W, generator=torch.Generator().manual_seed(VC.SEED + 1))
    with torch.no_grad():
        y = model(x)
    sd = model.state_dict()
    res = {"keys": np.array(list(sd.keys())), "x": x.numpy(), "y": y.numpy(), "num_params": np.int64(model.num_params)}
    for k, v in sd.items():
        res["sd_" + k] = v.numpy()
    e = VC.E(y, VC.functional_unet_v2(sd, x.double(), VC.HEADS, VC.MODES))
    assert e < 2.0 ** -18, f"the functional restatement misses the reference's output by E = {e:.3e}"
    for f in (8, 12):
        for (h, w) in ((13, 22), (41, 61), (32, 48)):
            m2 = VC.randomise_(M.WeatherUNetV2(VC.IN, VC.OUT, f, 4, 4), VC.SEED + f).eval()
            x2 = torch.randn(1, VC.IN, h, w, generator=torch.Generator().manual_seed(VC.SEED + h))
            with torch.no_grad():
                y2 = m2(x2)
            e2 = VC.E(y2, VC.functional_unet_v2(m2.state_dict(), x2.double(), 4, 4))
            print(f"base_filters {f}, {h} x {w}: E(reference float32, float64 restatement) = {e2:.3e}")
            assert e2 < 2.0 ** -18, f"base_filters {f}, {h} x {w}: the restatement misses the reference by E = {e2:.3e}"
    np.savez(VC.GOLDEN, **res)
    print(f"wrote {VC.GOLDEN} ({os.path.getsize(VC.GOLDEN) / 1e3:.1f} kB, {len(res)} arrays); E(y32, y64) = {e:.3e}")


if __name__ == "__main__":
    main()
