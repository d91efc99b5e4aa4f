"""Generate the WeatherUNet fixture by RUNNING the reference's own `WeatherUNet` (src/unet/model.py) with CPU torch.

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_unet_golden.py

The case is tests/helpers/unet_case.py: in = 7, out = 3, base_filters = 8, B = 2, H x W = 13 x 22 - every branch of the
network occurs at it (levels 13x22, 6x11, 3x5, 1x2: pools that drop a row or a column, an upsampling from a single row,
pads in h only, in w only and none, concatenated widths 96, 48, 24).  The weights and the BatchNorm statistics and affine
parameters are random (unet_case.randomise_, seed unet_case.SEED): fresh statistics (0, 1, 1, 0) hide every mistake of
the epilogue.  Output (data only): tests/golden/unet_vectors.npz

    keys            the state dict's key list, in order
    sd_<key>        the state dict's arrays (float32; num_batches_tracked int64)
    x               the input, float32 [2, 7, 13, 22], standard normal
    y               the reference module's output in eval mode, float32 [2, 3, 13, 22]
    num_params      the reference's num_params

The generator also asserts that the float64 functional restatement of unet_case reproduces y to float32 rounding.
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
import unet_case as UC  # noqa: E402

REF = make_golden.REF


def main():
    if not os.path.isdir(REF):
        raise SystemExit("reference tree not present; fixtures can only be regenerated in the build container")
    spec = importlib.util.spec_from_file_location("_ref_unet_model", os.path.join(REF, "src", "unet", "model.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    torch.manual_seed(0)
    model = UC.randomise_(M.WeatherUNet(UC.IN, UC.OUT, UC.BASE), UC.SEED).eval()
    x = torch.randn(UC.B, UC.IN, UC.H, UC.W, generator=torch.Generator().manual_seed(UC.SEED + 1))
    with torch.no_grad():
        y = model(x)
    sd = model.state_dict()
    res = {"keys": np.array(list(sd.keys())), "x": x.numpy(), "y": y.numpy(), "num_params": np.int64(model.num_params)}
    for k, v in sd.items():
        res["sd_" + k] = v.numpy()
    y64 = UC.functional_unet(sd, x.double())
    e = UC.E(y, y64)
    assert e < 2.0 ** -18, f"the functional restatement misses the reference's output by E = {e:.3e}"
    np.savez(UC.GOLDEN, **res)
    print(f"wrote {UC.GOLDEN} ({os.path.getsize(UC.GOLDEN) / 1e3:.1f} kB, {len(res)} arrays); E(y32, y64) = {e:.3e}")


if __name__ == "__main__":
    main()
