"""Generate the per-grid-point error-map fixtures by RUNNING the reference's own `scripts/metrics_maps.py` helpers
(`unit_label`, `inverse_standardize`, `apply_units`, `compute_stat`, `plot_field`; torch, numpy, matplotlib).

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_maps_golden.py

Output (data only - arrays, no reference source text): tests/golden/maps_vectors.npz
  unit_*          the eight variable names of the case and the reference's (label, factor, offset, special) of each
                  (special "" for None)
  y_mean/y_scale  realistic scaler statistics per channel
  all_t / all_p   standardised truth and prediction [N 6, G 32 x 16, leads 2 x C 8] (multiples of
                  1 / 32: fp16-representable, as the data sets hold them); channel 7 is constant in the truth
  all_conv_t/_p   inverse_standardize + apply_units of every lead slice and channel (float32): the unit conversion
  all_ref_<stat>  the reference's float32 compute_stat per lead slice and channel, [leads, G, C]
  all_x64_<stat>  the same statistics restated here in float64 from the converted float32 values (float64 differences,
                  float64 field means and unbiased standard deviations, 1e-8 added to the standard deviation): the
                  arbiter between two float32 results
  reg_rows        region_node_indices of a box; reg_ref_<stat> / reg_x64_<stat>: the same statistics over those rows only
                  ([leads, len(rows), C]; the inputs are the rows of the `all` case)
  grid_field / grid_out   a field [G] and the 2-D array plot_field hands to imshow for it
This generator asserts that its numpy restatement of the conversion (multiply, add, true division by float32 g0,
multiply, add; each rounded to float32) is bit-equal to the reference's.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (where the reference checkout lives; inert placeholders for absent modules)

REF = make_golden.REF
NAMES = ["t2m", "10u", "msl", "tp", "z@500", "q@850", "lsm", "t@850"]
Y_MEAN = np.array([278.4, -0.05, 100950.0, 5.1e-4, 54150.0, 4.6e-3, 0.34, 274.6])
Y_SCALE = np.array([21.3, 5.6, 1330.0, 1.6e-3, 3340.0, 4.1e-3, 0.46, 15.7])
STATS = ("rmse", "mae", "bias", "acc")
N, NLON, NLAT, LEADS = 6, 32, 16, 2
BOX = (20.0, 70.0, 60.0, 150.0)


def _script(name):
    spec = importlib.util.spec_from_file_location(f"_ref_{name}", os.path.join(REF, "scripts", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _restated_conversion(x, c, mm):
    """The conversion of channel c in numpy float32, operation by operation."""
    _, factor, offset, special = mm.unit_label(NAMES[c])
    v = x.astype(np.float32) * np.float32(Y_SCALE[c])
    v = v + np.float32(Y_MEAN[c])
    if special == "z_to_m":
        v = v / np.float32(9.80665)
    v = v * np.float32(factor)
    return v + np.float32(offset)


def _x64(stat, p, t):
    """compute_stat in float64 from converted float32 values p, t [N, rows]."""
    p, t = p.astype(np.float64), t.astype(np.float64)
    e = p - t
    if stat == "rmse":
        return np.sqrt(np.mean(e * e, axis=0))
    if stat == "mae":
        return np.mean(np.abs(e), axis=0)
    if stat == "bias":
        return np.mean(e, axis=0)
    ph = (p - p.mean(axis=1, keepdims=True)) / (p.std(axis=1, ddof=1, keepdims=True) + 1e-8)
    th = (t - t.mean(axis=1, keepdims=True)) / (t.std(axis=1, ddof=1, keepdims=True) + 1e-8)
    return np.mean(ph * th, axis=0)


def _maps(mm, conv_p, conv_t, rows, C):
    """ref_<stat> (the reference, float32) and x64_<stat> over the given rows, [leads, len(rows), C]."""
    out = {}
    for stat in STATS:
        ref = np.empty((LEADS, len(rows), C), dtype=np.float32)
        x64 = np.empty((LEADS, len(rows), C), dtype=np.float64)
        for lead in range(LEADS):
            for c in range(C):
                p, t = conv_p[:, rows, lead * C + c], conv_t[:, rows, lead * C + c]
                ref[lead, :, c] = mm.compute_stat(torch.from_numpy(p.copy()), torch.from_numpy(t.copy()), stat).numpy()
                x64[lead, :, c] = _x64(stat, p, t)
        out[f"ref_{stat}"], out[f"x64_{stat}"] = ref, x64
    return out


def main():
    make_golden._placeholders()
    sys.path.insert(0, REF)
    import matplotlib
    matplotlib.use("Agg")
    mm, pr = _script("metrics_maps"), _script("predict")
    out = {}
    C, G = len(NAMES), NLON * NLAT

    labels = [mm.unit_label(n) for n in NAMES]
    out["unit_names"] = np.array(NAMES)
    out["unit_label"] = np.array([u[0] for u in labels])
    out["unit_factor"] = np.array([u[1] for u in labels], dtype=np.float64)
    out["unit_offset"] = np.array([u[2] for u in labels], dtype=np.float64)
    out["unit_special"] = np.array([u[3] or "" for u in labels])
    out["y_mean"], out["y_scale"] = Y_MEAN, Y_SCALE

    rng = np.random.RandomState(314)
    t = rng.randn(N, G, LEADS * C)
    p = t + 0.3 * rng.randn(N, G, LEADS * C) + 0.05 * rng.randn(1, G, LEADS * C)
    t[:, :, C - 1::C] = 0.25  # the last channel is constant in the truth
    t = (np.round(t * 32.0) / 32.0).astype(np.float32)  # steps of 1 / 32: exact in fp16, and the file stays small
    p = (np.round(p * 32.0) / 32.0).astype(np.float32)
    out["all_t"], out["all_p"] = t, p

    conv_t, conv_p = np.empty_like(t), np.empty_like(p)
    for src, dst in ((t, conv_t), (p, conv_p)):
        for lead in range(LEADS):
            phys = mm.inverse_standardize(torch.from_numpy(src[:, :, lead * C:(lead + 1) * C].copy()), Y_MEAN, Y_SCALE)
            for c in range(C):
                conv, label = mm.apply_units(phys[..., c], NAMES[c])
                assert label == labels[c][0]
                dst[:, :, lead * C + c] = conv.numpy()
                mine = _restated_conversion(src[:, :, lead * C + c], c, mm)
                assert np.array_equal(mine, dst[:, :, lead * C + c]), f"conversion of {NAMES[c]} is not bit-equal"
    out["all_conv_t"], out["all_conv_p"] = conv_t, conv_p

    for k, v in _maps(mm, conv_p, conv_t, np.arange(G), C).items():
        out[f"all_{k}"] = v
    lats, lons = pr.linspace_lats_lons(NLAT, NLON)
    rows = pr.region_node_indices(*BOX, lats, lons)
    assert 8 <= len(rows) < G
    out["reg_rows"] = rows
    for k, v in _maps(mm, conv_p, conv_t, rows, C).items():
        out[f"reg_{k}"] = v

    # what plot_field hands to imshow
    seen = []

    class _Plt:
        def __getattr__(self, name):
            def call(*a, **k):
                if name == "imshow":
                    seen.append(np.array(a[0]))
            return call
    field = out["all_ref_rmse"][0, :, 0]
    mm.plt = _Plt()
    mm.plot_field(torch.from_numpy(field.copy()), NLON, NLAT, "title", "unused.png")
    assert len(seen) == 1 and seen[0].shape == (NLAT, NLON)
    out["grid_field"], out["grid_out"] = field, seen[0]
    out["grid_shape"] = np.array([NLON, NLAT], dtype=np.int64)

    for v in out.values():
        assert isinstance(v, np.ndarray) and v.dtype != object
    path = os.path.join(HERE, "maps_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
