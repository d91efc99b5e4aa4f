"""Generate the data-assimilation fixtures by RUNNING the reference's own `src/assimilation/` (torch + numpy only).

Run from the repo root, only where the reference checkout (`make_golden.REF`) exists (never on the GPU box):

    python tests/golden/make_assim_golden.py

Output (data only - arrays, no reference source text): tests/golden/assim_vectors.npz
  helper_*      build_feature_mask, build_feature_mask_from_indices, cosine_taper_2d, build_boundary_taper_mask
  nudge_*       NudgingAssimilator.apply (with / without a feature mask, a mask of the wrong length, a shape mismatch)
                and nudge_sequence_offline on inputs with NaN and inf
  oifull_*      OptimalInterpolation.apply in float32 on the 64 x 32 grid with poles, full-grid mode: 4 channels, two
                sharing one station set, one with its own, one without observations
  oiroi_*       the same in ROI mode on the 512 x 256 grid (the DA-experiment box 50-60N x 83-98E, indices numbered the
                way scripts/predict.py numbers them, 10 % stations with seed 42).  Only the ROI rows are stored: the
                forecast is `oiroi_fill` elsewhere and the observations are NaN elsewhere.
  oidup_*       a flat grid with duplicated coordinates: the reference's nearest-node index for an observation at every
                node (argmin of _build_H), and OI apply on it
  *_x64         the same OI arithmetic in float64 (B built without the float32 rounding, default dtype float64), the
                arbiter between two float32 results
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (where the reference checkout lives)

REF = make_golden.REF

SIGMA_B, SIGMA_O = 0.8, 0.5
ROI_BOX = (50.0, 60.0, 83.0, 98.0)


def _oi_pair(OI, args, kwargs, forecast, obs):
    """(float32 result, float64 result) of the reference's OptimalInterpolation.apply."""
    oi = OI(*args, **kwargs)
    x32 = oi.apply(forecast.clone(), obs.clone()).numpy()
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        oi64 = OI(*args, **kwargs)
        d = oi64._dist_matrix(oi64._oi_coords, oi64._oi_coords)
        oi64.B = torch.from_numpy(oi64.sigma_b ** 2 * np.exp(-(d ** 2) / (oi64.L ** 2)))
        x64 = oi64.apply(forecast.double(), obs.double()).numpy()
    finally:
        torch.set_default_dtype(old)
    return x32, x64


def _region_rows(lat_min, lat_max, lon_min, lon_max, lats, lons):
    """Grid indices of a lat / lon box, numbered longitude-major (lon_index * num_lat + lat_index) as the reference's
    predict script numbers them."""
    li = np.where((lats >= lat_min) & (lats <= lat_max))[0]
    lj = np.where((lons >= lon_min) & (lons <= lon_max))[0]
    return (lj[:, None] * len(lats) + li[None, :]).ravel().astype(np.int64)


def main():
    sys.path.insert(0, REF)
    from src.assimilation import nudging as N
    from src.assimilation.optimal_interpolation import OptimalInterpolation as OI

    out = {}
    # ---- helpers
    feats = ["t2m", "u10", "v10", "msl", "tp"]
    out["helper_feature_mask"] = N.build_feature_mask(feats, ["u10", "tp", "nope"], 3, "cpu").numpy()
    out["helper_feature_mask_idx"] = N.build_feature_mask_from_indices([0, 3, 7, -1], 5, 2, "cpu").numpy()
    out["helper_taper"] = N.cosine_taper_2d(12, 9, 3).numpy()
    out["helper_taper_b0"] = N.cosine_taper_2d(4, 5, 0).numpy()
    out["helper_boundary"] = N.build_boundary_taper_mask(9, 12, 2, 3).numpy()

    # ---- nudging
    g = torch.Generator().manual_seed(7)
    f = torch.randn(2, 50, 7, generator=g)
    o = f + torch.randn(2, 50, 7, generator=g)
    o[torch.rand(2, 50, 7, generator=g) < 0.6] = float("nan")
    o[0, 3, 2], o[1, 4, 5], o[0, 9, 0] = float("inf"), float("-inf"), float("inf")
    mask7 = torch.tensor([1, 0, 1, 1, 0, 1, 0], dtype=torch.bool)
    out.update(nudge_f=f.numpy(), nudge_o=o.numpy(), nudge_mask=mask7.numpy())
    out["nudge_seq_masked"] = N.NudgingAssimilator(alpha=0.3, feature_mask_flat=mask7).apply(f[0], o[0]).numpy()
    out["nudge_seq"] = N.NudgingAssimilator(alpha=0.3).apply(f[1], o[1]).numpy()
    out["nudge_seq_badmask"] = N.NudgingAssimilator(alpha=0.3, feature_mask_flat=mask7[:5]).apply(f[0], o[0]).numpy()
    out["nudge_seq_mismatch"] = N.NudgingAssimilator(alpha=0.3).apply(f[0], o[0, :, :5]).numpy()
    out["nudge_offline"] = N.nudge_sequence_offline(f, o, alpha=0.37).numpy()

    # ---- OI, full grid 64 x 32 with poles
    lats = np.linspace(-90, 90, 32, endpoint=True)
    lons = np.linspace(0, 360, 64, endpoint=False)
    G, C = 32 * 64, 4
    rng = np.random.RandomState(11)
    xb = torch.from_numpy(rng.randn(G, C).astype(np.float32))
    truth = xb + torch.from_numpy(rng.randn(G, C).astype(np.float32))
    y = torch.full((G, C), float("nan"))
    s01 = np.sort(rng.choice(G, 100, replace=False))
    s01 = np.unique(np.concatenate([s01, [0, 5, G - 1, G - 3]]))  # stations at both poles
    s2 = np.sort(rng.choice(G, 60, replace=False))
    y[s01, 0], y[s01, 1], y[s2, 2] = truth[s01, 0], truth[s01, 1], truth[s2, 2]
    L_full = 1.2e6
    x32, x64 = _oi_pair(OI, (lats, lons, SIGMA_B, SIGMA_O, L_full, "cpu"), {}, xb, y)
    out.update(oifull_lats=lats, oifull_lons=lons, oifull_L=np.float64(L_full), oifull_xb=xb.numpy(),
               oifull_y=y.numpy(), oifull_x32=x32, oifull_x64=x64)

    # ---- OI, ROI mode on 512 x 256 (the DA-experiment box)
    lats = np.linspace(-90, 90, 256, endpoint=True)
    lons = np.linspace(0, 360, 512, endpoint=False)
    G, C = 256 * 512, 5
    roi = _region_rows(*ROI_BOX, lats, lons)
    st = np.sort(np.random.RandomState(42).choice(roi, max(1, int(len(roi) * 0.1)), replace=False))
    rng = np.random.RandomState(12)
    fill = np.float32(0.25)
    xb = torch.full((G, C), float(fill))
    xb[roi] = torch.from_numpy(rng.randn(len(roi), C).astype(np.float32))
    truth = xb + torch.from_numpy(rng.randn(G, C).astype(np.float32))
    y = torch.full((G, C), float("nan"))
    y[st, 0:3] = truth[st, 0:3]  # channels 0-2 at the station network
    st4 = st[::2]
    y[st4, 3] = truth[st4, 3]  # channel 3 at half of it; channel 4 unobserved
    L_roi = 150e3
    x32, x64 = _oi_pair(OI, (lats, lons, SIGMA_B, SIGMA_O, L_roi, "cpu"), {"roi_idx": roi}, xb, y)
    assert np.array_equal(x32[np.setdiff1d(np.arange(G), roi)], xb.numpy()[np.setdiff1d(np.arange(G), roi)])
    out.update(oiroi_roi=roi, oiroi_stations=st, oiroi_fill=fill, oiroi_L=np.float64(L_roi),
               oiroi_xb=xb[roi].numpy(), oiroi_y=y[roi].numpy(), oiroi_x32=x32[roi], oiroi_x64=x64[roi])

    # ---- duplicated coordinates (flat grid): the nearest-node tie rule
    rng = np.random.RandomState(13)
    n = 40
    flat_lat = np.round(rng.uniform(40, 60, n), 2)
    flat_lon = np.round(rng.uniform(80, 100, n), 2)
    for dst, src in ((7, 3), (12, 3), (20, 15), (33, 15), (39, 0)):
        flat_lat[dst], flat_lon[dst] = flat_lat[src], flat_lon[src]
    oi = OI(flat_lat, flat_lon, SIGMA_B, SIGMA_O, 300e3, "cpu", flat_grid=True)
    nearest = oi._build_H(oi._oi_coords).argmax(dim=1).numpy()
    xb = torch.from_numpy(rng.randn(n, 3).astype(np.float32))
    y = torch.full((n, 3), float("nan"))
    obs_nodes = np.array([1, 3, 7, 12, 15, 20, 25, 33, 39])
    y[obs_nodes] = xb[obs_nodes] + torch.from_numpy(rng.randn(len(obs_nodes), 3).astype(np.float32))
    y[obs_nodes[::3], 2] = float("nan")
    x32, x64 = _oi_pair(OI, (flat_lat, flat_lon, SIGMA_B, SIGMA_O, 300e3, "cpu"), {"flat_grid": True}, xb, y)
    out.update(oidup_lat=flat_lat, oidup_lon=flat_lon, oidup_L=np.float64(300e3), oidup_nearest=nearest,
               oidup_xb=xb.numpy(), oidup_y=y.numpy(), oidup_x32=x32, oidup_x64=x64)

    out.update(sigma_b=np.float64(SIGMA_B), sigma_o=np.float64(SIGMA_O))
    path = os.path.join(HERE, "assim_vectors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path) / 1e3:.0f} kB")


if __name__ == "__main__":
    main()
