"""`downscale.predict_cascade` and `CascadeRefiner` (scripts/predict_cascade.py:292-372): a stand-in GNN with exact
element-wise arithmetic (helpers/diff_stub.py: its bits cannot depend on the batch), a 13 x 22 fine archive of 12 frames,
AR = 2 and 5 samples, against a host restatement of the loop in float64 fed with the same device outputs.

Rule: every score within relative 2^-22 of the restatement (differences and squares in float32 as the reference forms
them, the mean over the pixels in float64; the reference's own float32 pairwise mean is good to about log2(HW) 2^-24).
Batch 1 and batch 3 give equal bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import unet_case as UC  # noqa: E402
from diff_stub import DiffStub  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C, OBS, NS, T, H, W, AR = 4, 2, 2, 12, 13, 22, 2
STATIC = [3]
ROI = (20.0, 40.0, 70.0, 110.0)
# sample 2 loses its second step, sample 3 is never scored (its first target is past the archive), sample 4 is left out
# altogether (its persistence frame is)
LOCAL_T = [0, 3, 9, 10, 11]


class Windows:
    """A `batch(indices)`-style data set over a normalised series [frames, G, C] with the reference's _sample_indices."""

    def __init__(self, series):
        self.series = series
        self._sample_indices = [(0, t) for t in LOCAL_T]

    def __len__(self):
        return len(LOCAL_T)

    def batch(self, indices):
        X = torch.stack([torch.cat([self.series[i + o] for o in range(OBS)], dim=1) for i in indices])
        return X.contiguous(), None


@pytest.fixture(scope="module")
def case(lib_built):
    from graphcast_lite_amd import downscale as D
    from graphcast_lite_amd.unet import WeatherUNet

    r = np.random.default_rng(5)
    lat_g, lon_g = np.meshgrid(np.linspace(10.0, 50.0, 9), np.linspace(60.0, 125.0, 14), indexing="ij")
    fine = torch.from_numpy((r.normal(size=(T, W, H, C)) * 6).astype(np.float16)).to(DEV)
    pairs = D.DownscalerPairs(torch.zeros_like(fine), fine, torch.from_numpy(r.normal(size=(W, H, NS)).astype(np.float32)).to(DEV),
                              {"mean": r.normal(size=C) * 3, "std": 0.5 + r.random(C) * 4}, np.linspace(21.0, 39.0, H),
                              np.linspace(71.0, 109.0, W), {"static_channels": STATIC, "n_time": T},
                              ["t2m", "msl", "10u", "z_static"])
    series = torch.from_numpy(r.normal(size=(len(LOCAL_T) + OBS, lat_g.size, C)).astype(np.float32)).to(DEV)
    unet = UC.randomise_(WeatherUNet(OBS * C + NS, C, 8), 77).eval().to(DEV)
    return {"D": D, "pairs": pairs, "ds": Windows(series), "unet": unet, "lats": lat_g.ravel(), "lons": lon_g.ravel(),
            "gnn_mean": (r.normal(size=C) * 3).astype(np.float32), "gnn_std": (0.5 + r.random(C) * 4).astype(np.float32)}


def run(case, batch_size, unet_residual=False, refiner=None, **kw):
    D = case["D"]
    return D.predict_cascade(DiffStub(OBS, C), case["unet"], case["ds"], case["pairs"], case["lats"], case["lons"], ROI,
                             case["gnn_mean"], case["gnn_std"], ar_steps=AR, max_samples=50, batch_size=batch_size,
                             use_residual=True, unet_residual=unet_residual, obs_window=OBS, refiner=refiner, **kw)


def _mse64(a, b):
    return np.mean(((a - b) ** 2).astype(np.float64), axis=(0, 1))


@pytest.mark.parametrize("unet_residual", [False, True])
def test_predict_cascade_equals_the_host_restatement(case, unet_residual):
    D = case["D"]
    seen = []

    class Recording(D.CascadeRefiner):
        def score(self, step, cascade_out, coarse_phys, t_fine, t_persist):
            seen.append((step, cascade_out.cpu().numpy(), coarse_phys.cpu().numpy()))
            super().score(step, cascade_out, coarse_phys, t_fine, t_persist)

    ref = Recording(case["unet"], case["pairs"], case["gnn_mean"], case["gnn_std"], OBS, unet_residual, AR)
    got = run(case, 1, unet_residual, refiner=ref)
    # :292-372 on the host, one sample at a time, from the device outputs in the order the loop produced them
    fine = case["pairs"].fine.cpu().numpy()
    ds_mean, ds_std = (case["pairs"].scalers[k].astype(np.float32) for k in ("mean", "std"))
    mse, n_per = np.zeros((AR, C, 3)), np.zeros(AR, dtype=int)
    it = iter(seen)
    for local_t in LOCAL_T:
        t_persist = local_t + OBS - 1
        if t_persist >= T:
            continue
        persist = fine[t_persist].astype(np.float32).transpose(1, 0, 2)
        for step in range(AR):
            t_fine = local_t + OBS + step
            if t_fine >= T:
                break
            s, out, phys = next(it)
            while s != step:  # (a step the loop ran for a sample that is no longer scored)
                s, out, phys = next(it)
            target = fine[t_fine].astype(np.float32).transpose(1, 0, 2)
            casc = out[0].transpose(1, 2, 0) * ds_std + ds_mean
            assert casc.dtype == np.float32
            mse[step] += np.stack([_mse64(phys[0], target), _mse64(casc, target), _mse64(persist, target)], axis=1)
            n_per[step] += 1
    assert list(n_per) == [3, 2]
    names = case["pairs"].variables
    worst = 0.0
    for s in range(AR):
        block = got[f"+{(s + 1) * 6}h"]
        assert block["n_samples"] == n_per[s]
        assert list(block["per_channel"]) == [names[c] for c in range(C) if c not in STATIC]
        for c in range(C):
            if c in STATIC:
                continue
            want = np.sqrt(mse[s, c] / n_per[s])
            for k, key in enumerate(("rmse_gnn", "rmse_cascade", "rmse_persist")):
                worst = max(worst, abs(block["per_channel"][names[c]][key] - want[k]) / want[k])
    print(f"[unet] predict_cascade (unet_residual {unet_residual}): worst relative error {worst:.3e}")
    assert worst <= 2.0 ** -22


def test_batch_size_does_not_reach_the_bits(case):
    one, three, five = run(case, 1), run(case, 3), run(case, 5)
    assert one == three == five
    assert [one[k]["n_samples"] for k in ("+6h", "+12h")] == [3, 2]


# ---- the same loop around the small GNN the other pipeline tests build (64 x 32 grid, 33 features) ----
GC = 33


@pytest.fixture(scope="module")
def gnn_case(lib_built):
    import __graft_entry__ as ge
    from graphcast_lite_amd import downscale as D
    from graphcast_lite_amd.models import WeatherPrediction
    from graphcast_lite_amd.unet import WeatherUNet

    cfg = ge._small_config()
    torch.manual_seed(42)
    lats, lons = np.linspace(-90, 90, 32, endpoint=True), np.linspace(0, 360, 64, endpoint=False)
    gnn = WeatherPrediction((lats, lons), cfg.graph, cfg.pipeline, cfg.data, torch.device(DEV)).eval()
    lon_g, lat_g = np.meshgrid(lons, lats, indexing="ij")  # node = lon * 32 + lat
    r = np.random.default_rng(6)
    fine = torch.from_numpy((r.normal(size=(T, W, H, GC)) * 6).astype(np.float16)).to(DEV)
    pairs = D.DownscalerPairs(torch.zeros_like(fine), fine, torch.from_numpy(r.normal(size=(W, H, NS)).astype(np.float32)).to(DEV),
                              {"mean": r.normal(size=GC) * 3, "std": 0.5 + r.random(GC) * 4}, np.linspace(25.0, 65.0, H),
                              np.linspace(35.0, 115.0, W), {"static_channels": [7, 8], "n_time": T}, None)
    series = torch.from_numpy(r.normal(size=(len(LOCAL_T) + OBS, lat_g.size, GC)).astype(np.float32)).to(DEV)
    unet = UC.randomise_(WeatherUNet(OBS * GC + NS, GC, 8), 78).eval().to(DEV)
    return {"D": D, "gnn": gnn, "pairs": pairs, "ds": Windows(series), "unet": unet, "lats": lat_g.ravel(),
            "lons": lon_g.ravel(), "gnn_mean": (r.normal(size=GC) * 3).astype(np.float32),
            "gnn_std": (0.5 + r.random(GC) * 4).astype(np.float32)}


def test_cascade_around_the_small_gnn(gnn_case):
    """The real model in the loop: every batch size against the float64 restatement of the scores from its own device
    outputs, and batch 1 = batch 3 bit for bit."""
    c, D = gnn_case, gnn_case["D"]
    roi = (20.0, 70.0, 30.0, 120.0)
    fine = c["pairs"].fine.cpu().numpy()
    ds_mean, ds_std = (c["pairs"].scalers[k].astype(np.float32) for k in ("mean", "std"))
    results = {}
    for bs in (1, 3):
        seen = []

        class Recording(D.CascadeRefiner):
            def score(self, step, cascade_out, coarse_phys, t_fine, t_persist):
                seen.append((step, cascade_out.cpu().numpy(), coarse_phys.cpu().numpy(), [int(t) for t in t_fine.cpu()],
                             [int(t) for t in t_persist.cpu()]))
                super().score(step, cascade_out, coarse_phys, t_fine, t_persist)

        ref = Recording(c["unet"], c["pairs"], c["gnn_mean"], c["gnn_std"], OBS, False, AR)
        got = D.predict_cascade(c["gnn"], c["unet"], c["ds"], c["pairs"], c["lats"], c["lons"], roi, c["gnn_mean"],
                                c["gnn_std"], ar_steps=AR, batch_size=bs, use_residual=True, refiner=ref)
        mse, n_per = np.zeros((AR, GC, 3)), np.zeros(AR, dtype=int)
        pairs_seen = set()
        for step, out, phys, tf, tp in seen:
            for b in range(len(tf)):
                if not 0 <= tf[b] < T:
                    continue
                assert tf[b] == tp[b] + 1 + step  # t_fine = local_t + obs + step, t_persist = local_t + obs - 1
                pairs_seen.add((tp[b] - OBS + 1, step))
                target = fine[tf[b]].astype(np.float32).transpose(1, 0, 2)
                persist = fine[tp[b]].astype(np.float32).transpose(1, 0, 2)
                casc = out[b].transpose(1, 2, 0) * ds_std + ds_mean
                mse[step] += np.stack([_mse64(phys[b], target), _mse64(casc, target), _mse64(persist, target)], axis=1)
                n_per[step] += 1
        assert pairs_seen == {(0, 0), (0, 1), (3, 0), (3, 1), (9, 0)} and list(n_per) == [3, 2]
        worst = 0.0
        for s in range(AR):
            block = got[f"+{(s + 1) * 6}h"]
            assert block["n_samples"] == n_per[s] and list(block["per_channel"]) == [f"ch{k}" for k in range(GC) if k not in (7, 8)]
            for k in range(GC):
                if k in (7, 8):
                    continue
                want = np.sqrt(mse[s, k] / n_per[s])
                for j, key in enumerate(("rmse_gnn", "rmse_cascade", "rmse_persist")):
                    worst = max(worst, abs(block["per_channel"][f"ch{k}"][key] - want[j]) / want[j])
        print(f"[unet] predict_cascade around the small GNN, batch {bs}: worst relative error {worst:.3e}")
        assert worst <= 2.0 ** -22
        results[bs] = got
    assert results[1] == results[3]


def test_refiner_is_pack_then_network(case):
    D = case["D"]
    from graphcast_lite_amd import hip

    ref = D.CascadeRefiner(case["unet"], case["pairs"], case["gnn_mean"], case["gnn_std"], OBS, True, AR)
    coarse = torch.randn(3, H, W, C, generator=torch.Generator().manual_seed(3)).to(DEV)
    out, phys = ref.refine(coarse)
    phys2, X = hip.cascade_pack(coarse, ref.gnn_mean, ref.gnn_std, ref.ds_mean, ref.ds_std, ref.static_fine, OBS)
    assert X.shape == (3, OBS * C + NS, H, W) and torch.equal(phys, phys2)
    want = X[:, (OBS - 1) * C:OBS * C] + case["unet"](X)
    assert torch.equal(out, want)
    with pytest.raises(ValueError, match="coarse"):
        ref.refine(coarse[:, :, :-1])


def test_save_cascade_results(case, tmp_path):
    import json

    D = case["D"]
    res = run(case, 3)
    path = D.save_cascade_results(res, str(tmp_path))
    assert os.path.basename(path) == "cascade_results.json" and json.load(open(path)) == res
