"""What the predict / observations / regional-scoring tests share: the fixture of
tests/golden/make_predict_golden.py, the directories its option sets ran over (rebuilt from the fixture's inputs), the
wiring of one option set onto `predict_experiment`, and the numpy restatements of the two kernels of csrc/predict.hip."""
import json
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
_Z = None
LD = np.longdouble


def fixture():
    global _Z
    if _Z is None:
        _Z = np.load(os.path.join(GOLDEN, "predict_vectors.npz"))
    return _Z


def set_names():
    return [str(s) for s in fixture()["sets"]]


# ----------------------------------------------------------------------------------------------------------------------
# scripts/predict.py option sets
# ----------------------------------------------------------------------------------------------------------------------
SET_EXTRA = {  # what the generator's SETS give besides argv
    "onestep": dict(pred_model=1, targets=1), "onestep_nores": dict(pred_model=1, targets=1), "multistep": dict(pred_model=3),
    "flat": dict(flat=True), "bmw": dict(bmw=1), "short": dict(targets=1), "legacy": dict(legacy=True),
}
SET_DATA = {"plain": "coords", "flat": "flat", "prune": "coords", "legacy": "legacy"}  # every other set: "plain"


def write_dirs(tmp, z):
    """The data directories of the generator: {plain, coords, flat, legacy} -> path."""
    dirs = {}
    for name in ("plain", "coords", "flat", "legacy"):
        d = os.path.join(str(tmp), "data_" + name)
        os.makedirs(d, exist_ok=True)
        json.dump([str(v) for v in z["variables"]], open(os.path.join(d, "variables.json"), "w"))
        np.savez(os.path.join(d, "scalers.npz"), std=z["std"], mean=np.zeros(len(z["std"])))
        if name != "legacy":
            open(os.path.join(d, "dataset_info.json"), "w").write("{}")
        dirs[name] = d
    np.savez(os.path.join(dirs["coords"], "coords.npz"), latitude=z["coords_lats"], longitude=z["coords_lons"])
    np.savez(os.path.join(dirs["flat"], "coords.npz"), latitude=z["flat_lats"], longitude=z["flat_lons"])
    torch.save(torch.from_numpy(z["background"]), os.path.join(str(tmp), "background.pt"))
    return dirs


def set_args(z, name, tmp):
    """The parsed options of one recorded set (through the product's own parser)."""
    from graphcast_lite_amd.predict import build_parser

    argv = [str(a).replace("<tmp>", str(tmp)) for a in z[f"{name}:argv"] if str(a)]
    return build_parser().parse_args(["exp"] + argv)


def set_meta(z, name):
    n_lon, n_lat, C, obs, ns = (int(v) for v in z["dims"])
    if SET_EXTRA.get(name, {}).get("flat"):
        return types.SimpleNamespace(num_latitudes=0, num_longitudes=0, flat_grid=True, num_grid_nodes=n_lon * n_lat,
                                     is_regional=z["is_regional"],
                                     cordinates=(z["flat_lats"].astype(np.float32), z["flat_lons"].astype(np.float32)))
    return types.SimpleNamespace(num_latitudes=n_lat, num_longitudes=n_lon, flat_grid=False, num_grid_nodes=n_lon * n_lat,
                                 is_regional=None)


def recorded_objects(z, name):
    """The recorded `StreamingMetrics` objects of a set, in creation order, as {field: value}."""
    fields = [str(f) for f in z["sm_fields"]]
    n = int(z[f"{name}:n_objects"])
    return [{f: z[f"{name}:sm:{f}"][i] for f in fields} for i in range(n)]


def creation_order(ar_steps: int, has_region: bool):
    """scripts/predict.py:425-439: the (kind, method, horizon) of every object in the order the script creates them."""
    order = [("overall", "pred", None), ("overall", "base", None)]
    if has_region:
        order += [("region", "pred", None), ("region", "base", None)]
    if ar_steps > 1:
        for p in range(ar_steps):
            order += [("horizon", "pred", p), ("horizon", "base", p)]
            if has_region:
                order += [("region_horizon", "pred", p), ("region_horizon", "base", p)]
    return order


def verifier_object(ver, kind, method, p):
    group = getattr(ver, kind)[method]
    return group if p is None else group[p]


def host_metrics(rec, C, exclude):
    """A `verify.StreamingMetrics` whose state is a recorded object's (on the host)."""
    from graphcast_lite_amd.verify import StreamingMetrics

    sm = StreamingMetrics(C, exclude_channels=[int(c) for c in exclude])
    sm._state = torch.from_numpy(np.concatenate([[rec["sum_se"], rec["sum_ae"], rec["n"], rec["total_elem"]],
                                                 rec["sum_se_per_ch"], rec["sum_acc"], rec["elem_per_ch"],
                                                 rec["acc_count"]]).astype(np.float64))
    return sm


_NUM = r"-?\d+\.\d+"


def same_lines(got, want, rel, what):
    """The rule of `_same_lines` in tests/test_regional_train_golden.py (restated, so that no test module imports
    another): the same text once the numbers are masked, and every number within rel (plus one unit of its last printed
    digit; percentages, which are differences of two scores over one of them, within 0.02 points + that)."""
    import re

    assert re.sub(_NUM, "#", got) == re.sub(_NUM, "#", want), (what, got, want)
    for a, b in zip(re.finditer(_NUM + "%?", got), re.finditer(_NUM + "%?", want)):
        digit = 10.0 ** -len(b.group().rstrip("%").split(".")[1])
        x, y = float(a.group().rstrip("%")), float(b.group().rstrip("%"))
        tol = 1.01 * digit + (0.02 if b.group().endswith("%") else rel * abs(y))
        assert abs(x - y) <= tol, (what, got, want)


def summary_block(text: str) -> str:
    """From the `=====` line before `=== Inference summary` to the end."""
    return text[text.index("=" * 60 + "\n=== Inference summary"):].rstrip("\n")


class ListDataset:
    """`batch(indices)` over device tensors X [N, G, F], y [N, G, K]."""

    def __init__(self, X, y):
        self.X, self.y = X, y

    def __len__(self):
        return self.X.shape[0]

    def batch(self, indices, out=None):
        idx = torch.as_tensor(list(indices), dtype=torch.int64, device=self.X.device)
        return self.X.index_select(0, idx), self.y.index_select(0, idx)


class PerSample(torch.nn.Module):
    """A model applied sample by sample: its rows cannot depend on the batch size."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.obs_window = inner, inner.obs_window

    def forward(self, X, attention_threshold=0.0, **kw):
        return torch.cat([self.inner(X[b:b + 1]) for b in range(X.shape[0])], dim=0)


def run_set(z, name, tmp, device, batch_size=8, per_sample=False, say=print, dirs=None):
    """One recorded option set through `predict_experiment`, wired as `predict.main` wires it, on the fixture's
    samples and its tanh stub model.  Returns (PredictRun, args, (variables, std))."""
    from stub_model import StubModel

    from graphcast_lite_amd import predict as P
    from graphcast_lite_amd.assimilation import OptimalInterpolation, build_boundary_taper_mask, station_network
    from graphcast_lite_amd.verify import linspace_lats_lons

    extra = SET_EXTRA.get(name, {})
    n_lon, n_lat, C, obs, ns = (int(v) for v in z["dims"])
    G = n_lon * n_lat
    dirs = dirs or write_dirs(tmp, z)
    data_dir = dirs[SET_DATA.get(name, "plain")]
    args = set_args(z, name, tmp)
    meta = set_meta(z, name)
    p_model = extra.get("pred_model", 1)
    tag = "s1" if extra.get("targets", 3) == 1 else "s3"
    ds = ListDataset(torch.from_numpy(z[f"{tag}_X"]).to(device), torch.from_numpy(z[f"{tag}_y"]).to(device))
    model = StubModel(obs, z["W3"] if p_model == 3 else z["W0"], z["b3"] if p_model == 3 else z["b0"], device)
    if per_sample:
        model = PerSample(model)
    AR = args.ar_steps if args.ar_steps else p_model
    chunked = P.is_chunked_dir(data_dir)
    max_samples = args.max_samples if args.max_samples is not None else (min(len(ds), 200) if chunked else len(ds))
    rows, label = P.scored_rows(args.region, extra.get("bmw", 0), meta, data_dir, G, say=say)
    oi = None
    coords_file = os.path.join(data_dir, "coords.npz")
    if args.assim_method == "oi":
        if os.path.exists(coords_file):
            c = np.load(coords_file)
            lats, lons = c["latitude"].astype(np.float32), c["longitude"].astype(np.float32)
        else:
            lats, lons = linspace_lats_lons(n_lat, n_lon)
        roi_idx = rows
        if roi_idx is None and meta.flat_grid and meta.is_regional is not None:
            roi_idx = np.where(meta.is_regional)[0]
        oi = OptimalInterpolation(lats, lons, args.oi_sigma_b, args.oi_sigma_o, args.oi_corr_len, device,
                                  flat_grid=meta.flat_grid, roi_idx=roi_idx)
    stations = None
    if args.obs_sparsity is not None and args.assim_method != "none":
        stations = station_network(P.station_pool(args.obs_roi_only, rows, meta, G), args.obs_sparsity, args.obs_seed)
    obs_ch = None
    if args.obs_channels is not None:
        obs_ch = P.observed_channels(args.obs_channels, [str(v) for v in z["variables"]], C, say=say)
    mask = background = None
    if args.boundary_blending:
        background = torch.load(args.background_path, weights_only=True)
        mask = build_boundary_taper_mask(n_lat, n_lon, args.taper_width, args.taper_width).reshape(G).float().to(device)
    keep = bool(args.save) and not args.no_save
    run = P.predict_experiment(model, ds, C, AR, pred_window=p_model, max_samples=max_samples, batch_size=batch_size,
                               use_residual=not args.no_residual, static_channels=[1], forcing_channels=[3],
                               region_rows=rows, region_label=label, grid=(meta.num_longitudes, meta.num_latitudes),
                               assim_method=args.assim_method, nudging_mode=args.nudging_mode,
                               nudging_alpha=args.nudging_alpha, nudge_first_k=args.nudge_first_k, oi=oi,
                               station_rows=stations, obs_channels=obs_ch, boundary_mask=mask, background=background,
                               keep=keep, use_graph=False, device=device, say=say)
    variables = std = None
    if args.per_channel:
        variables, std = [str(v) for v in z["variables"]], z["std"]
    run.stations, run.obs_channels, run.rows = stations, obs_ch, rows
    return run, args, (variables, std)


# ----------------------------------------------------------------------------------------------------------------------
# gcl_obs_pack, restated
# ----------------------------------------------------------------------------------------------------------------------
def obs_pack_ref(y, keep_row, keep_chan):
    """int32 bits of the packed observations: y [B, G, K] float32, keep_row bool [G], keep_chan bool [C]."""
    B, G, K = y.shape
    keep = keep_row[None, :, None] & keep_chan[np.arange(K) % len(keep_chan)][None, None, :]
    bits = np.ascontiguousarray(y).view(np.int32).copy()
    bits[~np.broadcast_to(keep, bits.shape)] = 0x7fc00000
    return bits


# ----------------------------------------------------------------------------------------------------------------------
# gcl_region_interp_scores, restated
# ----------------------------------------------------------------------------------------------------------------------
def region_fields(pred, n_lat, cell, w, series, t0, mean, std, P, C):
    """float64 (v, t, b) [N, P, nr, C] as include/gcl.h states them (NaN rows for skipped samples): the bilinear value
    with its four products rounded one by one and added left to right, truth and persistence from the fp16 series."""
    N = pred.shape[0]
    nr = cell.shape[0]
    n00 = cell[:, 0].astype(np.int64) * n_lat + cell[:, 1]
    v = np.full((N, P, nr, C), np.nan)
    t, b = v.copy(), v.copy()
    src = pred.astype(np.float64)
    sr = series.astype(np.float64)
    for s in range(N):
        if t0[s] < 1 or t0[s] + P > series.shape[0]:
            continue
        for p in range(P):
            cols = src[s][:, p * C:(p + 1) * C]
            acc = cols[n00] * w[:, 0:1]
            acc = acc + cols[n00 + 1] * w[:, 1:2]
            acc = acc + cols[n00 + n_lat] * w[:, 2:3]
            acc = acc + cols[n00 + n_lat + 1] * w[:, 3:4]
            v[s, p] = acc
            t[s, p] = (sr[t0[s] + p][:, :C] - mean) / std
            b[s, p] = (sr[t0[s] - 1][:, :C] - mean) / std
    return v, t, b


def region_sums(v, t, b, t0, n_time):
    """[P, C, 11] in extended precision, rounded to float64: the sums of include/gcl.h about the pivots (node 0 of the
    first matched sample)."""
    N, P, nr, C = v.shape
    ok = np.asarray([(t0[s] >= 1 and t0[s] + P <= n_time) for s in range(N)])
    first = int(np.nonzero(ok)[0][0])
    vl, tl, bl = v[ok].astype(LD), t[ok].astype(LD), b[ok].astype(LD)
    out = np.zeros((P, C, 11), dtype=np.float64)
    for p in range(P):
        for c in range(C):
            vv, tt, bb = vl[:, p, :, c].ravel(), tl[:, p, :, c].ravel(), bl[:, p, :, c].ravel()
            tp, vp = LD(t[first, p, 0, c]), LD(v[first, p, 0, c])
            tc, vc = tt - tp, vv - vp
            out[p, c] = [((vv - tt) ** 2).sum(), np.abs(vv - tt).sum(), ((bb - tt) ** 2).sum(), vv.size, tc.sum(),
                         (tc * tc).sum(), vc.sum(), (vc * vc).sum(), (tc * vc).sum(), tp, vp]
    return out


def interp_inputs(z):
    """The regional-scoring fixture: everything `interpolate_to_region.main()` read, as arrays."""
    nlg, ntg, nlr, ntr, C, P, nf, nt, obs = (int(v) for v in z["interp:dims"])
    series = z["interp:series_bits"].view(np.float16).reshape(nt, nlr * ntr, nf)
    return dict(nlg=nlg, ntg=ntg, nlr=nlr, ntr=ntr, C=C, P=P, nf=nf, nt=nt, obs=obs, series=series,
                pred=z["interp:predictions"], truth=z["interp:ground_truth"],
                offsets=[int(v) for v in z["interp:sample_offsets"]], g_lats=z["interp:g_lats"], g_lons=z["interp:g_lons"],
                r_lats=z["interp:r_lats"], r_lons=z["interp:r_lons"], mean=z["interp:mean"], std=z["interp:std"],
                names=[str(v) for v in z["interp:names"]])


def write_interp_dirs(tmp, z):
    """(bundle path, global directory, regional directory) as the generator wrote them."""
    f = interp_inputs(z)
    gd, rd = os.path.join(str(tmp), "glob"), os.path.join(str(tmp), "reg")
    os.makedirs(gd, exist_ok=True), os.makedirs(rd, exist_ok=True)
    np.savez(os.path.join(gd, "coords.npz"), latitude=f["g_lats"], longitude=f["g_lons"])
    np.savez(os.path.join(rd, "coords.npz"), latitude=f["r_lats"], longitude=f["r_lons"])
    json.dump(f["names"], open(os.path.join(gd, "variables.json"), "w"))
    open(os.path.join(gd, "dataset_info.json"), "w").write(str(z["interp:global_info"]))
    open(os.path.join(rd, "dataset_info.json"), "w").write(str(z["interp:region_info"]))
    np.savez(os.path.join(rd, "scalers.npz"), mean=f["mean"], std=f["std"])
    np.ascontiguousarray(f["series"]).tofile(os.path.join(rd, "data.npy"))
    bundle = os.path.join(str(tmp), "pred_bundle.pt")
    from graphcast_lite_amd.predict import save_predictions

    save_predictions(bundle, torch.from_numpy(f["pred"]), torch.from_numpy(f["truth"]), f["C"], f["P"], f["obs"], f["nlg"],
                     f["ntg"], sample_offsets=f["offsets"], data_dir="x")
    return bundle, gd, rd
