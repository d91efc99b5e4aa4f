"""The MOS kernels (csrc/mos.hip) called through their C entry points on operands laid out by tests/helpers/layouts.py (NaN
around every input, a sentinel around every output), against restatements written in tests/helpers/mos_ref.py from the
kernel file's header comments.  MOSForest only packs the nodes; nothing else of mos.py runs here.  The file holds the CPU
tests that tie the restatements to sklearn's and the reference's recorded output, so the GPU tests carry the mark one by
one.

Rules:
  forest_eval     bit-equal to the float64 walk, for tree counts on both sides of every pass_max and the LDS limit
  forest_predict  features bit-equal (the wind-direction sine and cosine to 4 spacing(1.0): atan2 to 2 ulp of an angle
                  up to pi, through a slope <= 1), group bias bit-equal with numpy's own np.mean as the arbiter of the
                  pairwise sum, n_corrected zeroed; the reference proves that no feature 3 / 4 it compares lies within
                  1e-9 of its threshold
  idw_apply       own rows bit-equal to x + bias; float32 output within one float32 ulp; the float64 field held to
                  c eps (1 + power) sum_k |w_k b_k| with c four times what numpy float64 loses against np.longdouble
                  on the same cases (floor 8), and bit-equal to numpy where every point in reach is under the clamp
                  (the order of the one-step pairwise sum then decides the bits alone); n_corrected equal for both `idw` values; every other element keeps its bits
  idw_sweep       acc within n_terms 2^-52 sum(e) of math.fsum over the squared errors restated from fields_out, with
                  257 and 513 block partials per (setting, step)
  table_apply     bit-equal to x + float32(tb[s]) (float64: x + tb[s]), past the 8192-block grid and in place
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import mos_ref as R  # noqa: E402
from layouts import DEV, NAN, SENT, Field4, Guarded, Worst, has, launched, same_bits  # noqa: E402

gpu = pytest.mark.gpu
W_ = Worst("MOS kernels")
EPS = 2.0 ** -52
KMAX = 128  # kMaxPoints: station groups, stations per group, IDW points


@pytest.fixture(scope="module")
def hip(lib_built):
    from graphcast_lite_amd import hip as H

    return H


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV).contiguous()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def ptr_of(g):
    """Address of a Guarded view's first element (an empty view's data_ptr() is 0)."""
    return g.buf.data_ptr() + 8 * g.buf.element_size()


# ------------------------------------------------------------------------------------------------------------------
# Forests
# ------------------------------------------------------------------------------------------------------------------
# stations per pass: max(1, min(128, 49152 / (8 T), (8192 - 128) / (20 + T))), the second bound keeping features, leaves
# and the 128 group biases within 64 KiB of LDS; 64 and 8044 trees fill it exactly
TREES = (1, 48, 49, 384, 6144, 8044)
PASS_MAX = {1: 128, 48: 118, 49: 116, 64: 96, 384: 16, 768: 8, 6144: 1, 8044: 1}
EVAL_N = (0, 1, 127, 128, 129)  # around the 128-row block


@functools.lru_cache(maxsize=None)
def forest(T, zero=False):
    return R.synth_forest(T, 9000 + T, zero)


_packed = {}


def packed(T, zero=False):
    """(nodes, roots) of forest(T) on the device, in the kernels' 16-byte node layout."""
    from graphcast_lite_amd.mos import MOSForest

    if (T, zero) not in _packed:
        fr = forest(T, zero)
        _packed[T, zero] = MOSForest(*(fr[k] for k in MOSForest._FIELDS), fr["baseline"]).to(DEV)
    return _packed[T, zero]


def special(x, rng, pool_cols, p_eq=0.15, p_nan=0.15, p_inf=0.03):
    """x [.., F] with some entries equal to a threshold of their feature (pool_cols [F, POOL]), some NaN, some +-inf."""
    u = rng.random(x.shape)
    j = rng.integers(0, R.POOL, x.shape)
    eq = pool_cols[np.broadcast_to(np.arange(x.shape[-1]), x.shape), j]
    x = np.where(u < p_eq, eq, x)
    x = np.where((u >= p_eq) & (u < p_eq + p_nan), np.nan, x)
    x = np.where((u >= 0.9) & (u < 0.9 + p_inf), np.inf, x)
    return np.where(u >= 1 - p_inf, -np.inf, x)


def eval_rows(T, n):
    rng = np.random.default_rng(T * 1000 + n)
    X = R.CENTRE + R.SCALE * rng.standard_normal((n, R.NUM_FEAT))
    return special(X, rng, R.pools(9000 + T))


def test_synthetic_forests_cover_the_walk():
    """CPU: the forests and rows of the GPU tests hold what the issue lists - a tree whose root is a leaf, depth 6,
    splits on features 0 and 19, NaN sent both ways, a feature equal to its threshold, infinite features - and the
    leaves span twelve decades."""
    for T in TREES + (64, 768):
        fr = forest(T)
        assert PASS_MAX[T] == max(1, min(KMAX, 48 * 1024 // (8 * T), (8192 - KMAX) // (R.NUM_FEAT + T)))
        if T >= 48:
            assert fr["is_leaf"][fr["roots"]].any() and not fr["is_leaf"][fr["roots"]].all()
            split = fr["is_leaf"] == 0
            assert {0, 19} <= set(fr["feature"][split].tolist())
            lv = np.abs(fr["value"][~split])
            assert lv.min() < 1e-5 and lv.max() > 1e5
            depth = np.zeros(fr["value"].size, dtype=np.int64)  # children follow their parent in the node array
            for i in np.flatnonzero(split):
                depth[fr["left"][i]] = depth[fr["right"][i]] = depth[i] + 1
            assert depth.max() == 6 if T >= 384 else depth.max() >= 4
            st = {}
            R.walk(fr, eval_rows(T, 129), stats=st)
            assert min(st[k] for k in ("nan_left", "nan_right", "equal", "inf")) > 0, st
    lds = lambda T: (PASS_MAX[T] * R.NUM_FEAT + PASS_MAX[T] * T + KMAX) * 8  # noqa: E731
    assert lds(8044) == lds(64) == 64 * 1024 and (1 * R.NUM_FEAT + 8045 + KMAX) * 8 > 64 * 1024
    assert all(lds(T) <= 64 * 1024 for T in PASS_MAX)


def test_walk_reproduces_sklearn():
    """CPU: the test's walk gives sklearn's recorded predictions of the fixture forest bit for bit."""
    gm = np.load(os.path.join(GOLDEN, "mos_vectors.npz"))
    fr = fixture_forest(gm)
    y, _ = R.walk(fr, gm["pred_X"])
    assert np.array_equal(bits(y), bits(gm["pred_y"]))


def fixture_forest(gm):
    return dict(feature=gm["forest_feature"].astype(np.int32), value=gm["forest_value"],
                left=gm["forest_left"].astype(np.int64), right=gm["forest_right"].astype(np.int64),
                missing_left=gm["forest_missing_left"], is_leaf=gm["forest_is_leaf"], roots=gm["forest_roots"],
                baseline=float(gm["forest_baseline"]))


@pytest.mark.parametrize("case,power,radius", [("c", 2.0, 300.0), ("d", 1.5, 150.0)])
def test_idw_restatement_reproduces_reference_field(case, power, radius):
    """CPU: the reference's recorded features of cases c and d (19 stations on the 41 x 61 box grid, 4 steps), through
    the test's walk, np.mean and IDW restatement, give the reference's recorded bias field bit for bit."""
    gm = np.load(os.path.join(GOLDEN, "mos_vectors.npz"))
    fr = fixture_forest(gm)
    feat, steps = gm[f"{case}_feat"], 4
    lat = np.tile(50.0 + 0.25 * np.arange(41), 61).astype(np.float32)
    lon = np.repeat(85.0 + 0.25 * np.arange(61), 41).astype(np.float32)
    y, _ = R.walk(fr, feat)
    # the rows come group by group, step by step, station by station: a group's first station returns after n rows
    pt_idx, bias, p = [], [], 0
    while p < len(feat):
        n = 1
        while not np.array_equal(feat[p + n, 17:19], feat[p, 17:19]):
            n += 1
        near = {int(np.argmin((lat - feat[p + q, 17]) ** 2 + (lon - feat[p + q, 18]) ** 2)) for q in range(n)}
        assert len(near) == 1
        pt_idx.append(near.pop())
        bias.append([float(np.mean(list(y[p + s * n:p + (s + 1) * n]))) for s in range(steps)])
        p += n * steps
    assert len(set(pt_idx)) == len(pt_idx)
    assert np.array_equal(bits(y), bits(gm[f"{case}_bias"]))  # the model's recorded prediction of every feature row
    dists, own = R.idw_dists(lat, lon, pt_idx)
    field, _ = R.idw_field(dists, own, np.array(bias), power, radius)
    assert np.array_equal(bits(field), bits(gm[f"{case}_field"]))


@gpu
@pytest.mark.parametrize("T", TREES)
def test_forest_eval(hip, T):
    fr = forest(T)
    nodes, roots = packed(T)
    for n in EVAL_N:
        X = eval_rows(T, n)
        Xd = Guarded((n, R.NUM_FEAT), torch.float64, fill=NAN, init=dev(X) if n else None)
        y = Guarded((n,), torch.float64)
        hip._check(hip.lib().gcl_mos_forest_eval(nodes.data_ptr(), roots.data_ptr(), T, fr["baseline"], ptr_of(Xd), n,
                                                 ptr_of(y), hip._stream()))
        torch.cuda.synchronize()
        assert y.untouched()
        ref, _ = R.walk(fr, X)
        assert np.array_equal(bits(y.view.cpu().numpy()), bits(ref)), f"T={T} n={n}"
    W_.exact("forest_eval")


# ------------------------------------------------------------------------------------------------------------------
# Station recurrence
# ------------------------------------------------------------------------------------------------------------------
CH = dict(t2m=2, u=0, v=4, sp=5, tp=3)  # of 7 channels; 1 and 6 are never read and hold NaN
NCH = 7
MANY = tuple([1, 2, 3, 8, 9, 7, 12][i % 7] for i in range(KMAX))  # 128 groups
PREDICT = {  # trees, group sizes, B, steps, float64, absent channel, feat_out, n_corrected, all-zero forest
    "ragged_last_pass": (49, (128, 1, 7, 13), 1, 2, False, None, True, True, False),  # 128 = 116 + 12
    "lds_filled_at_64_trees": (64, (127, 9), 1, 2, True, None, True, True, False),  # 127 = 96 + 31
    "nine_passes_of_one": (6144, (9, 1), 3, 5, True, "u", True, False, False),
    "three_passes_of_eight": (768, (24, 8, 12), 1, 5, False, "v", False, True, False),
    "passes_of_sixteen": (384, (16, 17, 64, 9), 3, 2, True, "sp", True, True, False),
    "128_groups": (48, MANY, 1, 1, False, "tp", True, True, False),
    "lds_limit": (8044, (12, 127), 1, 1, True, None, False, False, False),
    "single_pass": (1, (128, 127, 64, 17, 16), 3, 2, False, None, True, True, False),
    "signed_zero": (48, (8, 16, 9, 7), 1, 2, True, None, True, True, True),
}
assert {n for c in PREDICT.values() for n in c[1]} >= {1, 7, 8, 9, 12, 13, 16, 17, 24, 64, 127, 128}


@functools.lru_cache(maxsize=None)
def predict_case(name):
    T, sizes, B, steps, f64, absent, _, _, zero = PREDICT[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    ng, nst = len(sizes), sum(sizes)
    G = 2 * ng + 3
    grid_idx = rng.permutation(G)[:ng].astype(np.int32)
    gstart = np.cumsum((0,) + tuple(sizes)).astype(np.int32)
    v = rng.standard_normal((B, ng, steps, NCH))
    v[..., CH["t2m"]] = 265 + 15 * v[..., CH["t2m"]]
    v[..., CH["u"]] *= 6
    v[..., CH["v"]] *= 6
    v[..., CH["sp"]] = 95000 + 3000 * v[..., CH["sp"]]
    v[..., CH["tp"]] = 1e-3 * np.abs(v[..., CH["tp"]])
    v[..., [1, 6]] = np.nan
    x = np.full((B, G, steps, NCH), np.nan)  # only the groups' rows hold numbers
    x[:, grid_idx] = v
    x = x.astype(np.float64 if f64 else np.float32)
    chans = tuple(-1 if k == absent else CH[k] for k in ("t2m", "u", "v", "sp", "tp"))
    tf = special(rng.standard_normal((B, nst, steps, 8)), rng, R.pools(9000 + T)[list(R.TIME_COLS)], p_nan=0.05)
    fr = forest(T, zero)
    bias, feats, gap = R.station_recurrence(fr, x.astype(np.float64), chans, grid_idx, gstart, tf)
    return dict(x=x, chans=chans, tf=tf, grid_idx=grid_idx, gstart=gstart, bias=bias, feats=feats, gap=gap, G=G)


def test_predict_inputs_leave_wind_direction_splits_alone():
    """CPU: no wind-direction sine or cosine that a reference walk compares lies within 1e-9 of its threshold, in any
    case, so the 4 spacing(1.0) the device may differ by cannot change a branch; and numpy's mean of an all -0.0
    group is +0.0 at every group size."""
    for name in PREDICT:
        assert predict_case(name)["gap"] >= 1e-9, name
    z = predict_case("signed_zero")["bias"]
    assert not np.signbit(z).any() and (z == 0).all()


@gpu
@pytest.mark.parametrize("name", list(PREDICT))
def test_forest_predict(hip, name):
    T, sizes, B, steps, f64, _, want_feat, want_n, zero = PREDICT[name]
    c = predict_case(name)
    assert c["gap"] >= 1e-9
    fr = forest(T, zero)
    nodes, roots = packed(T, zero)
    ng, nst = len(sizes), sum(sizes)
    X = Field4.of(dev(c["x"]))
    tf = Guarded((B, nst, steps, 8), torch.float64, fill=NAN, init=dev(c["tf"]))
    bias = Guarded((B, ng, steps), torch.float64)
    fo = Guarded((B, nst, steps, R.NUM_FEAT), torch.float64)
    nc = Guarded((B,), torch.int32, fill=-7, init=torch.full((B,), 77, dtype=torch.int32, device=DEV))
    gi, gs = dev(c["grid_idx"]), dev(c["gstart"])

    def call(ngroups=ng):
        hip._check(hip.lib().gcl_mos_forest_predict(
            nodes.data_ptr(), roots.data_ptr(), T, fr["baseline"], X.ptr, int(f64), *X.strides, steps, *c["chans"],
            gi.data_ptr(), gs.data_ptr(), ngroups, nst, ptr_of(tf), ptr_of(bias), ptr_of(fo) if want_feat else None,
            ptr_of(nc) if want_n else None, B, hip._stream()))

    _, names = launched(call)
    assert has(names, "forest_station_kernel")
    assert bias.untouched() and fo.untouched() and nc.untouched() and X.untouched()
    assert same_bits(X.view, dev(c["x"]))
    got = bias.view.cpu().numpy()
    assert np.array_equal(bits(got), bits(c["bias"])), \
        f"{name}: bias differs at {np.argwhere(bits(got) != bits(c['bias']))[:4].tolist()}"
    if want_feat:
        f, ref = fo.view.cpu().numpy(), c["feats"]
        exact = [j for j in range(R.NUM_FEAT) if j not in (3, 4)]
        assert np.array_equal(bits(f[..., exact]), bits(ref[..., exact]))
        for j in (3, 4):
            assert np.array_equal(np.isnan(f[..., j]), np.isnan(ref[..., j]))
            ok = ~np.isnan(ref[..., j])
            assert np.abs(f[..., j][ok] - ref[..., j][ok]).max(initial=0) <= 4 * np.spacing(1.0)
    else:
        assert (fo.view == SENT).all()
    assert nc.view.tolist() == [0 if want_n else 77] * B
    W_.exact("forest_predict")


@gpu
def test_forest_predict_limits(hip):
    """129 groups and 8045 trees are refused before any launch."""
    c = predict_case("128_groups")
    nodes, roots = packed(48)
    gi = dev(np.append(c["grid_idx"], 0).astype(np.int32))
    gs = dev(np.append(c["gstart"], c["gstart"][-1] + 1).astype(np.int32))
    nst = int(c["gstart"][-1]) + 1
    X = Field4.of(dev(c["x"]))
    tf = torch.zeros(1, nst, 1, 8, dtype=torch.float64, device=DEV)
    bias = torch.zeros(1, KMAX + 1, 1, dtype=torch.float64, device=DEV)

    def call(nd, rt, T, ngroups):
        hip._check(hip.lib().gcl_mos_forest_predict(
            nd.data_ptr(), rt.data_ptr(), T, 0.0, X.ptr, 0, *X.strides, 1, *c["chans"], gi.data_ptr(), gs.data_ptr(),
            ngroups, nst, tf.data_ptr(), bias.data_ptr(), None, None, 1, hip._stream()))

    with pytest.raises(RuntimeError, match="129 groups"):
        call(nodes, roots, 48, KMAX + 1)
    n2, r2 = packed(8045)
    with pytest.raises(RuntimeError, match="8045 trees"):
        call(n2, r2, 8045, 2)
    torch.cuda.synchronize()
    assert (bias == 0).all()


# ------------------------------------------------------------------------------------------------------------------
# IDW spread and apply
# ------------------------------------------------------------------------------------------------------------------
C_LAT, C_LON = 56.0, 92.0
T2M, IDW_C = 1, 3  # t2m channel of three
IDW = {  # G, K, steps, power, idw, B, float64, placement, radius, special
    "one_row": (1, 1, 1, 2.0, True, 1, False, "out", 300.0, None),
    "k7": (127, 7, 2, 1.0, True, 3, True, "inplace", 300.0, None),
    "all_stations": (128, 128, 15, 2.0, False, 1, False, "strided", 300.0, None),
    "k8": (129, 8, 16, 1.5, True, 1, True, "out", 300.0, None),
    "k9": (129, 9, 17, 2.0, True, 3, False, "inplace", 300.0, None),
    "k16": (257, 16, 33, 1.0, True, 1, True, "strided", 300.0, None),
    "k17_one_step": (257, 17, 1, 2.0, True, 1, True, "out", 300.0, None),
    "k127_one_step": (257, 127, 1, 1.5, True, 3, False, "out", 300.0, None),
    "k128": (257, 128, 2, 2.0, True, 1, True, "inplace", 300.0, None),
    "k128_one_step": (257, 128, 1, 2.0, True, 1, True, "strided", 300.0, None),
    "station_only": (257, 17, 2, 2.0, False, 1, True, "out", 300.0, None),
    "station_only_inplace": (129, 9, 16, 2.0, False, 3, False, "inplace", 300.0, None),
    "nothing_in_reach": (129, 9, 2, 2.0, True, 1, True, "out", 0.01, "far"),
    "signed_zero": (129, 9, 1, 2.0, True, 1, True, "out", 300.0, "zero"),
    "nan_bias": (129, 9, 2, 2.0, True, 3, True, "out", 300.0, "nan"),
    # K points at one place, a row at that place, one 44 m north of it and one far away: every distance in reach is
    # clamped to 0.1 km, so every raw weight is the same IEEE value on both sides (d, or d * d rounded once), their numpy
    # sum and w / wsum are the same correctly rounded operations, and with biases over twelve decades the bits of a
    # one-step field are numpy's pairwise order of the terms and nothing else: bit-equal
    "stack8_one_step": (11, 8, 1, 2.0, True, 1, True, "out", 1.0, "stack"),
    "stack9_one_step": (12, 9, 1, 1.0, True, 3, True, "strided", 1.0, "stack"),
    "stack16_one_step": (19, 16, 1, 1.0, True, 1, True, "inplace", 1.0, "stack"),
    "stack17_one_step": (20, 17, 1, 2.0, True, 1, True, "out", 1.0, "stack"),
    "stack17_two_steps": (20, 17, 2, 2.0, True, 1, True, "out", 1.0, "stack"),  # numpy's axis-0 sum: point by point
}
WANT_NMASK = (0, 1, 7, 8, 9, 16)


def hav_np(la1, lo1, la2, lo2):
    """Vectorised haversine (km), for placing rows only: every reference distance comes from mos_ref."""
    r = math.pi / 180.0
    a = np.sin((la2 - la1) * r / 2) ** 2 + np.cos(la1 * r) * np.cos(la2 * r) * np.sin((lo2 - lo1) * r / 2) ** 2
    return 6371.0 * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))


def idw_geometry(G, K, radius, seed, near):
    """(lat, lon, pt_idx): K points within a degree of (56 N, 92 E), so that a row among them sees all of them; of the
    other rows one shares a point's coordinates (d = 0) and one lies 44 m north of a point (both under the 0.1 km
    clamp, neither the point's own row), one per count in WANT_NMASK and one for K sit along a ray from the centre where
    exactly that many points are within the radius, and the rest are scattered over ten degrees, every ninth far away."""
    rng = np.random.default_rng(seed)
    pt_idx = rng.permutation(G)[:K].astype(np.int32)
    lat, lon = C_LAT + 10 * (rng.random(G) - 0.5), C_LON + 10 * (rng.random(G) - 0.5)
    lat[::9] -= 60
    lat[pt_idx], lon[pt_idx] = C_LAT + 2 * (rng.random(K) - 0.5), C_LON + 2 * (rng.random(K) - 0.5)
    free = [g for g in range(G) if g not in set(pt_idx.tolist())]
    if near and len(free) >= 2:
        g0, g1 = free.pop(0), free.pop(0)
        lat[g0], lon[g0] = lat[pt_idx[0]], lon[pt_idx[0]]
        lat[g1], lon[g1] = lat[pt_idx[K - 1]] + 0.0004, lon[pt_idx[K - 1]]
    s = np.arange(0.0, 12.0, 0.002)
    rla, rlo = C_LAT + s * math.cos(0.7), C_LON + s * math.sin(0.7)
    count = (hav_np(rla[:, None], rlo[:, None], lat[pt_idx][None, :], lon[pt_idx][None, :]) < radius).sum(axis=1)
    for m in sorted(set(WANT_NMASK + (K,))):
        hit = np.flatnonzero(count == m)
        if m <= K and len(hit) and free:
            g = free.pop(0)
            i = hit[len(hit) // 2]
            lat[g], lon[g] = rla[i], rlo[i]
    return lat, lon, pt_idx


@functools.lru_cache(maxsize=None)
def idw_case(name):
    G, K, steps, power, idw, B, f64, _, radius, kind = IDW[name]
    seed = sum(map(ord, name))
    rng = np.random.default_rng(seed)
    lat, lon, pt_idx = idw_geometry(G, K, radius, seed + 1, kind != "far")
    bias = 2 * rng.standard_normal((B, K, steps))
    if kind == "stack":
        pt_idx = np.arange(K, dtype=np.int32)
        lat, lon = np.full(G, C_LAT + 0.37), np.full(G, C_LON - 1.21)
        lat[K + 1] += 0.0004  # 44 m
        lat[K + 2] -= 30.0
        bias = rng.choice((-1.0, 1.0), bias.shape) * 10.0 ** rng.uniform(-6, 6, bias.shape)
    if kind == "zero":
        bias[:] = -0.0
    if kind == "nan":
        bias[0, 3, 1] = np.nan
    dists, own = R.idw_dists(lat, lon, pt_idx)
    x = rng.standard_normal((B, G, steps, IDW_C))
    x[..., T2M] = 265 + 15 * x[..., T2M]
    if f64:  # x = 0 off the points' own rows: out - x is the field exactly
        x[..., T2M][:, own < 0] = -0.0 if kind == "zero" else 0.0
    x = x.astype(np.float64 if f64 else np.float32)
    field = np.zeros((B, G, steps))
    ld_field = np.zeros((B, G, steps), dtype=np.longdouble)
    mag = np.zeros((B, G, steps), dtype=np.longdouble)
    for b in range(B):
        field[b], nmask = R.idw_field(dists, own, bias[b], power, radius)
        ld_field[b], mag[b], ld_d = R.idw_field_ld(lat, lon, pt_idx, bias[b], power, radius)
    with np.errstate(invalid="ignore"):
        n_idw = [int((np.abs(field[b]).max(axis=1) > 1e-6).sum()) for b in range(B)]
    return dict(lat=lat, lon=lon, pt_idx=pt_idx, bias=bias, x=x, own=own, dists=dists, nmask=nmask, field=field,
                ld_field=ld_field, mag=mag, ld_d=ld_d, n_idw=n_idw)


def field_ratio(got, c, power):
    """|got - longdouble field| / (eps (1 + power) sum_k |w_k b_k|) where the sum is not zero or NaN."""
    ok = (c["mag"] > 0) & (c["own"] < 0)[None, :, None]
    err = np.abs(got.astype(np.longdouble) - c["ld_field"])
    return float((err[ok] / (EPS * (1 + power) * c["mag"][ok])).max(initial=0))


@functools.lru_cache(maxsize=None)
def idw_c():
    """The constant of the float64 field's bound: four times the worst ratio of the numpy float64 restatement against
    the longdouble one over this file's cases, at least 8."""
    worst = max(field_ratio(idw_case(n)["field"], idw_case(n), IDW[n][3]) for n in IDW if IDW[n][4])
    return max(8.0, 4.0 * worst), worst


def test_idw_inputs_leave_the_bounds_to_the_kernel():
    """CPU: on the longdouble restatement no distance lies within 1e-9 radius of the radius or within 1e-12 of the
    0.1 km clamp, and no row's max |field| within 1e-9 of the 1e-6 counting threshold (rows of zeros aside), with no
    case or row left out; the rows see every count in WANT_NMASK, K and the clamp; float64 numpy agrees with
    longdouble on every mask."""
    seen, clamped = set(), 0
    for name, (G, K, steps, power, idw, B, f64, _, radius, kind) in IDW.items():
        c = idw_case(name)
        d = c["ld_d"][c["own"] < 0].astype(np.float64)
        if d.size:
            assert np.abs(d - radius).min() > 1e-9 * radius, name
            assert np.abs(d - 0.1).min() > 1e-12, name
            assert np.array_equal(d < radius, c["dists"][c["own"] < 0] < radius)
        top = np.nanmax(np.abs(c["ld_field"]).astype(np.float64), axis=2)
        top = top[(top != 0) & ~np.isnan(c["field"]).any(axis=2)]
        assert top.size == 0 or np.abs(top - 1e-6).min() > 1e-9, name
        if kind == "stack":
            assert c["nmask"].tolist() == [-1] * K + [K, K, 0] and np.nanmax(c["dists"][K:K + 2]) < 0.1, name
            assert c["dists"][K].tolist() == [0.0] * K
        if idw:
            seen |= {(int(m), int(m) == K) for m in c["nmask"] if m >= 0}
            clamped += int(((c["dists"] < 0.1) & (c["own"] < 0)[:, None]).sum())
    assert {m for m, _ in seen} >= set(WANT_NMASK) and any(full for _, full in seen)
    assert clamped >= 2 * sum(1 for n in IDW if IDW[n][4] and IDW[n][0] - IDW[n][1] >= 2 and IDW[n][9] != "far")
    assert (idw_case("nothing_in_reach")["nmask"] <= 0).all()
    z = idw_case("signed_zero")
    assert 8 in z["nmask"] and not np.signbit(z["field"][:, z["own"] < 0]).any()  # numpy sums eight -0.0 to +0.0
    cc, worst = idw_c()
    print(f"[MOS kernels] numpy float64 against longdouble: worst ratio {worst:.3f}, so c = {cc:.1f}")


@gpu
@pytest.mark.parametrize("name", list(IDW))
def test_idw_apply(hip, name):
    G, K, steps, power, idw, B, f64, place, radius, kind = IDW[name]
    c = idw_case(name)
    dt = torch.float64 if f64 else torch.float32
    x = dev(c["x"])
    X = Field4.of(x)
    O = X if place == "inplace" else Field4(B, G, steps, IDW_C, dt, pad=place == "strided", fill=SENT)
    lat, lon = Guarded((G,), torch.float64, fill=NAN, init=dev(c["lat"])), Guarded((G,), torch.float64, fill=NAN,
                                                                                   init=dev(c["lon"]))
    bias = Guarded((B, K, steps), torch.float64, fill=NAN, init=dev(c["bias"]))
    nc = Guarded((B,), torch.int32, fill=-7, init=torch.zeros(B, dtype=torch.int32, device=DEV))
    pt = dev(c["pt_idx"])

    def call(k=K):
        hip._check(hip.lib().gcl_mos_idw_apply(
            X.ptr, int(f64), *X.strides, O.ptr, *O.strides, G, steps, IDW_C, T2M, ptr_of(lat), ptr_of(lon),
            pt.data_ptr(), k, ptr_of(bias), int(idw), power, radius, ptr_of(nc), B, hip._stream()))

    _, names = launched(call)
    assert has(names, "idw_apply_kernel")
    assert O.untouched() and X.untouched() and nc.untouched()
    out = O.view.cpu().numpy()
    others = [ch for ch in range(IDW_C) if ch != T2M]
    assert np.array_equal(bits(out[..., others]), bits(c["x"][..., others])), "the other channels are not copied"
    if place != "inplace":
        assert same_bits(X.view, x)
    own = c["own"] >= 0
    x64 = c["x"][..., T2M].astype(np.float64)
    want_own = (x64[:, own] + c["bias"][:, c["own"][own]]).astype(c["x"].dtype)
    t2m_out = out[..., T2M]
    assert np.array_equal(bits(t2m_out[:, own]), bits(want_own)), "an own row is not x + bias"
    got, xin = t2m_out[:, ~own], c["x"][..., T2M][:, ~own]
    if not idw:
        assert np.array_equal(bits(got), bits(xin)), "station-only: a row without a point changed"
        assert nc.view.tolist() == [K] * B
    else:
        want = x64[:, ~own] + c["field"][:, ~own]
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert nc.view.tolist() == c["n_idw"]
        if kind == "zero":
            assert np.array_equal(bits(got), bits(want)), "eight -0.0 terms do not sum to numpy's +0.0"
        elif kind == "stack":
            assert np.array_equal(bits(got), bits(want)), "equal weights: the field's bits are numpy's order of the sum"
        elif not f64:
            ulp = np.abs(bits(got).astype(np.int64) - bits(want.astype(np.float32)).astype(np.int64))
            assert ulp[~np.isnan(want)].max(initial=0) <= 1
        else:
            unreached = (c["mag"][:, ~own] == 0)
            assert np.array_equal(bits(got[unreached]), bits(want[unreached]))
            field = np.zeros_like(c["field"])
            field[:, ~own] = got
            ratio = field_ratio(field, c, power)  # (NaN entries, checked above, have no magnitude and stay out)
            cc, _ = idw_c()
            W_.worst["idw float64 field"] = max(W_.worst.get("idw float64 field", 0.0), ratio / cc)
            W_.worst["idw float64 field, in units of eps (1 + power) sum |w b|"] = max(
                W_.worst.get("idw float64 field, in units of eps (1 + power) sum |w b|", 0.0), ratio)
            assert ratio <= cc, f"{name}: the field is {ratio:.2f} eps (1 + power) sum |w b| from longdouble, c = {cc}"
    if name == "k8":
        with pytest.raises(RuntimeError, match="129 station points"):
            call(KMAX + 1)
    W_.report("idw float64 field", "idw float64 field, in units of eps (1 + power) sum |w b|")


# ------------------------------------------------------------------------------------------------------------------
# IDW sweep: more than 256 block partials
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nblk,f64", [(257, False), (513, True)])
def test_idw_sweep_block_partials_past_256(hip, nblk, f64):
    """G = 64 (nblk - 1) + 1 rows of one sample: idw_sweep_final_kernel's threads take a second (and third) partial."""
    G, K, steps, H = 64 * (nblk - 1) + 1, 3, 2, 5
    rng = np.random.default_rng(nblk)
    dt = torch.float64 if f64 else torch.float32
    lat, lon = C_LAT + 6 * (rng.random(G) - 0.5), C_LON + 6 * (rng.random(G) - 0.5)
    pt = np.array([5, G // 2, G - 1], dtype=np.int32)
    x = rng.standard_normal((1, G, steps, 2))
    x[..., 0] = 265 + 15 * x[..., 0]
    pred = Field4.of(dev(x, dt))
    truth = dev(x[..., 0] + rng.standard_normal((1, G, steps)), dt)
    bias = dev(2 * rng.standard_normal((1, K, steps)))
    power, radius = dev([2.0, 1.5]), dev([300.0, 150.0])
    P = 2
    acc = torch.full((P, H), 0.25, dtype=torch.float64, device=DEV)
    fields = torch.empty(P, 1, G, steps, dtype=dt, device=DEV)

    def call(h0):
        hip.mos_idw_sweep(pred.view, truth, 0, dev(lat), dev(lon), dev(pt), bias, True, power, radius, acc, h0,
                          fields_out=fields)

    _, names = launched(lambda: call(0))
    assert has(names, "idw_sweep_final_kernel") and pred.untouched()
    assert hip.lib().gcl_mos_idw_sweep_ws_bytes(G, P, steps, 1) == nblk * P * steps * 8
    first = acc.clone()
    d = fields[:, 0] - truth  # the squared errors in the forecast's type, each operation rounded on its own
    e = (d * d).double().cpu().numpy()
    for p in range(P):
        for s in range(steps):
            tot = math.fsum(e[p, :, s])
            err = abs(first[p, s].item() - (0.25 + tot))
            W_.worst["sweep acc"] = max(W_.worst.get("sweep acc", 0.0), err / (G * EPS * tot))
            assert err <= G * EPS * tot, (p, s, first[p, s].item(), tot)
    assert (first[:, steps:] == 0.25).all()
    call(2)
    torch.cuda.synchronize()
    assert same_bits(acc[:, :2], first[:, :2]) and same_bits(acc[:, 2:4], first[:, :2]) and (acc[:, 4] == 0.25).all()
    W_.report("sweep acc")


# ------------------------------------------------------------------------------------------------------------------
# Table MOS
# ------------------------------------------------------------------------------------------------------------------
TABLE = {  # B, G, steps, C, in place, float64, nvalid, padded rows
    # 256 * 8192 + 256 * 3 + 5 elements: 8196 blocks wanted, 8192 launched, the first 773 threads take a second trip
    "past_cap_by_773": (1, 83917, 5, 5, False, False, 5, True),
    "same_rows_in_place": (1, 83917, 5, 5, True, True, 1, True),  # per = steps: 1640 blocks
    "two_full_trips": (2, 8192, 16, 16, False, False, 16, False),  # 2 * 8192 * 256 elements
    "no_valid_step": (3, 300, 4, 3, False, True, 0, True),
    "one_valid_step_in_place": (3, 300, 4, 3, True, False, 1, True),
}


@gpu
@pytest.mark.parametrize("name", list(TABLE))
def test_table_apply(hip, name):
    B, G, steps, C, inplace, f64, nvalid, pad = TABLE[name]
    dt = torch.float64 if f64 else torch.float32
    t2m = C - 2
    g = torch.Generator(device=DEV).manual_seed(len(name))
    x = torch.randn(B, G, steps, C, generator=g, device=DEV, dtype=dt) * 15 + 265
    tb = Guarded((steps,), torch.float64, fill=NAN, init=dev(np.random.default_rng(3).standard_normal(steps) * 1.7))
    want = x.clone()
    add = tb.view if f64 else tb.view.float()
    want[:, :, :nvalid, t2m] = x[:, :, :nvalid, t2m] + add[:nvalid]
    X = Field4.of(x, pad=pad)
    O = X if inplace else Field4(B, G, steps, C, dt, pad=pad, fill=SENT)
    _, names = launched(lambda: hip._check(hip.lib().gcl_mos_table_apply(
        X.ptr, int(f64), *X.strides, O.ptr, *O.strides, G, steps, C, t2m, ptr_of(tb), nvalid, B, hip._stream())))
    assert has(names, "table_apply_kernel")
    assert O.untouched() and X.untouched() and same_bits(O.view, want)
    if not inplace:
        assert same_bits(X.view, x)
    W_.exact("table_apply")


@gpu
def test_table_apply_of_no_rows_launches_nothing(hip):
    """G = 0: the entry point returns before the launch, and so does apply_mos_t2m, whose empty views have null
    data_ptr()s that the entry point would refuse."""
    from torch.profiler import ProfilerActivity, profile

    from graphcast_lite_amd import mos

    X, O = Field4(2, 0, 3, 4), Field4(2, 0, 3, 4, fill=SENT)
    tb = torch.ones(3, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        hip._check(hip.lib().gcl_mos_table_apply(X.ptr, 0, *X.strides, O.ptr, *O.strides, 0, 3, 4, 1, tb.data_ptr(), 3,
                                                 2, hip._stream()))
        torch.cuda.synchronize()
    assert not [e.name for e in prof.events() if "table_apply" in e.name]
    assert O.untouched() and X.untouched()
    from datetime import datetime

    out = mos.apply_mos_t2m(torch.zeros(0, 3, 4, device=DEV), ["u10", "t2m", "v10", "sp"],
                            {"bias_table": {"1": {"0": 1.0}}}, [datetime(2024, 1, 1, 0)])
    assert out.shape == (0, 3, 4)
