"""Synthetic forests and float64 restatements of csrc/mos.hip's header comments, for tests/test_mos_kernels.py: the
sklearn walk, the station recurrence with numpy's own mean, and the IDW spread line for line as the reference's
mos_correction.py orders it (math haversine per pair, numpy for every sum)."""
import math

import numpy as np

NUM_FEAT = 20
ALWAYS_NAN = (1, 6, 7, 14)  # dewpoint, cloud cover, radiation, dewpoint depression: never available
TIME_COLS = (9, 10, 11, 12, 13, 17, 18, 19)  # where the eight host features go
# centre and scale of each feature's values, so that thresholds drawn from them send rows both ways
CENTRE = np.array([-8, 0, 7, 0, 0, 950, 0, 0, 1e-3, 0, 0, 0, 0, 0, 0, -8, 0, 0, 0, 0], dtype=np.float64)
SCALE = np.array([15, 1, 5, .7, .7, 30, 1, 1, 1e-3, 1, 1, 1, 1, 1, 1, 15, 20, 1, 1, 1], dtype=np.float64)
POOL = 8  # thresholds per feature: few, so that a feature can be set equal to one


def pools(seed):
    rng = np.random.default_rng(seed)
    return CENTRE[:, None] + SCALE[:, None] * rng.standard_normal((NUM_FEAT, POOL))


def synth_forest(ntrees, seed, zero=False):
    """A seeded forest as MOSForest's flat arrays: trees of depth 0 (the root is a leaf) to 6, splits on every feature
    (0 and 19 most often) with thresholds from `pools(seed)`, both missing directions, leaf values of either sign over
    twelve decades.  `zero`: the baseline and every leaf are -0.0."""
    rng = np.random.default_rng(seed)
    pool = pools(seed)
    feat, val, left, right, miss, leaf, roots = [], [], [], [], [], [], []
    fprob = np.full(NUM_FEAT, 1.0)
    fprob[[0, 19]] = 4.0
    fcum = np.cumsum(fprob / fprob.sum())

    def node(depth, u):
        i = len(val)
        r = u[i - roots[-1]]  # one row of uniform draws per node of the tree (at most 127)
        feat.append(0), left.append(0), right.append(0), miss.append(0)
        if depth == 0 or r[0] < 0.25:
            leaf.append(1)
            val.append(-0.0 if zero else (1.0 if r[1] < 0.5 else -1.0) * 10.0 ** (12.0 * r[2] - 6.0))
            return i
        leaf.append(0)
        f = min(int(np.searchsorted(fcum, r[1])), NUM_FEAT - 1)
        feat[i], miss[i] = f, int(r[2] < 0.5)
        val.append(float(pool[f, int(r[3] * POOL)]))
        left[i] = node(depth - 1, u)
        right[i] = node(depth - 1, u)
        return i

    depths = rng.integers(1, 7, ntrees)
    for t in range(ntrees):
        roots.append(len(val))
        node(0 if t % 5 == 3 else int(depths[t]), rng.random((127, 4)))
    return dict(feature=np.array(feat, np.int32), value=np.array(val), left=np.array(left, np.int64),
                right=np.array(right, np.int64), missing_left=np.array(miss, np.uint8), is_leaf=np.array(leaf, np.uint8),
                roots=np.array(roots, np.int32), baseline=-0.0 if zero else float(rng.standard_normal()))


def walk(fr, X, gap_feats=(), stats=None):
    """sklearn's prediction of rows X [n, 20] in float64: NaN follows missing_go_to_left, otherwise x <= threshold goes
    left; the raw prediction is ((baseline + v0) + v1) + ... in tree order (a cumulative sum adds strictly left to
    right).  All (row, tree) walks advance together, one level per trip.  Also returns the smallest |x - threshold| met
    at a split on one of `gap_feats`; `stats` counts what the walks met: a NaN sent left / right, a feature equal to its
    threshold, an infinite feature."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    node = np.broadcast_to(fr["roots"].astype(np.int64), (n, fr["roots"].size)).copy()
    rows = np.arange(n)[:, None]
    gap = math.inf
    while True:
        active = fr["is_leaf"][node] == 0
        if not active.any():
            break
        f = fr["feature"][node]
        x = X[rows, f]
        thr = fr["value"][node]
        with np.errstate(invalid="ignore"):
            go_left = np.where(np.isnan(x), fr["missing_left"][node] != 0, x <= thr)
            if stats is not None:
                nanx = active & np.isnan(x)
                for key, m in (("nan_left", nanx & go_left), ("nan_right", nanx & ~go_left), ("equal", active & (x == thr)),
                               ("inf", active & np.isinf(x))):
                    stats[key] = stats.get(key, 0) + int(m.sum())
            for gf in gap_feats:
                m = active & (f == gf) & np.isfinite(x)
                if m.any():
                    gap = min(gap, float(np.abs(x[m] - thr[m]).min()))
        node = np.where(active, np.where(go_left, fr["left"][node], fr["right"][node]), node)
    leaves = fr["value"][node]
    raw = np.cumsum(np.concatenate([np.full((n, 1), fr["baseline"]), leaves], axis=1), axis=1)[:, -1]
    return raw, gap


def station_features(vals, chans, tf, prev):
    """_build_features_from_forecast in float64: `vals` one forecast row of one step, chans = (t2m, u, v, sp, tp)
    channel indices (-1: absent), tf the eight host features, prev the lagged corrected t2m (None at step 0)."""
    nan = float("nan")

    def get(c):
        return float(vals[c]) if c >= 0 else nan

    t2m_c = get(chans[0]) - 273.15
    u, v = get(chans[1]), get(chans[2])
    bad = math.isnan(u) or math.isnan(v)
    ws = nan if bad else math.sqrt(u ** 2 + v ** 2)
    wd = nan if bad else math.atan2(-u, -v)
    sp = get(chans[3])
    sp = sp / 100.0 if not math.isnan(sp) else nan
    f = np.full(NUM_FEAT, nan)
    f[0], f[2], f[5], f[8] = t2m_c, ws, sp, get(chans[4])
    if not bad:
        f[3], f[4] = math.sin(wd), math.cos(wd)
    f[list(TIME_COLS)] = tf
    if prev is not None:
        f[15], f[16] = prev, t2m_c - prev
    return f


def station_recurrence(fr, pred, chans, grid_idx, gstart, tfeat):
    """(bias [B, groups, steps], features [B, stations, steps, 20], smallest gap of features 3 / 4 to a threshold) of
    mos_correction.py:307-323: per group the steps in order, the group mean is numpy's own np.mean of the stations'
    predictions, and the lag of the next step is the corrected t2m."""
    B, _, steps, _ = pred.shape
    ng, nst = len(grid_idx), int(gstart[-1])
    bias = np.zeros((B, ng, steps))
    feats = np.zeros((B, nst, steps, NUM_FEAT))
    gap = math.inf
    for b in range(B):
        for g in range(ng):
            prev = None
            for s in range(steps):
                vals = pred[b, grid_idx[g], s]
                X = np.array([station_features(vals, chans, tfeat[b, q, s], prev) for q in range(gstart[g], gstart[g + 1])])
                feats[b, gstart[g]:gstart[g + 1], s] = X
                y, gp = walk(fr, X, (3, 4))
                gap = min(gap, gp)
                bias[b, g, s] = float(np.mean(list(y)))
                prev = float(float(vals[chans[0]]) + bias[b, g, s]) - 273.15
    return bias, feats, gap


def haversine_km(lat1, lon1, lat2, lon2):
    R = 6371.0
    dlat = math.radians(lat2 - lat1)
    dlon = math.radians(lon2 - lon1)
    a = (math.sin(dlat / 2) ** 2 + math.cos(math.radians(lat1)) * math.cos(math.radians(lat2)) * math.sin(dlon / 2) ** 2)
    return R * 2 * math.atan2(math.sqrt(a), math.sqrt(1 - a))


def idw_dists(lat, lon, pt_idx):
    """(dists [G, K] of every row to every point, NaN on a point's own row; own [G]: the row's point or -1)."""
    G, K = len(lat), len(pt_idx)
    first = {}
    for k, g in enumerate(pt_idx):
        first.setdefault(int(g), k)
    own = np.array([first.get(g, -1) for g in range(G)])
    dists = np.full((G, K), np.nan)
    for g in range(G):
        if own[g] < 0:
            dists[g] = [haversine_km(float(lat[g]), float(lon[g]), float(lat[i]), float(lon[i])) for i in pt_idx]
    return dists, own


def idw_field(dists, own, bias, power, radius):
    """_idw_interpolate_bias (mos_correction.py:209-241) for bias [K, steps] on distances already taken: (field
    [G, steps], nmask [G], -1 on a point's own row)."""
    G, steps = len(own), bias.shape[1]
    field = np.zeros((G, steps))
    nmask = np.full(G, -1, dtype=np.int64)
    for g in range(G):
        if own[g] >= 0:
            field[g, :] = bias[own[g]]
            continue
        mask = dists[g] < radius
        nmask[g] = int(mask.sum())
        if not mask.any():
            continue
        d = dists[g][mask]
        d = np.maximum(d, 0.1)
        w = 1.0 / d ** power
        w /= w.sum()
        field[g, :] = (w[:, None] * bias[mask]).sum(axis=0)
    return field, nmask


def idw_field_ld(lat, lon, pt_idx, bias, power, radius):
    """The same formulas in np.longdouble, vectorised: (field [G, steps], sum_k |w_k b_k| [G, steps], dists [G, K]); own
    rows hold the bias itself and NaN distances."""
    ld = np.longdouble
    lat, lon, bias = np.asarray(lat, ld), np.asarray(lon, ld), np.asarray(bias, ld)
    r = ld(math.pi) / ld(180)
    la1, lo1, la2, lo2 = lat[:, None], lon[:, None], lat[pt_idx][None, :], lon[pt_idx][None, :]
    a = np.sin((la2 - la1) * r / 2) ** 2 + np.cos(la1 * r) * np.cos(la2 * r) * np.sin((lo2 - lo1) * r / 2) ** 2
    d = ld(6371.0) * 2 * np.arctan2(np.sqrt(a), np.sqrt(1 - a))
    mask = d < ld(radius)
    w = np.where(mask, 1 / np.maximum(d, ld(0.1)) ** ld(power), ld(0))
    ws = w.sum(axis=1, keepdims=True)
    w = np.divide(w, ws, out=np.zeros_like(w), where=ws > 0)
    terms = np.where(mask[:, :, None], w[:, :, None] * bias[None, :, :], ld(0))  # an unreached NaN bias stays out
    field, mag = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    for k, g in reversed(list(enumerate(pt_idx))):
        field[g], mag[g], d[g] = bias[k], np.abs(bias[k]), np.nan
    return field, mag, d
