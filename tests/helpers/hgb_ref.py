"""A float64 numpy restatement of histogram gradient boosting for squared error without missing values: the steps
the kernels of csrc/mos_fit.hip carry (binning, gradients, histogram, best split, stable partition, best-first tree
growth), written from sklearn's rules.  tests/test_mos_fit.py checks it against sklearn's own forests in the fixture;
the kernel tests then use it as their yardstick."""
import heapq

import numpy as np


def bin_rows(X, thresholds):
    """uint8 [F, n]: bin = number of thresholds below the value (a value on a threshold goes left)."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([np.searchsorted(np.asarray(t, dtype=np.float64), X[:, f], side="left").astype(np.uint8)
                     for f, t in enumerate(thresholds)])


def gradients(raw, y):
    return (np.asarray(raw, dtype=np.float64) - np.asarray(y, dtype=np.float64)).astype(np.float32)


def histogram(bins, rows, g):
    """(sum float64 [F, 256], count uint32 [F, 256]) over `rows`, each bin's rows added in order."""
    F = bins.shape[0]
    gs = g[rows].astype(np.float64)
    hs = np.stack([np.bincount(bins[f, rows], weights=gs, minlength=256) for f in range(F)])
    hc = np.stack([np.bincount(bins[f, rows], minlength=256) for f in range(F)]).astype(np.uint32)
    return hs, hc


def value(g, h, l2):
    return -g / (h + l2 + 1e-15)


def best_split(hs, hc, nthr, n, G, min_samples_leaf, l2):
    """dict(gain, feature, bin, n_left, sum_g_left, missing_left); gain = -1.0 when no split is valid.  The left sums
    are formed bin after bin (np.cumsum adds in order); a later candidate wins only with a strictly larger gain."""
    nthr = np.asarray(nthr)
    nl = np.cumsum(hc.astype(np.int64), axis=1)
    gl = np.cumsum(hs, axis=1)
    gr = G - gl
    with np.errstate(all="ignore"):
        gain = G * value(G, float(n), l2) - gl * value(gl, nl.astype(np.float64), l2)
        gain = gain - gr * value(gr, float(n) - nl.astype(np.float64), l2)
    ok = (np.arange(hs.shape[1])[None, :] < nthr[:, None]) & (nl >= min_samples_leaf) & (n - nl >= min_samples_leaf)
    gain = np.where(ok & (gain > 0.0), gain, -1.0)
    b = np.argmax(gain, axis=1)  # the first of equal maxima: the lowest bin
    per_feature = gain[np.arange(hs.shape[0]), b]
    f = int(np.argmax(per_feature))  # ... and the lowest feature
    best = dict(gain=float(per_feature[f]), feature=f, bin=int(b[f]), n_left=0, sum_g_left=0.0, missing_left=0)
    if best["gain"] > 0:
        best["n_left"], best["sum_g_left"] = int(nl[f, b[f]]), float(gl[f, b[f]])
        best["missing_left"] = int(best["n_left"] > n - best["n_left"])
    else:
        best["feature"] = best["bin"] = 0
    return best


def partition(bins, rows, feature, b):
    """Stable: (left rows, right rows) in their old order."""
    left = bins[feature, rows] <= b
    return rows[left], rows[~left]


class _Node:
    def __init__(self, rows, depth, G):
        self.rows, self.depth, self.G = rows, depth, G
        self.split = self.left = self.right = self.hist = None
        self.leaf = False
        self.value = 0.0


def grow_tree(bins, nthr, thresholds, g, max_leaf_nodes=31, max_depth=8, min_samples_leaf=20, l2=0.1,
              learning_rate=0.05, rows=None, gains=None):
    """One tree, best-first.  Returns (nodes, leaves): nodes a list of dicts in creation order (children after their
    parent) with feature / threshold / bin / left / right / missing_left / is_leaf / value, leaves a list of (rows,
    value)."""
    n = bins.shape[1]
    rows = np.arange(n) if rows is None else rows
    hs, hc = histogram(bins, rows, g)
    root = _Node(rows, 0, float(np.cumsum(hs[0])[-1]))  # feature 0's bins added in order
    root.value = value(root.G, float(len(rows)), l2)
    root.hist = (hs, hc)
    order, heap, tick = [root], [], 0

    def push(node):
        nonlocal tick
        node.split = best_split(node.hist[0], node.hist[1], nthr, len(node.rows), node.G, min_samples_leaf, l2)
        if node.split["gain"] <= 0:
            node.leaf = True
        else:
            heapq.heappush(heap, (-node.split["gain"], tick, node))
            tick += 1
            if gains is not None:
                gains.append(node.split["gain"])

    if len(rows) < 2 * min_samples_leaf:
        root.leaf = True
    else:
        push(root)
    while heap:
        _, _, node = heapq.heappop(heap)
        sp = node.split
        lrows, rrows = partition(bins, node.rows, sp["feature"], sp["bin"])
        assert len(lrows) == sp["n_left"]
        L = _Node(lrows, node.depth + 1, sp["sum_g_left"])
        R = _Node(rrows, node.depth + 1, node.G - sp["sum_g_left"])
        L.value = value(L.G, float(len(lrows)), l2)
        R.value = value(R.G, float(len(node.rows)) - float(len(lrows)), l2)
        node.left, node.right = L, R
        order += [L, R]
        n_leaves = sum(1 for k in order if k.left is None)
        if n_leaves == max_leaf_nodes:
            L.leaf = R.leaf = True
            for _, _, k in heap:
                k.leaf = True
            heap = []
            break
        if L.depth == max_depth:
            L.leaf = R.leaf = True
            continue
        L.leaf, R.leaf = len(lrows) < 2 * min_samples_leaf, len(rrows) < 2 * min_samples_leaf
        if not (L.leaf and R.leaf):
            small, large = (L, R) if len(lrows) < len(rrows) else (R, L)
            small.hist = histogram(bins, small.rows, g)
            large.hist = (node.hist[0] - small.hist[0], node.hist[1] - small.hist[1])
            if not L.leaf:
                push(L)
            if not R.leaf:
                push(R)
        node.hist = None
    idx = {id(k): i for i, k in enumerate(order)}
    nodes, leaves = [], []
    for k in order:
        if k.left is None:
            v = k.value * learning_rate
            nodes.append(dict(is_leaf=1, value=v, feature=0, bin=0, threshold=0.0, left=0, right=0, missing_left=0))
            leaves.append((k.rows, v))
        else:
            sp = k.split
            nodes.append(dict(is_leaf=0, value=0.0, feature=sp["feature"], bin=sp["bin"],
                              threshold=float(thresholds[sp["feature"]][sp["bin"]]), left=idx[id(k.left)],
                              right=idx[id(k.right)], missing_left=sp["missing_left"]))
    return nodes, leaves


def walk_binned(nodes, bins_col):
    """Leaf value of one row given its bins [F]."""
    k = 0
    while not nodes[k]["is_leaf"]:
        k = nodes[k]["left"] if bins_col[nodes[k]["feature"]] <= nodes[k]["bin"] else nodes[k]["right"]
    return nodes[k]["value"]


def fit(X, y, thresholds, n_iter, X_val=None, y_val=None, **kw):
    """n_iter boosting iterations.  Returns dict(trees=[nodes, ...], baseline, raw, scores)."""
    y = np.asarray(y, dtype=np.float64)
    bins = bin_rows(X, thresholds)
    nthr = [len(t) for t in thresholds]
    baseline = float(np.mean(y))
    raw = np.full(y.shape, baseline)
    scores, raw_v, bins_v = [], None, None
    if X_val is not None:
        bins_v = bin_rows(X_val, thresholds)
        raw_v = np.full(len(y_val), baseline)
        scores.append(-0.5 * float(np.mean((raw_v - y_val) ** 2)))
    trees = []
    for _ in range(n_iter):
        g = gradients(raw, y)
        nodes, leaves = grow_tree(bins, nthr, thresholds, g, **kw)
        for rows, v in leaves:
            raw[rows] += v
        if X_val is not None:
            raw_v += np.array([walk_binned(nodes, bins_v[:, i]) for i in range(bins_v.shape[1])])
            scores.append(-0.5 * float(np.mean((raw_v - y_val) ** 2)))
        trees.append(nodes)
    return dict(trees=trees, baseline=baseline, raw=raw, scores=np.array(scores))


def flatten(trees):
    """The trees as MOSForest arrays (global child indices)."""
    cols = {k: [] for k in ("feature", "value", "left", "right", "missing_left", "is_leaf")}
    roots, off = [], 0
    for nodes in trees:
        roots.append(off)
        for nd in nodes:
            leaf = nd["is_leaf"]
            cols["feature"].append(nd["feature"])
            cols["value"].append(nd["value"] if leaf else nd["threshold"])
            cols["left"].append(0 if leaf else nd["left"] + off)
            cols["right"].append(0 if leaf else nd["right"] + off)
            cols["missing_left"].append(nd["missing_left"])
            cols["is_leaf"].append(leaf)
        off += len(nodes)
    return {k: np.asarray(v) for k, v in cols.items()}, np.asarray(roots)


def same_forest(a, a_roots, b, b_roots, rtol=1e-12):
    """Walk two flattened forests (dicts of MOSForest arrays) from each root: structure, features, threshold bits,
    missing_left and leaf flags equal, leaf values within rtol relative.  Returns a list of differences."""
    bad = []
    if len(a_roots) != len(b_roots):
        return [f"{len(a_roots)} trees against {len(b_roots)}"]
    for t, (ra, rb) in enumerate(zip(a_roots, b_roots)):
        stack = [(int(ra), int(rb))]
        while stack:
            i, j = stack.pop()
            la, lb = int(a["is_leaf"][i]), int(b["is_leaf"][j])
            if la != lb:
                bad.append(f"tree {t}: leaf flag {la} against {lb} at nodes {i} / {j}")
                continue
            va, vb = float(a["value"][i]), float(b["value"][j])
            if la:
                if abs(va - vb) > rtol * max(abs(va), abs(vb)):
                    bad.append(f"tree {t}: leaf value {va!r} against {vb!r}")
                continue
            if int(a["feature"][i]) != int(b["feature"][j]) or np.float64(va).tobytes() != np.float64(vb).tobytes() \
                    or int(a["missing_left"][i]) != int(b["missing_left"][j]):
                bad.append(f"tree {t}: split (f{int(a['feature'][i])}, {va!r}, {int(a['missing_left'][i])}) against "
                           f"(f{int(b['feature'][j])}, {vb!r}, {int(b['missing_left'][j])})")
                continue
            stack.append((int(a["left"][i]), int(b["left"][j])))
            stack.append((int(a["right"][i]), int(b["right"][j])))
        if len(bad) > 5:
            break
    return bad
