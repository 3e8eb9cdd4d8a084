"""numpy / scipy restatement of sicp_filter (include/sicp.h, "filtering a cloud", rules 1 - 8).  Imports nothing of the product.

The k-d tree only proposes candidates -- a few neighbours more than the list is long, or every pair inside a slightly larger
radius; the float32 arithmetic of the rules decides among them, and a query whose candidates might not hold its whole list is
redone against every point.  filter_slow() states the same rules once more without a tree, for the CPU tests to hold the fast
form against."""
import math

import numpy as np
from scipy.spatial import cKDTree

import cluster_ref

TREE_RUN = 512  # caller indices one workgroup of the tree sum reduces (the shapes the GPU tests straddle; no rule depends on it)
MAX_MEAN_K = 31
MAX_LABELS = 16


class TooFewPoints(ValueError):
    pass


def classes(xyz, labels, mask, drop, protect):
    """rule 1: (finite, removed, protected, tested) as boolean arrays over the caller's points"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    if set(int(v) for v in drop) & set(int(v) for v in protect):
        raise ValueError("a label in both lists")
    if labels is None and (len(drop) or len(protect)):
        raise ValueError("lists with a cloud without labels")
    finite = np.isfinite(xyz).all(axis=1)
    removed = ~finite
    if mask is not None:
        removed |= np.asarray(mask).reshape(n) == 0
    prot = np.zeros(n, bool)
    if labels is not None:
        lab = np.asarray(labels, np.uint32)
        if len(drop):
            removed |= np.isin(lab, np.asarray(list(drop), np.uint32))
        if len(protect):
            prot = np.isin(lab, np.asarray(list(protect), np.uint32)) & ~removed
    return finite, removed, prot, ~removed & ~prot


def _d2_rows(q, t):
    """float32 (dx dx + dy dy) + dz dz of every query against every target: [nq, nt]"""
    with np.errstate(over="ignore"):
        return cluster_ref.d2_f32(q[:, None, :], t[None, :, :])


def knn_d2(pts, queries, k):
    """the k smallest float32 squared distances from pts[queries] to pts, ascending: [len(queries), k].  The tree answers k + 16
    neighbours in double; they hold the float32 list when the list's last entry lies clearly inside the last candidate's
    distance, and the queries where it does not go against every point."""
    n, nq = len(pts), len(queries)
    out = np.empty((nq, k), np.float32)
    if nq == 0:
        return out
    kk = min(n, k + 16)
    p64 = pts.astype(np.float64)
    dist, idx = cKDTree(p64).query(p64[queries], k=kk)
    dist, idx = dist.reshape(nq, kk), idx.reshape(nq, kk)
    with np.errstate(over="ignore"):
        d2 = cluster_ref.d2_f32(pts[queries][:, None, :], pts[idx])
    d2 = np.sort(d2, axis=1)[:, :k]
    sure = np.full(nq, kk == n)
    if kk < n:
        sure = np.sqrt(d2[:, k - 1].astype(np.float64)) * (1.0 + 1e-5) < dist[:, kk - 1]
    out[:] = d2
    redo = np.flatnonzero(~sure)
    for a in range(0, len(redo), 64):
        rows = redo[a:a + 64]
        out[rows] = np.sort(_d2_rows(pts[queries[rows]], pts), axis=1)[:, :k]
    return out


def mean_dist_of_lists(d2, mean_k):
    """rule 3: the first entry left out, float32 roots, added to a double in ascending order, divided by (double)mean_k"""
    root = np.sqrt(d2[:, 1:mean_k + 1]).astype(np.float32)
    s = np.zeros(len(d2), np.float64)
    for k in range(mean_k):
        s = s + root[:, k].astype(np.float64)
    return s / float(mean_k)


def tree_sum(values, present, n_points):
    """rule 3: the sum over the perfect binary tree on 2^ceil(log2 n_points) caller indices; absent entries are +0.0"""
    size = 1
    while size < n_points:
        size *= 2
    s = np.zeros(size, np.float64)
    s[np.flatnonzero(present)] = values[present]
    while len(s) > 1:
        s = s[0::2] + s[1::2]
    return float(s[0])


def tree_levels(values, present, n_points, run=TREE_RUN):
    """the same tree cut the way the launches cut it: level 0 holds the sums of the aligned runs of `run` caller indices, level l
    those of the runs of `run` entries of level l - 1, each the perfect binary tree over its run with +0.0 for what is absent;
    the last level holds one sum -- tree_sum's, a taller tree adding nothing but +0.0"""
    s = np.zeros(n_points, np.float64)
    s[np.flatnonzero(present)] = values[present]
    levels = []
    while True:
        blocks = (len(s) + run - 1) // run
        t = np.zeros(blocks * run, np.float64)
        t[:len(s)] = s
        t = t.reshape(blocks, run)
        while t.shape[1] > 1:
            t = t[:, 0::2] + t[:, 1::2]
        s = t[:, 0].copy()
        levels.append(s)
        if blocks == 1:
            return levels


def threshold(S1, S2, n_tested, std_mul):
    """rule 3: (mean, raw variance, stddev, threshold): double operations, each rounded on its own"""
    nt = float(n_tested)
    mean = S1 / nt
    t = S1 * S1
    t = t / nt
    t = S2 - t
    raw = t / (nt - 1.0)
    var = raw if raw > 0.0 else 0.0
    sd = math.sqrt(var)
    return mean, raw, sd, mean + std_mul * sd


def radius_counts(pts, radius):
    """rule 4: per point the number of other points with float32 d2 < r2"""
    n = len(pts)
    c = np.zeros(n, np.int64)
    if n < 2:
        return c
    r = float(np.float32(radius)) * (1.0 + 1e-5) + 1e-30  # a superset: the float32 compare decides
    pairs = cKDTree(pts.astype(np.float64)).query_pairs(r, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    if len(pairs):
        with np.errstate(over="ignore"):
            hit = cluster_ref.d2_f32(pts[pairs[:, 0]], pts[pairs[:, 1]]) < cluster_ref.t2_of(radius)
        pairs = pairs[hit]
        c += np.bincount(pairs[:, 0], minlength=n) + np.bincount(pairs[:, 1], minlength=n)
    return c


def _check(mean_k, std_mul, radius, min_neighbors, drop, protect):
    if not 0 <= mean_k <= MAX_MEAN_K or not (math.isfinite(std_mul) and std_mul >= 0) or not (math.isfinite(radius) and radius >= 0):
        raise ValueError("parameters")
    if radius > 0 and min_neighbors < 1:
        raise ValueError("min_neighbors")
    if len(drop) > MAX_LABELS or len(protect) > MAX_LABELS:
        raise ValueError("lists")


def _finish(xyz, labels, finite, prot, tested, m, counts, mean_k, std_mul, radius, min_neighbors):
    """rules 3 (sums and threshold) to 8 from the per-point values m (over all points; used where tested) and counts"""
    n = len(xyz)
    nan = float("nan")
    info = dict(n_points=n, n_finite=int(finite.sum()), n_tested=int(tested.sum()), n_protected=int(prot.sum()), n_fail_stat=0,
                n_fail_radius=0, mean=nan, stddev=nan, threshold=nan, raw_variance=nan)
    mean_dist = np.full(n, np.nan, np.float64)
    neighbors = np.full(n, -1, np.int32)
    ok = tested.copy()
    if mean_k > 0:
        if info["n_tested"] < 2:
            raise TooFewPoints("fewer than 2 tested points")
        mean_dist[tested] = m[tested]
        S1 = tree_sum(m, tested, n)
        S2 = tree_sum(m * m, tested, n)
        info["mean"], info["raw_variance"], info["stddev"], info["threshold"] = threshold(S1, S2, info["n_tested"], float(std_mul))
        info["S1"], info["S2"] = S1, S2
        fail = tested & ~(mean_dist <= info["threshold"])
        info["n_fail_stat"] = int(fail.sum())
        ok &= ~fail
    if radius > 0:
        neighbors[tested] = np.minimum(counts[tested], min_neighbors)
        fail = tested & (counts < min_neighbors)
        info["n_fail_radius"] = int(fail.sum())
        ok &= ~fail
    keep = (ok | prot).astype(np.uint8)
    info["n_kept"] = int(keep.sum())
    out = dict(info)
    out.update(keep=keep, mean_dist=mean_dist, neighbors=neighbors, xyz_kept=xyz[keep == 1],
               labels_kept=None if labels is None else np.asarray(labels, np.uint32)[keep == 1])
    return out


def _grid_check(pts, radius):
    """rule 4: the search grid's range refusal (rule 9 of sicp_cluster)"""
    if len(pts) and (np.abs(cluster_ref.cell_coords(pts, radius)) >= cluster_ref.CELL_LIMIT).any():
        raise cluster_ref.GridOverflow("a cell coordinate reaches 2^20 - 1")


def filter(xyz, labels=None, mask=None, mean_k=20, std_mul=2.0, radius=0.0, min_neighbors=2, drop=(), protect=()):
    """the whole call: {"keep", "mean_dist", "neighbors", "xyz_kept", "labels_kept"} and the fields of sicp_filter_info (and
    raw_variance, S1, S2: what rule 3 clamps and sums)"""
    _check(mean_k, std_mul, radius, min_neighbors, drop, protect)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    finite, removed, prot, tested = classes(xyz, labels, mask, drop, protect)
    fin = np.flatnonzero(finite)
    pts = xyz[fin]
    where = np.full(n, -1, np.int64)
    where[fin] = np.arange(len(fin))
    m = np.zeros(n, np.float64)
    counts = np.zeros(n, np.int64)
    if mean_k > 0:
        if len(fin) < mean_k + 1:
            raise TooFewPoints("fewer than mean_k + 1 finite points")
        t = np.flatnonzero(tested)
        m[t] = mean_dist_of_lists(knn_d2(pts, where[t], mean_k + 1), mean_k)
    if radius > 0:
        _grid_check(pts, radius)
        counts[fin] = radius_counts(pts, radius)
    return _finish(xyz, labels, finite, prot, tested, m, counts, mean_k, std_mul, radius, min_neighbors)


def tree_sum_slow(values, present, n_points):
    """the same tree by recursion over index ranges, one Python add per node"""
    size = 1
    while size < n_points:
        size *= 2

    def node(lo, hi):
        if hi - lo == 1:
            return float(values[lo]) if lo < n_points and present[lo] else 0.0
        mid = (lo + hi) // 2
        return node(lo, mid) + node(mid, hi)

    return node(0, size)


def filter_slow(xyz, labels=None, mask=None, mean_k=20, std_mul=2.0, radius=0.0, min_neighbors=2, drop=(), protect=()):
    """the rules without a tree: every tested point against every finite point, lists by a full sort"""
    _check(mean_k, std_mul, radius, min_neighbors, drop, protect)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = len(xyz)
    finite, removed, prot, tested = classes(xyz, labels, mask, drop, protect)
    fin = np.flatnonzero(finite)
    pts = xyz[fin]
    m = np.zeros(n, np.float64)
    counts = np.zeros(n, np.int64)
    if mean_k > 0 and len(fin) < mean_k + 1:
        raise TooFewPoints("fewer than mean_k + 1 finite points")
    if radius > 0:
        _grid_check(pts, radius)
    t = np.flatnonzero(tested)
    for a in range(0, len(t), 128):
        rows = t[a:a + 128]
        d2 = _d2_rows(xyz[rows], pts)
        if mean_k > 0:
            lists = np.sort(d2, axis=1)[:, :mean_k + 1]
            m[rows] = mean_dist_of_lists(lists, mean_k)
        if radius > 0:
            counts[rows] = (d2 < cluster_ref.t2_of(radius)).sum(axis=1) - 1  # (the point itself: d2 = 0 < r2)
    return _finish(xyz, labels, finite, prot, tested, m, counts, mean_k, std_mul, radius, min_neighbors)
