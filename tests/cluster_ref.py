"""numpy / scipy restatement of sicp_cluster (include/sicp.h, "objects of a labelled cloud", rules 1 - 4): candidate pairs from
a k-d tree at a slightly larger radius, re-decided by the float32 arithmetic of rule 2; components by
scipy.sparse.csgraph.connected_components; numbering by smallest caller index; centroids as sequential float64 sums.  Imports
nothing of the product.  cluster_slow() states the same rules once more as an O(n^2) loop over all pairs with a union-find of
its own, for the CPU tests to hold the fast form against."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


CELL_LIMIT = 2 ** 20 - 1  # include/sicp.h, rule 9: a cell coordinate of this magnitude or more is refused
PAIR_CHUNK = 256          # points of a cell one workgroup of the pair pass (and of the filter's radius count) takes per step
PAIR_CHUNK_GROUPS = 8     # workgroups a cell's chunks go round: a cell of more than PAIR_CHUNK PAIR_CHUNK_GROUPS points gives one a second
                          # step (the shapes the GPU tests straddle; no rule depends on either)


class GridOverflow(ValueError):
    pass


def grid_inv(tolerance):
    """cells per metre of the search grid: the largest float32 inv with inv * (float)tolerance <= 1 (exact product)"""
    t = np.float32(tolerance)
    inv = np.float32(1.0 / float(t))
    while float(inv) * float(t) > 1.0:
        inv = np.nextafter(inv, np.float32(0))
    return inv


def cell_coords(xyz, tolerance):
    """floor of the exact product (double)p * (double)inv per axis, as int64"""
    return np.floor(np.asarray(xyz, np.float32).astype(np.float64) * float(grid_inv(tolerance))).astype(np.int64)


def t2_of(tolerance):
    """(float)tolerance * (float)tolerance in float32"""
    t = np.float32(tolerance)
    return np.float32(t * t)


def d2_f32(p, q):
    """rule 2: d = p - q in float32, d2 = (dx dx + dy dy) + dz dz, every operation rounded to float32"""
    d = (np.asarray(p, np.float32) - np.asarray(q, np.float32)).astype(np.float32)
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32) + (dz * dz).astype(np.float32)


def vertices(xyz, labels, ignore):
    """caller indices of the vertices (rule 1), ascending"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    ok = np.isfinite(xyz).all(axis=1)
    if labels is not None and len(ignore):
        ok &= ~np.isin(np.asarray(labels, np.uint32), np.asarray(list(ignore), np.uint32))
    return np.flatnonzero(ok)


def edges(xyz, labels, v, tolerance, same_label):
    """rule 2 over the vertices v: pairs (a, b) of positions in v, a < b"""
    p = xyz[v].astype(np.float64)
    if len(v) < 2:
        return np.zeros((0, 2), dtype=np.int64)
    r = float(np.float32(tolerance)) * (1.0 + 1e-5) + 1e-30  # a superset: rule 2 decides
    pairs = cKDTree(p).query_pairs(r, output_type="ndarray").astype(np.int64).reshape(-1, 2)
    if len(pairs) == 0:
        return pairs
    with np.errstate(over="ignore"):
        keep = d2_f32(xyz[v[pairs[:, 0]]], xyz[v[pairs[:, 1]]]) < t2_of(tolerance)
    if same_label and labels is not None:
        keep &= labels[v[pairs[:, 0]]] == labels[v[pairs[:, 1]]]
    return pairs[keep]


def table(xyz, labels, v, comp, n_points, min_points, max_points):
    """rules 3 and 4 from the component number of every vertex"""
    n_comp = int(comp.max()) + 1 if len(comp) else 0
    size = np.bincount(comp, minlength=n_comp)
    first = np.full(n_comp, n_points, dtype=np.int64)
    np.minimum.at(first, comp, v)
    hi = max_points if max_points > 0 else np.iinfo(np.int64).max
    is_cluster = (size >= min_points) & (size <= hi)
    order = np.argsort(first, kind="stable")
    order = order[is_cluster[order]]
    number = np.full(n_comp, -1, dtype=np.int32)
    number[order] = np.arange(len(order), dtype=np.int32)
    cid = np.full(n_points, -1, dtype=np.int32)
    cid[v] = number[comp]
    k = len(order)
    out = {
        "cluster_id": cid,
        "label": np.zeros(k, dtype=np.uint32),
        "count": size[order].astype(np.int32),
        "first_index": first[order].astype(np.int32),
        "centroid": np.zeros((k, 3), dtype=np.float64),
        "bbox_min": np.zeros((k, 3), dtype=np.float32),
        "bbox_max": np.zeros((k, 3), dtype=np.float32),
        "n_points": n_points,
        "n_kept": len(v),
        "n_components": n_comp,
        "n_clusters": k,
        "max_cluster_points": int(size[order].max()) if k else 0,
        "n_clustered": int(size[order].sum()) if k else 0,
    }
    members = np.argsort(cid, kind="stable")  # ascending caller index inside a cluster
    members = members[cid[members] >= 0]
    ends = np.cumsum(out["count"])
    for c in range(k):
        m = members[ends[c] - out["count"][c]:ends[c]]
        pts = xyz[m]
        out["centroid"][c] = np.cumsum(pts.astype(np.float64), axis=0)[-1] / float(len(m))
        out["bbox_min"][c] = pts.min(axis=0)
        out["bbox_max"][c] = pts.max(axis=0)
        if labels is not None:
            val, cnt = np.unique(labels[m], return_counts=True)  # ascending values: argmax takes the smallest of a tie
            out["label"][c] = val[np.argmax(cnt)]
    return out


def components(xyz, labels, tolerance=0.5, same_label=1, ignore=()):
    """rules 1 and 2: (caller indices of the vertices, component number of each)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    labels = None if labels is None else np.ascontiguousarray(labels, np.uint32)
    if labels is None and (same_label or len(ignore)):
        raise ValueError("a cloud without labels needs same_label = 0 and nothing ignored")
    v = vertices(xyz, labels, ignore)
    if len(v) and np.abs(cell_coords(xyz[v], tolerance)).max() >= CELL_LIMIT:
        raise GridOverflow(f"tolerance {tolerance}: a cell coordinate reaches 2^20 - 1")
    e = edges(xyz, labels, v, tolerance, same_label)
    n = len(v)
    if n:
        g = coo_matrix((np.ones(len(e), dtype=np.int8), (e[:, 0], e[:, 1])), shape=(n, n))
        _, comp = connected_components(g, directed=False)
    else:
        comp = np.zeros(0, dtype=np.int64)
    return v, comp.astype(np.int64)


def cluster(xyz, labels, tolerance=0.5, min_points=10, max_points=0, same_label=1, ignore=(), parts=None):
    """parts: what components() gave for the same cloud, tolerance, same_label and ignore (the size bounds play no part in it)"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    labels = None if labels is None else np.ascontiguousarray(labels, np.uint32)
    v, comp = parts if parts is not None else components(xyz, labels, tolerance, same_label, ignore)
    return table(xyz, labels, v, comp, len(xyz), min_points, max_points)


def cluster_slow(xyz, labels, tolerance=0.5, min_points=10, max_points=0, same_label=1, ignore=()):
    """the same rules, every pair of vertices visited"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    labels = None if labels is None else np.ascontiguousarray(labels, np.uint32)
    v = vertices(xyz, labels, ignore)
    n = len(v)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a

    t2 = t2_of(tolerance)
    for a in range(n):
        with np.errstate(over="ignore"):
            hit = d2_f32(xyz[v[a]][None, :], xyz[v[a + 1:]]) < t2
        if same_label and labels is not None:
            hit &= labels[v[a + 1:]] == labels[v[a]]
        for b in np.flatnonzero(hit) + a + 1:
            ra, rb = find(a), find(int(b))
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(a) for a in range(n)], dtype=np.int64)
    _, comp = np.unique(roots, return_inverse=True)
    return table(xyz, labels, v, comp.astype(np.int64), len(xyz), min_points, max_points)


def partition(cid):
    """the partition a cluster_id array describes, free of numbering: a sorted list of sorted member tuples"""
    cid = np.asarray(cid)
    return sorted(tuple(np.flatnonzero(cid == c).tolist()) for c in np.unique(cid[cid >= 0]))
