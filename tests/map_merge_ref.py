"""numpy restatement of sicp_map_merge and of the map's state calls (include/sicp.h, "fusing maps" and "the map's exact
contents") on top of tests/map_ref.py's Map.  merge(dst, src, qt, ...) follows rules 1 - 6: src's rows in ascending key, the
sums moved by the pose with one np.float64 operation at a time, the float32 centroid of the MOVED sums cropped and keyed on dst's
grid, a stable argsort, and per touched voxel a sequential fold from the stored value in ascending src row -- the left fold of
Map.integrate with rows for points.  state() / from_state() are the arrays of sicp_map_get_state / the checks of
sicp_map_set_state.  Beside them merge_slow: the same rules row by row with python floats and a dict keyed by the voxel key, as
map_ref.MapSlow is for integrate.  numpy only: no library, no GPU."""
from __future__ import annotations

import numpy as np

import map_ref
import merge_ref
import np_ref

MAX_VOXELS = (1 << 31) - 1
MAX_POINTS = (1 << 32) - 1
INFO_KEYS = ("n_src_rows", "n_kept_rows", "n_kept_points", "n_touched", "n_new_voxels", "max_run", "n_voxels")


class Refused(ValueError):
    """a call the library answers with SICP_ERR_INVALID_ARGUMENT; nothing has changed"""


class BadState(Refused):
    def __init__(self, row, why):
        super().__init__(f"row {row}: {why}")
        self.row = row


def moved_sums(s, cnt, qt):
    """rule 2: per axis ((M0 sx + M1 sy) + M2 sz) + M3 (double)c, every operation rounded on its own"""
    M = np_ref.qt_to_mat(merge_ref.IDENT if qt is None else np.asarray(qt, dtype=np.float64))
    s = np.asarray(s, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(cnt).astype(np.float64)
    t = np.empty_like(s)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            t[:, a] = ((M[a, 0] * s[:, 0] + M[a, 1] * s[:, 1]) + M[a, 2] * s[:, 2]) + M[a, 3] * c
    return t


def _check_args(dst, src, qt, min_count, center, crop_range):
    if dst is src:
        raise Refused("src and dst are the same map")
    if min_count < 1:
        raise Refused("min_count must be >= 1")
    if not crop_range >= 0.0:
        raise Refused("crop_range must be >= 0")
    if not np.isfinite(np.asarray(center, dtype=np.float64)).all():
        raise Refused("crop_center must be finite")
    if qt is not None and not np.isfinite(np.asarray(qt, dtype=np.float64)).all():
        raise Refused("the pose is not finite")
    if dst.C > 0 and src.C != dst.C:
        raise Refused(f"src keeps {src.C} classes, dst {dst.C}")


def merge(dst, src, qt=None, min_count=1, center=(0.0, 0.0, 0.0), crop_range=0.0, descending=False):
    """adds src's rows into dst (both map_ref.Map); returns the fields of sicp_map_merge_info; a refusal raises before anything
    changes.  descending=True folds every run in DESCENDING src row: not the rule, the contrast the tests tell it from."""
    _check_args(dst, src, qt, min_count, center, crop_range)
    info = dict(n_src_rows=len(src.key), n_kept_rows=0, n_kept_points=0, n_touched=0, n_new_voxels=0, max_run=0, n_voxels=len(dst.key))
    rows = np.flatnonzero(src.cnt >= min_count)  # rule 1 (the rows ascend in key)
    cnt = src.cnt[rows]
    t = moved_sums(src.s[rows], cnt, qt)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (t / cnt.astype(np.float64)[:, None]).astype(np.float32)  # rule 3
        keep = merge_ref.crop_mask(p, center, crop_range)
    rows, cnt, t, p = rows[keep], cnt[keep], t[keep], p[keep]
    try:
        v = merge_ref.voxel_coords(p, dst.leaf)
    except merge_ref.GridOverflow as e:
        raise Refused(str(e)) from e
    if not len(rows):
        return info
    k = map_ref.keys_of(v)
    order = np.argsort(k, kind="stable")  # by key, then src row
    ks, ts, cs, rs = k[order], t[order], cnt[order], rows[order]
    uniq, starts, counts = np.unique(ks, return_index=True, return_counts=True)
    keys = np.union1d(dst.key, uniq)
    points = int(cnt.sum())
    if len(keys) > MAX_VOXELS:
        raise Refused("dst would hold more than 2^31 - 1 voxels")
    if int(dst.cnt.sum()) + points > MAX_POINTS:
        raise Refused("dst would hold more than 2^32 - 1 points")
    old = np.searchsorted(keys, dst.key)
    s, c, hist = np.zeros((len(keys), 3)), np.zeros(len(keys), np.int64), np.zeros((len(keys), dst.C + 1), np.uint32)
    s[old], c[old], hist[old] = dst.s, dst.cnt, dst.hist
    into = np.searchsorted(keys, uniq)
    acc = s[into]
    for j in range(int(counts.max())):  # rule 4: sequential per voxel, from the stored value, one add per axis and row
        live = counts > j
        at = starts[live] + (counts[live] - 1 - j if descending else j)
        acc[live] += ts[at]
    s[into] = acc
    per_row = np.repeat(into, counts)
    np.add.at(c, per_row, cs)
    if dst.C > 0:
        np.add.at(hist, per_row, src.hist[rs])
    info.update(n_kept_rows=len(rows), n_kept_points=points, n_touched=len(uniq), n_new_voxels=len(keys) - len(dst.key),
                max_run=int(counts.max()), n_voxels=len(keys))
    dst.key, dst.s, dst.cnt, dst.hist = keys, s, c, hist
    return info


# ---- the state ------------------------------------------------------------------------------------------------------------------
def state(m):
    """sicp_map_get_state's arrays of a map_ref.Map, with the creation parameters beside them"""
    return dict(key=m.key.astype(np.uint64), sums=m.s.astype(np.float64).reshape(-1, 3).copy(), count=m.cnt.astype(np.uint32),
                hist=m.hist.astype(np.uint32).copy() if m.C > 0 else None, leaf_size=m.leaf, num_classes=m.C)


def check_state(st):
    """sicp_map_set_state's checks, row by row in its order; raises BadState with the row"""
    key = np.asarray(st["key"], dtype=np.uint64).reshape(-1)
    sums = np.asarray(st["sums"], dtype=np.float64).reshape(-1, 3)
    count = np.asarray(st["count"], dtype=np.uint32).reshape(-1)
    C = int(st["num_classes"])
    if len(key) > MAX_VOXELS:
        raise Refused("more than 2^31 - 1 rows")
    points = 0
    for r in range(len(key)):
        k = int(key[r])
        if r > 0 and not int(key[r - 1]) < k:
            raise BadState(r, "the keys do not ascend strictly")
        if k >> 63 or not (k & 0x1fffff) or not ((k >> 21) & 0x1fffff) or not ((k >> 42) & 0x1fffff):
            raise BadState(r, "no point has this key")
        if count[r] == 0:
            raise BadState(r, "the count is 0")
        if not np.isfinite(sums[r]).all():
            raise BadState(r, "a sum is not finite")
        if C > 0 and int(np.asarray(st["hist"][r], dtype=np.uint64).sum()) != int(count[r]):
            raise BadState(r, "the histogram does not add up to the count")
        points += int(count[r])
        if points > MAX_POINTS:
            raise BadState(r, "more than 2^32 - 1 points")


def from_state(st):
    check_state(st)
    m = map_ref.Map(float(st["leaf_size"]), int(st["num_classes"]))
    n = len(st["key"])
    m.key = np.asarray(st["key"], dtype=np.uint64).astype(np.int64).reshape(-1)
    m.s = np.asarray(st["sums"], dtype=np.float64).reshape(-1, 3).copy()
    m.cnt = np.asarray(st["count"], dtype=np.uint32).astype(np.int64).reshape(-1)
    m.hist = np.asarray(st["hist"], dtype=np.uint32).reshape(n, m.C + 1).copy() if m.C > 0 else np.zeros((n, 1), np.uint32)
    return m


def copy_of(m):
    c = map_ref.Map(m.leaf, m.C)
    c.key, c.s, c.cnt, c.hist = m.key.copy(), m.s.copy(), m.cnt.copy(), m.hist.copy()
    return c


def state_bytes(st):
    return tuple(None if st[k] is None else np.ascontiguousarray(st[k]).tobytes() for k in ("key", "sums", "count", "hist"))


def centroid_keys(m):
    """the key of every row's own float centroid (float)(s / count) on the map's grid: rule 3's invariant says it is the row's"""
    return map_ref.keys_of(merge_ref.voxel_coords(m.centroids(), m.leaf))


# ---- the slow restatement ---------------------------------------------------------------------------------------------------------
def merge_slow(dst, src, qt=None, min_count=1, center=(0.0, 0.0, 0.0), crop_range=0.0):
    """the same rules row by row on copies: python floats for every sum and product, np.float32 scalars for the centroid, the crop
    and the voxel, a dict keyed by the voxel key.  Returns the merged map's state (dst itself is not touched)."""
    f32 = np.float32
    M = [[float(x) for x in row] for row in np_ref.qt_to_mat(merge_ref.IDENT if qt is None else np.asarray(qt, dtype=np.float64))[:3]]
    cells = {int(k): [float(dst.s[i, 0]), float(dst.s[i, 1]), float(dst.s[i, 2]), int(dst.cnt[i]), [int(h) for h in dst.hist[i]]]
             for i, k in enumerate(dst.key)}
    c32 = [f32(x) for x in np.asarray(center, dtype=np.float64)]
    inv = f32(1.0) / f32(dst.leaf)
    bias = map_ref.BIAS
    for r in range(len(src.key)):  # ascending key
        c = int(src.cnt[r])
        if c < min_count:
            continue
        sx, sy, sz = (float(x) for x in src.s[r])
        t = [((M[a][0] * sx + M[a][1] * sy) + M[a][2] * sz) + M[a][3] * float(c) for a in range(3)]
        p = [f32(t[a] / float(c)) for a in range(3)]
        if crop_range > 0:
            d = [f32(p[a] - c32[a]) for a in range(3)]
            d2 = f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))
            if not float(d2) <= float(crop_range) * float(crop_range):
                continue
        v = [int(np.floor(f32(p[a] * inv))) for a in range(3)]
        assert all(abs(x) < bias for x in v)
        key = ((v[2] + bias) << 42) | ((v[1] + bias) << 21) | (v[0] + bias)
        cell = cells.setdefault(key, [0.0, 0.0, 0.0, 0, [0] * (dst.C + 1)])
        cell[0] += t[0]; cell[1] += t[1]; cell[2] += t[2]
        cell[3] += c
        if dst.C > 0:
            for b in range(dst.C + 1):
                cell[4][b] += int(src.hist[r, b])
    keys = sorted(cells)
    return dict(key=np.array(keys, dtype=np.uint64), sums=np.array([cells[k][:3] for k in keys], dtype=np.float64).reshape(-1, 3),
                count=np.array([cells[k][3] for k in keys], dtype=np.uint32),
                hist=np.array([cells[k][4] for k in keys], dtype=np.uint32).reshape(-1, dst.C + 1) if dst.C > 0 else None,
                leaf_size=dst.leaf, num_classes=dst.C)
