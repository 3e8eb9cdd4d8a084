"""numpy restatement of sicp_map_raycast (include/sicp.h, "ray casting") on top of tests/map_ref.Map and tests/map_carve_ref.py:
the rays are carve's (rays_of: the transform's rounding, the key, the range test) and so is the walk (walk: python floats,
IEEE doubles rounded operation by operation); what is new is the opaque rule, the stop at the first opaque voxel and the
per-ray outputs.  numpy only: no library, no GPU."""
from __future__ import annotations

import numpy as np

import map_carve_ref
import map_ref

MAX_IGNORE = 64
COUNTS = ("n_in", "n_rays", "n_steps", "n_hits", "n_voxels", "n_visible")
ARRAYS = ("row", "step", "length", "xyz", "labels", "count", "range_sq")


def defaults(**overrides):
    p = dict(max_range=0.0, min_count=1, start_margin=1, ignore=())
    for k in overrides:
        if k not in p:
            raise AttributeError(k)
    p.update(overrides)
    return p


def opaque_rows(m: map_ref.Map, P):
    """rule 4: count >= min_count and, with labels ignored, the fullest bin not among them"""
    ignore = [int(l) for l in P["ignore"]]
    opaque = m.cnt >= P["min_count"]
    if ignore:
        opaque = opaque & ~np.isin(map_carve_ref.fullest_bin(m.hist), ignore)
    return opaque


def key_of(c):
    return ((c[2] + map_ref.BIAS) << 42) | ((c[1] + map_ref.BIAS) << 21) | (c[0] + map_ref.BIAS)


def raycast(m: map_ref.Map, ends, qt=None, sensor_origin=None, params=None):
    """{"row", "step", "length" int32 [n], "xyz" float32 [n, 3], "labels", "count" uint32 [n], "range_sq" float64 [n], "info":
    sicp_map_raycast_info's counts}, ray i belonging to ends[i].  A refusal raises."""
    P = defaults() if params is None else params
    ignore = [int(l) for l in P["ignore"]]
    if not P["max_range"] >= 0.0 or P["min_count"] < 1 or P["start_margin"] < 0:
        raise ValueError("a parameter out of range")
    if len(ignore) > MAX_IGNORE or (ignore and m.C == 0) or any(l > m.C for l in ignore):
        raise ValueError("ignore")
    ends = np.asarray(ends, np.float32).reshape(-1, 3)
    n_in = len(ends)
    # (rays_of works on the finite ends -- merge_ref.gather drops the others: `at` maps them back to their index)
    at = np.flatnonzero(np.isfinite(ends).all(axis=1))
    p, o, vo, v, valid, casts = map_carve_ref.rays_of(ends, qt, sensor_origin, m.leaf, P["max_range"])
    assert len(p) == len(at)
    n_map = len(m.key)
    row_of = {int(k): r for r, k in enumerate(m.key)}
    opaque = opaque_rows(m, P)
    centroid = m.centroids()
    fullest = map_carve_ref.fullest_bin(m.hist) if m.C > 0 else np.zeros(n_map, np.int64)
    inv = map_carve_ref.inv_leaf(m.leaf)
    sm = P["start_margin"]
    row = np.full(n_in, -1, np.int32)
    step = np.full(n_in, -1, np.int32)
    length = np.full(n_in, -1, np.int32)
    xyz = np.zeros((n_in, 3), np.float32)
    labels = np.zeros(n_in, np.uint32)
    count = np.zeros(n_in, np.uint32)
    range_sq = np.full(n_in, -1.0, np.float64)
    n_steps = 0
    for g in np.flatnonzero(casts):
        i = int(at[g])
        cells = map_carve_ref.walk(o, p[g], vo, v[g], inv)
        n = len(cells) - 1
        length[i] = n
        hit = -1
        for s in range(sm, n + 1):
            r = row_of.get(key_of(cells[s]))
            if r is not None and opaque[r]:
                hit = s
                break
        if hit < 0:
            n_steps += max(n + 1 - sm, 0)
            continue
        n_steps += hit - sm + 1
        row[i], step[i] = r, hit
        xyz[i] = centroid[r]
        labels[i] = fullest[r]
        count[i] = m.cnt[r]
        dx, dy, dz = (float(centroid[r, a]) - float(o[a]) for a in range(3))
        range_sq[i] = (dx * dx + dy * dy) + dz * dz
    info = dict(n_in=n_in, n_rays=int(casts.sum()), n_steps=n_steps, n_hits=int((row >= 0).sum()), n_voxels=n_map,
                n_visible=len(np.unique(row[row >= 0])))
    return dict(row=row, step=step, length=length, xyz=xyz, labels=labels, count=count, range_sq=range_sq, info=info)


def visible_cloud(m: map_ref.Map, out):
    """rule 9: (xyz, labels or None) of the distinct rows hit, ascending key -- what dst's slot is set to"""
    u = np.unique(out["row"][out["row"] >= 0])
    ex = m.extract()
    return ex["xyz"][u], None if ex["labels"] is None else ex["labels"][u]
