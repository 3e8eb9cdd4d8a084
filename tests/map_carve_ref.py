"""numpy restatement of sicp_map_carve (include/sicp.h, "free-space carving") on top of tests/map_ref.Map, op for op: float32
where the rules say float (the transform's rounding, the key, the range test -- merge_ref's gather, voxel_coords' arithmetic
and crop_mask), python floats, which are IEEE doubles rounded operation by operation, for the walk.  Beside it segment_voxels:
the voxels a segment meets by an independent rule, in exact rational arithmetic.  numpy only: no library, no GPU."""
from __future__ import annotations

import fractions

import numpy as np

import map_ref
import merge_ref

MAX_PROTECT = 64


def defaults(**overrides):
    p = dict(max_range=0.0, min_rays=3, end_margin=1, dry_run=0, protect=())
    for k in overrides:
        if k not in p:
            raise AttributeError(k)
    p.update(overrides)
    return p


def inv_leaf(leaf):
    return np.float32(1.0) / np.float32(leaf)


def voxels_of(p, leaf):
    """(v [n, 3] int64, valid [n]): the key's float arithmetic; a coordinate beyond the key's fields makes a point invalid"""
    v = np.floor((np.asarray(p, np.float32) * inv_leaf(leaf)).astype(np.float32))
    valid = (np.abs(v) < merge_ref.LIMIT).all(axis=1)
    return np.where(valid[:, None], v, 0).astype(np.int64), valid


def walk(o, p, vo, vp, inv):
    """rule 4: the voxels v_0 .. v_n of the ray from o (voxel vo) to p (voxel vp), as tuples"""
    inv = float(inv)
    rem = [abs(int(vp[a]) - int(vo[a])) for a in range(3)]
    step = [(int(vp[a]) > int(vo[a])) - (int(vp[a]) < int(vo[a])) for a in range(3)]
    tmax, tdelta = [0.0] * 3, [0.0] * 3
    for a in range(3):
        if rem[a] > 0:
            u = float(o[a]) * inv
            w = float(p[a]) * inv
            du = w - u
            tmax[a] = (float(int(vo[a]) + (1 if step[a] > 0 else 0)) - u) / du
            tdelta[a] = float(step[a]) / du
    v = [int(vo[0]), int(vo[1]), int(vo[2])]
    out = [tuple(v)]
    for _ in range(rem[0] + rem[1] + rem[2]):
        axis = -1
        for a in range(3):
            if rem[a] > 0 and (axis < 0 or tmax[a] < tmax[axis]):
                axis = a
        v[axis] += step[axis]
        rem[axis] -= 1
        tmax[axis] = tmax[axis] + tdelta[axis]
        out.append(tuple(v))
    return out


def scan_frame(xyz, qt, sensor_origin):
    """(p [n, 3] float32: the finite points transformed; o [3] float32: (float)sensor_origin through the same arithmetic)"""
    p, _ = merge_ref.gather([(xyz, None)], None if qt is None else [qt])
    so = np.zeros((1, 3), np.float32) if sensor_origin is None else np.asarray(sensor_origin, np.float64).astype(np.float32).reshape(1, 3)
    o, _ = merge_ref.gather([(so, None)], None if qt is None else [qt])
    return p, o[0]


def rays_of(xyz, qt, sensor_origin, leaf, max_range=0.0):
    """p, o, vo, v [n, 3], valid [n], casts [n] (rules 1 - 3); an origin beyond the key's range raises GridOverflow"""
    p, o = scan_frame(xyz, qt, sensor_origin)
    vo, ok = voxels_of(o[None], leaf)
    if not ok[0]:
        raise merge_ref.GridOverflow(f"leaf size {leaf}: the sensor origin's voxel coordinate reaches 2^20")
    v, valid = voxels_of(p, leaf)
    casts = valid & merge_ref.crop_mask(p, o, max_range)
    return p, o, vo[0], v, valid, casts


def fullest_bin(hist):
    """extract's label per row: ties to the smallest label, bin 0 can win"""
    return np.argmax(hist, axis=1) if hist.shape[1] else np.zeros(len(hist), np.int64)


def carve(m: map_ref.Map, xyz, qt=None, sensor_origin=None, params=None):
    """{"miss": uint32 per row of the map before the call, "info": sicp_map_carve_info's counts}; removes the rows from `m`
    unless params["dry_run"].  A refusal raises before anything changes."""
    P = defaults() if params is None else params
    protect = [int(l) for l in P["protect"]]
    if not P["max_range"] >= 0.0 or P["min_rays"] < 1 or P["end_margin"] < 0 or P["dry_run"] not in (0, 1):
        raise ValueError("a parameter out of range")
    if len(protect) > MAX_PROTECT or (protect and m.C == 0) or any(l > m.C for l in protect):
        raise ValueError("protect")
    p, o, vo, v, valid, casts = rays_of(xyz, qt, sensor_origin, m.leaf, P["max_range"])
    n_map = len(m.key)
    row_of = {int(k): r for r, k in enumerate(m.key)}
    hit = np.zeros(n_map, bool)
    for k in map_ref.keys_of(v[valid]):
        r = row_of.get(int(k))
        if r is not None:
            hit[r] = True
    miss = np.zeros(n_map, np.uint32)
    inv = inv_leaf(m.leaf)
    n_steps = 0
    for g in np.flatnonzero(casts):
        cells = walk(o, p[g], vo, v[g], inv)
        n = len(cells) - 1
        cand = cells[:max(n - P["end_margin"], 0)]
        n_steps += len(cand)
        for c in cand:
            r = row_of.get(((c[2] + map_ref.BIAS) << 42) | ((c[1] + map_ref.BIAS) << 21) | (c[0] + map_ref.BIAS))
            if r is not None:
                miss[r] += 1
    enough = miss >= P["min_rays"]
    label_kept = np.isin(fullest_bin(m.hist), protect) if protect else np.zeros(n_map, bool)
    spared_hit = enough & hit
    spared_label = enough & ~hit & label_kept
    removed = enough & ~hit & ~label_kept
    info = dict(n_in=len(p), n_rays=int(casts.sum()), n_steps=n_steps, n_voxels=n_map, n_touched=int((miss > 0).sum()),
                n_hit=int(hit.sum()), n_removed=int(removed.sum()), n_spared_hit=int(spared_hit.sum()),
                n_spared_label=int(spared_label.sum()))
    if not P["dry_run"]:
        keep = ~removed
        m.key, m.s, m.cnt, m.hist = m.key[keep], m.s[keep], m.cnt[keep], m.hist[keep]
        info["n_voxels"] = len(m.key)
    return dict(miss=miss, info=info)


# ---- an independent rule ------------------------------------------------------------------------------------------------------
def segment_voxels(o, p, inv):
    """the voxels whose OPEN box the segment from o to p (float32, in units of 1 / inv) meets, in exact rational arithmetic:
    per voxel of the bounding box of the two ends, the open interval of t in which the segment is inside the box on every axis
    must meet [0, 1]"""
    F = fractions.Fraction
    U = [F(float(o[a])) * F(float(inv)) for a in range(3)]
    W = [F(float(p[a])) * F(float(inv)) for a in range(3)]
    lo = [min(U[a], W[a]).__floor__() for a in range(3)]
    hi = [max(U[a], W[a]).__floor__() for a in range(3)]
    spans = []
    for a in range(3):
        d = W[a] - U[a]
        per = {}
        for i in range(lo[a], hi[a] + 1):
            if d == 0:
                per[i] = (F(-1), F(2)) if i < U[a] < i + 1 else None
            else:
                t0, t1 = (i - U[a]) / d, (i + 1 - U[a]) / d
                per[i] = (min(t0, t1), max(t0, t1))
        spans.append(per)
    out = set()
    for i, sx in spans[0].items():
        if sx is None:
            continue
        for j, sy in spans[1].items():
            if sy is None:
                continue
            a0, a1 = max(sx[0], sy[0], F(0)), min(sx[1], sy[1], F(1))
            if not a0 < a1:
                continue
            for k, sz in spans[2].items():
                if sz is None:
                    continue
                if max(a0, sz[0]) < min(a1, sz[1]):
                    out.add((i, j, k))
    return out
