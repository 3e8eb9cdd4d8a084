"""numpy restatement of sicp_map_distance (include/sicp.h, "distance"): a pure function of VoxelMap.get_state()'s rows, the
params, the centre and, optionally, points with a pose.  The field is formed as the header's cost note says: obstacle cells are
seeded with the packed key (0 << 32) | row, every other cell with a "none" key, and one windowed minimum per axis adds s^2 to the
high field; integers throughout, so every byte is fixed.  numpy only: no library, no GPU.  (tests/distance_cases.py holds a
naive twin, obstacle by obstacle and cell by cell, written from the header's rules and not from this file.)"""
from __future__ import annotations

import numpy as np

import np_ref

BIAS = 1 << 20
MAX_LABELS = 64
MAX_CELLS = 1 << 24
NONE = (0x40000000 << 32) | 0xFFFFFFFF
NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
CELL_ARRAYS = (("dist_sq", np.int32), ("nearest", np.int32), ("label", np.uint32))
POINT_ARRAYS = (("point_cell", np.int32), ("point_dist_sq", np.int32), ("point_nearest", np.int32), ("point_range_sq", np.float32))
INFO = ("n_voxels", "n_points", "n_points_inside", "x0", "y0", "z0", "nx", "ny", "nz", "n_obstacles", "n_reached", "max_dist_sq",
        "voxel_size")


class Refused(ValueError):
    pass


def defaults(**kw):
    p = dict(nx=0, ny=0, nz=0, max_dist_voxels=10, min_count=1, planar=0, z_min=-np.inf, z_max=np.inf, ignore=(), only=())
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


def point_arrays(p):
    """the point arrays a call with these params can give (point_range_sq is a 3-D output)"""
    return tuple((n, dt) for n, dt in POINT_ARRAYS if not (p["planar"] and n == "point_range_sq"))


def inv_leaf(leaf):
    return np.float32(1.0) / np.float32(leaf)


def level_of(v, inv, lo, hi):
    """floorf((float)v * inv_leaf), clamped to lo .. hi"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.float32(np.float32(v) * inv))
    if not f > np.float32(lo):
        return lo
    if not f < np.float32(hi):
        return hi
    return int(f)


def refusal(leaf, num_classes, p, center, qt=None, have_handle=False, which=0, want_points=False, want_range=False):
    """the cause sicp_map_distance refuses these arguments for, or None"""
    if p is None:
        return "params"
    if center is None:
        return "center"
    if not (1 <= p["nx"] <= 1024 and 1 <= p["ny"] <= 1024 and 1 <= p["nz"] <= 256):
        return "window"
    if p["nx"] * p["ny"] * p["nz"] > MAX_CELLS:
        return "window"
    if not 1 <= p["max_dist_voxels"] <= 64:
        return "max_dist_voxels"
    if p["min_count"] < 1:
        return "min_count"
    if p["planar"] not in (0, 1) or (p["planar"] and p["nz"] != 1):
        return "planar"
    if np.isnan(p["z_min"]) or np.isnan(p["z_max"]) or not p["z_min"] <= p["z_max"]:
        return "z"
    for name in ("ignore", "only"):
        if len(p[name]) > MAX_LABELS:
            return name
        if len(p[name]) and num_classes == 0:
            return name
        if any(int(l) > num_classes for l in p[name]):
            return name
    c = np.asarray(center, dtype=np.float64).reshape(3)
    if not np.isfinite(c).all():
        return "center"
    with np.errstate(over="ignore"):
        vc = np.floor((c.astype(np.float32) * inv_leaf(leaf)).astype(np.float32))
    if not (np.abs(vc[:2 if p["planar"] else 3]) < BIAS).all():
        return "center"
    if qt is not None and not np.isfinite(np.asarray(qt, dtype=np.float64)).all():
        return "pose"
    if want_points and not have_handle:
        return "points"
    if want_range and p["planar"]:
        return "point_range_sq"
    if have_handle and which not in (0, 1):
        return "which"
    return None


def window(leaf, p, center):
    """x0, y0, z0 (rule 1; z0 = 0 in planar mode)"""
    c = np.asarray(center, dtype=np.float64).reshape(3).astype(np.float32)
    with np.errstate(over="ignore"):
        vc = np.floor((c * inv_leaf(leaf)).astype(np.float32))
    x0, y0 = int(vc[0]) - p["nx"] // 2, int(vc[1]) - p["ny"] // 2
    return x0, y0, (0 if p["planar"] else int(vc[2]) - p["nz"] // 2)


def _listed(labels, given):
    return np.isin(labels, np.asarray(list(given), dtype=np.int64))


def _sweep(key, axis, R):
    """key[c] <- min over s in -R..R of key[c + s along axis] + (s^2 << 32); cells outside the array take no part"""
    n = key.shape[axis]
    out = key.copy()
    for s in range(1, min(R, n - 1) + 1):
        add = np.int64(s * s) << np.int64(32)
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, n - s), slice(s, n)
        a, b = tuple(a), tuple(b)
        out[a] = np.minimum(out[a], key[b] + add)
        out[b] = np.minimum(out[b], key[a] + add)
    return out


def distance(state, params, center, points=None, qt=None):
    """{the CELL_ARRAYS [nz, ny, nx], with points point_arrays(params) [n], "info": the INFO fields}; Refused for what the library
    refuses"""
    leaf, C = float(state["leaf_size"]), int(state["num_classes"])
    p = params
    why = refusal(leaf, C, p, center, qt, points is not None, 0, False)
    if why:
        raise Refused(why)
    nx, ny, nz, R, planar = p["nx"], p["ny"], p["nz"], p["max_dist_voxels"], p["planar"]
    inv = inv_leaf(leaf)
    x0, y0, z0 = window(leaf, p, center)
    lo = level_of(p["z_min"], inv, -(BIAS - 1), BIAS - 1)
    hi = level_of(p["z_max"], inv, -(BIAS - 1), BIAS - 1)

    key = np.asarray(state["key"], dtype=np.uint64).astype(np.int64)
    n_map = len(key)
    cnt = np.asarray(state["count"], dtype=np.uint32).astype(np.int64)
    row_label = np.zeros(n_map, np.int64) if C == 0 else \
        np.argmax(np.asarray(state["hist"], dtype=np.uint32).reshape(-1, C + 1), axis=1).astype(np.int64)
    vx, vy, vz = (key & 0x1FFFFF) - BIAS, ((key >> 21) & 0x1FFFFF) - BIAS, ((key >> 42) & 0x1FFFFF) - BIAS
    i, j, k = vx - x0, vy - y0, (np.zeros_like(vz) if planar else vz - z0)
    counts = (cnt >= p["min_count"]) & (i >= 0) & (i < nx) & (j >= 0) & (j < ny) & (k >= 0) & (k < nz)
    if planar:
        counts &= (vz >= lo) & (vz <= hi)
    if len(p["ignore"]):
        counts &= ~_listed(row_label, p["ignore"])
    if len(p["only"]):
        counts &= _listed(row_label, p["only"])
    rows = np.flatnonzero(counts)
    field = np.full(nx * ny * nz, NONE, np.int64)
    np.minimum.at(field, ((k * ny + j) * nx + i)[rows], rows.astype(np.int64))  # (a column's smallest row in planar mode)
    n_obstacles = int((field != NONE).sum())
    field = field.reshape(nz, ny, nx)
    for axis in (2, 1, 0):  # x, y, z
        field = _sweep(field, axis, R)
    field = field.reshape(-1)
    d2, row = field >> 32, field & 0xFFFFFFFF
    reached = d2 <= R * R
    out = dict(dist_sq=np.where(reached, d2, -1).astype(np.int32), nearest=np.where(reached, row, -1).astype(np.int32))
    out["label"] = np.where(reached, row_label[np.where(reached, row, 0)] if n_map else 0, 0).astype(np.uint32)

    n_points = n_inside = 0
    if points is not None:  # rule 5
        xyz = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        n_points = len(xyz)
        pc, pd, pn = (np.full(n_points, -1, np.int32) for _ in range(3))
        pr = np.full(n_points, NAN, np.float32)
        fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
        q = np_ref.transform_points(np_ref.qt_to_mat(np.array([0, 0, 0, 1, 0, 0, 0.0]) if qt is None else qt), xyz[fin])
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.floor((q * inv).astype(np.float32))
            ok = (np.abs(v[:, :2 if planar else 3]) < BIAS).all(axis=1)
        fin, q, v = fin[ok], q[ok], v[ok]
        v = np.where(np.abs(v) < BIAS, v, 0).astype(np.int64)  # (planar: a z that is not looked at)
        pi, pj, pk = v[:, 0] - x0, v[:, 1] - y0, (np.zeros(len(v), np.int64) if planar else v[:, 2] - z0)
        inside = (pi >= 0) & (pi < nx) & (pj >= 0) & (pj < ny) & (pk >= 0) & (pk < nz)
        fin, q, c = fin[inside], q[inside], ((pk * ny + pj) * nx + pi)[inside]
        n_inside = len(fin)
        pc[fin], pd[fin], pn[fin] = c, out["dist_sq"][c], out["nearest"][c]
        if not planar:
            near = out["nearest"][c]
            has = near >= 0
            r = near[has]
            sums = np.asarray(state["sums"], dtype=np.float64).reshape(-1, 3)
            with np.errstate(over="ignore", invalid="ignore"):
                centroid = (sums[r] / cnt[r].astype(np.float64)[:, None]).astype(np.float32)
                d = (q[has] - centroid).astype(np.float32)
                sq = (d * d).astype(np.float32)
                pr[fin[has]] = ((sq[:, 0] + sq[:, 1]).astype(np.float32) + sq[:, 2]).astype(np.float32)
        out["point_cell"], out["point_dist_sq"], out["point_nearest"] = pc, pd, pn
        if not planar:
            out["point_range_sq"] = pr

    for name, _ in CELL_ARRAYS:
        out[name] = out[name].reshape(nz, ny, nx)
    out["info"] = dict(n_voxels=n_map, n_points=n_points, n_points_inside=n_inside, x0=x0, y0=y0, z0=z0, nx=nx, ny=ny, nz=nz,
                       n_obstacles=n_obstacles, n_reached=int(reached.sum()), max_dist_sq=int(d2[reached].max()) if reached.any() else -1,
                       voxel_size=leaf)
    return out
