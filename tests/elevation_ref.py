"""numpy restatement of sicp_map_elevation (include/sicp.h, "elevation"): a pure function of VoxelMap.get_state()'s rows, the
params, the centre and, optionally, points with a pose.  Vectorised; every float32 step is np.float32 arithmetic, every float64
sum a left fold in ascending map row.  numpy only: no library, no GPU.  (tests/elevation_cases.py holds a naive twin, cell by
cell in plain Python, written from the header's rules and not from this file.)"""
from __future__ import annotations

import numpy as np

import np_ref

BIAS = 1 << 20
MAX_LABELS = 64
NAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]
UNKNOWN, FREE, BLOCKED_LABEL, OBSTACLE, LOW_CLEARANCE, STEP, SPARSE = range(7)
CELL_ARRAYS = (("state", np.uint8), ("elevation", np.float32), ("bottom", np.float32), ("ceiling", np.float32), ("label", np.uint32),
               ("count", np.uint32), ("level_top", np.int32), ("level_bottom", np.int32), ("n_levels", np.int32), ("step", np.float32),
               ("neighbors", np.uint8), ("cell_class", np.uint8))
POINT_ARRAYS = (("point_cell", np.int32), ("point_height", np.float32))
WINDOW_FREE = ("state", "elevation", "bottom", "ceiling", "label", "count", "level_top", "level_bottom", "n_levels")  # rule 9
INFO = ("n_voxels", "n_points", "x0", "y0", "width", "height", "n_class", "cell_size")


class Refused(ValueError):
    pass


def defaults(**kw):
    p = dict(width=0, height=0, cell_voxels=1, min_count=1, ignore=(), z_min=-np.inf, z_max=np.inf, clearance_voxels=10, use_ref_z=0,
             ref_z=0.0, blocked=(), drivable=(), max_extent_voxels=2, min_clearance=0.0, max_step=np.inf, min_neighbors=0)
    for k, v in kw.items():
        if k not in p:
            raise KeyError(k)
        p[k] = v
    return p


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


def refusal(leaf, num_classes, p, center, qt=None, have_handle=False, which=0, want_points=False):
    """the cause sicp_map_elevation refuses these arguments for, or None"""
    if p is None:
        return "params"
    if center is None:
        return "center"
    if not (1 <= p["width"] <= 2048 and 1 <= p["height"] <= 2048):
        return "window"
    if not 1 <= p["cell_voxels"] <= 8:
        return "cell_voxels"
    if p["min_count"] < 1:
        return "min_count"
    if np.isnan(p["z_min"]) or np.isnan(p["z_max"]) or not p["z_min"] <= p["z_max"]:
        return "z"
    if p["clearance_voxels"] < 1:
        return "clearance_voxels"
    if p["use_ref_z"] not in (0, 1):
        return "use_ref_z"
    if p["use_ref_z"] and not np.isfinite(p["ref_z"]):
        return "ref_z"
    if p["max_extent_voxels"] < 0:
        return "max_extent_voxels"
    if not p["min_clearance"] >= 0:
        return "min_clearance"
    if not p["max_step"] >= 0:
        return "max_step"
    if not 0 <= p["min_neighbors"] <= 8:
        return "min_neighbors"
    for name in ("ignore", "blocked", "drivable"):
        if len(p[name]) > MAX_LABELS:
            return name
        if len(p[name]) and num_classes == 0:
            return name
        if any(int(l) > num_classes for l in p[name]):
            return name
    c = np.asarray(center, dtype=np.float64).reshape(2)
    if not np.isfinite(c).all():
        return "center"
    with np.errstate(over="ignore"):
        vc = np.floor((c.astype(np.float32) * inv_leaf(leaf)).astype(np.float32))
    if not (np.abs(vc) < BIAS).all():
        return "center"
    if qt is not None and not np.isfinite(np.asarray(qt, dtype=np.float64)).all():
        return "pose"
    if want_points and not have_handle:
        return "points"
    if have_handle and which not in (0, 1):
        return "which"
    return None


def window(leaf, p, center):
    """x0, y0 (rule 1)"""
    c = np.asarray(center, dtype=np.float64).reshape(2).astype(np.float32)
    vc = np.floor((c * inv_leaf(leaf)).astype(np.float32)).astype(np.int64)
    B = p["cell_voxels"]
    return int(vc[0] // B - p["width"] // 2), int(vc[1] // B - p["height"] // 2)


def _fold(values, starts, sizes):
    """per group the left fold 0.0 + v[s] + v[s + 1] + ... in float64"""
    acc = np.zeros(len(starts), np.float64)
    for j in range(int(sizes.max()) if len(sizes) else 0):
        live = sizes > j
        acc[live] = acc[live] + values[starts[live] + j]
    return acc


def _listed(labels, given):
    return np.isin(labels, np.asarray(list(given), dtype=np.int64)) if len(given) else np.zeros(len(labels), bool)


def elevation(state, params, center, points=None, qt=None):
    """{the CELL_ARRAYS [height, width], with points the POINT_ARRAYS [n], "info": the INFO fields}; Refused for what the library
    refuses"""
    leaf, C = float(state["leaf_size"]), int(state["num_classes"])
    p = params
    why = refusal(leaf, C, p, center, qt, points is not None, 0, False)
    if why:
        raise Refused(why)
    W, H, B = p["width"], p["height"], p["cell_voxels"]
    inv = inv_leaf(leaf)
    x0, y0 = window(leaf, p, center)
    lo = level_of(p["z_min"], inv, -(BIAS - 1), BIAS - 1)
    hi = level_of(p["z_max"], inv, -(BIAS - 1), BIAS - 1)
    vref = level_of(p["ref_z"], inv, -BIAS, BIAS) if p["use_ref_z"] else 0

    key = np.asarray(state["key"], dtype=np.uint64).astype(np.int64)
    sz = np.asarray(state["sums"], dtype=np.float64).reshape(-1, 3)[:, 2]
    cnt = np.asarray(state["count"], dtype=np.uint32).astype(np.int64)
    hist = None if C == 0 else np.asarray(state["hist"], dtype=np.uint32).reshape(-1, C + 1).astype(np.int64)
    vx, vy, vz = (key & 0x1FFFFF) - BIAS, ((key >> 21) & 0x1FFFFF) - BIAS, ((key >> 42) & 0x1FFFFF) - BIAS
    ci, cj = vx // B - x0, vy // B - y0
    counts = (cnt >= p["min_count"]) & (vz >= lo) & (vz <= hi) & (ci >= 0) & (ci < W) & (cj >= 0) & (cj < H)
    if len(p["ignore"]):
        counts &= ~_listed(np.argmax(hist, axis=1), p["ignore"])

    out = {name: np.zeros(W * H, dt) for name, dt in CELL_ARRAYS}
    for name in ("elevation", "bottom", "ceiling", "step"):
        out[name][:] = NAN
    rows = np.flatnonzero(counts)
    if len(rows):
        cell, lev = (cj * W + ci)[rows], vz[rows]
        order = np.lexsort((lev, cell))  # stable: equal (cell, level) stay in ascending map row
        rows, cell, lev = rows[order], cell[order], lev[order]
        head = np.ones(len(rows), bool)
        head[1:] = (cell[1:] != cell[:-1]) | (lev[1:] != lev[:-1])
        g_at = np.flatnonzero(head)  # the level groups
        g_size = np.diff(np.append(g_at, len(rows)))
        g_cell, g_lev = cell[g_at], lev[g_at]
        g_n = np.add.reduceat(cnt[rows], g_at)
        with np.errstate(over="ignore"):
            g_mean = (_fold(sz[rows], g_at, g_size) / g_n.astype(np.float64)).astype(np.float32)
        if C > 0:
            g_label = np.argmax(np.add.reduceat(hist[rows], g_at, axis=0), axis=1)
        else:
            g_label = np.zeros(len(g_at), np.int64)
        # runs (rule 3)
        new_run = np.ones(len(g_at), bool)
        new_run[1:] = (g_cell[1:] != g_cell[:-1]) | (g_lev[1:] - g_lev[:-1] > p["clearance_voxels"])
        r_first = np.flatnonzero(new_run)  # a run's bottom group
        r_last = np.append(r_first[1:], len(g_at)) - 1  # its top group
        r_cell, r_bottom = g_cell[r_first], g_lev[r_first]
        # the chosen run of every occupied cell (rule 4)
        c_head = np.ones(len(r_first), bool)
        c_head[1:] = r_cell[1:] != r_cell[:-1]
        c_first = np.flatnonzero(c_head)
        c_runs = np.diff(np.append(c_first, len(r_first)))
        chosen = c_first.copy()
        if p["use_ref_z"]:
            below = np.add.reduceat((r_bottom <= vref).astype(np.int64), c_first)  # (bottoms ascend: they are the cell's first runs)
            chosen = c_first + np.maximum(below - 1, 0)
        has_next = chosen + 1 < c_first + c_runs
        nxt = np.where(has_next, chosen + 1, chosen)
        c = r_cell[chosen]
        t, b = r_last[chosen], r_first[chosen]
        out["state"][c] = 1
        out["elevation"][c] = g_mean[t]
        out["bottom"][c] = g_mean[b]
        out["ceiling"][c] = np.where(has_next, g_mean[r_first[nxt]], np.float32(np.inf))
        out["count"][c] = g_n[t]
        out["label"][c] = g_label[t]
        out["level_top"][c] = g_lev[t]
        out["level_bottom"][c] = g_lev[b]
        out["n_levels"][c] = t - b + 1

    # rule 6
    surface = out["state"].reshape(H, W) == 1
    e = out["elevation"].reshape(H, W)
    step = np.where(surface, np.float32(0), NAN).astype(np.float32)
    nb = np.zeros((H, W), np.int64)
    ps = np.zeros((H + 2, W + 2), bool)
    ps[1:-1, 1:-1] = surface
    pe = np.zeros((H + 2, W + 2), np.float32)
    pe[1:-1, 1:-1] = e
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if di == 0 and dj == 0:
                continue
            ns, ne = ps[1 + dj:1 + dj + H, 1 + di:1 + di + W], pe[1 + dj:1 + dj + H, 1 + di:1 + di + W]
            both = surface & ns
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.abs((ne - e).astype(np.float32))
                step = np.where(both & (d > step), d, step).astype(np.float32)
            nb += both
    out["step"] = step.reshape(-1)
    out["neighbors"] = nb.reshape(-1).astype(np.uint8)
    # rule 7
    surface = surface.reshape(-1)
    lab = out["label"].astype(np.int64)
    blocked = _listed(lab, p["blocked"])
    if len(p["drivable"]):
        blocked = blocked | ~_listed(lab, p["drivable"])
    with np.errstate(invalid="ignore", over="ignore"):
        gap = (out["ceiling"] - out["elevation"]).astype(np.float32).astype(np.float64)
        low = (p["min_clearance"] > 0) & np.isfinite(out["ceiling"]) & (gap < p["min_clearance"])
        stepped = out["step"].astype(np.float64) > p["max_step"]
    cls = np.select([~surface, blocked, out["level_top"] - out["level_bottom"] > p["max_extent_voxels"], low, stepped,
                     out["neighbors"] < p["min_neighbors"]], [UNKNOWN, BLOCKED_LABEL, OBSTACLE, LOW_CLEARANCE, STEP, SPARSE], FREE)
    out["cell_class"] = cls.astype(np.uint8)
    n_class = np.bincount(cls, minlength=8).astype(int).tolist()

    n_points = 0
    if points is not None:  # rule 8
        xyz = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        n_points = len(xyz)
        pc = np.full(n_points, -1, np.int32)
        ph = np.full(n_points, NAN, np.float32)
        fin = np.flatnonzero(np.isfinite(xyz).all(axis=1))
        q = np_ref.transform_points(np_ref.qt_to_mat(np_ref_ident() if qt is None else qt), xyz[fin])
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.floor((q * inv).astype(np.float32))
            ok = (np.abs(v) < BIAS).all(axis=1)
        fin, q, v = fin[ok], q[ok], v[ok].astype(np.int64)
        i, j = v[:, 0] // B - x0, v[:, 1] // B - y0
        inside = (i >= 0) & (i < W) & (j >= 0) & (j < H)
        fin, q, c = fin[inside], q[inside], (j * W + i)[inside]
        pc[fin] = c
        on = out["state"][c] == 1
        with np.errstate(over="ignore", invalid="ignore"):
            ph[fin[on]] = (q[on, 2] - out["elevation"][c[on]]).astype(np.float32)
        out["point_cell"], out["point_height"] = pc, ph

    for name, _ in CELL_ARRAYS:
        out[name] = out[name].reshape(H, W)
    out["info"] = dict(n_voxels=len(key), n_points=n_points, x0=x0, y0=y0, width=W, height=H, n_class=n_class, cell_size=B * leaf)
    return out


def np_ref_ident():
    return np.array([0, 0, 0, 1, 0, 0, 0.0])
