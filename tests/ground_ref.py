"""numpy restatement of sicp_segment_ground (include/sicp.h, "ground of a cloud", rules 1 - 9), written from the header's text.
Imports nothing of the product.

Every operation is a float64 operation of numpy or of Python's float, rounded on its own in the order the rules give.  A sum
over a set (rule 5) is formed lane by lane: the cell's members lie in rows of 64, a member outside the set contributes +0.0
(a sum that begins at +0.0 is never -0.0, so adding +0.0 changes nothing: the same bytes as leaving the member out -- the naive
twin in test_ground_cpu.py leaves it out), np.cumsum down the rows adds in ascending j, and six pairwise steps combine the
lanes.  The Jacobi is plane_ref's, rotation by rotation."""
import math

import numpy as np

import plane_ref

MAX_RINGS, MAX_SECTORS, MAX_IGNORE = 64, 256, 16
EMPTY, GROUND, TOO_FEW, NOT_UPRIGHT, TOO_HIGH, TOO_THICK = range(6)
TWO_PI = 6.283185307179586
DEFAULTS = dict(n_rings=16, n_sectors=32, min_range=2.7, max_range=80.0, sensor_height=1.73, max_below=1.0, n_lpr=20, th_seeds=0.5,
                th_dist=0.2, n_iter=3, min_points=10, min_cos=0.707, elevation_rings=4, max_elevation=0.5, max_thickness=0.0, select=0,
                ignore=())
POINT_ARRAYS = ("ground", "cell", "height")
CELL_ARRAYS = ("status", "n_members", "n_ground", "n_fit", "normal", "centroid", "lambda_min", "lpr")
COUNTS = ("n_points", "n_finite", "n_candidates", "n_below", "n_cells")  # and "n_ground_total" (info.n_ground), "cells"


class TooFewPoints(ValueError):
    pass


def check_params(P, labels, ring_edge):
    """rule 9's ranges"""
    doubles = [P[k] for k in ("min_range", "max_range", "sensor_height", "max_below", "th_seeds", "th_dist", "min_cos", "max_elevation", "max_thickness")]
    if not all(math.isfinite(v) for v in doubles):
        raise ValueError("a double is not finite")
    R, S = P["n_rings"], P["n_sectors"]
    if P["min_range"] < 0 or not P["max_range"] > P["min_range"]:
        raise ValueError("range")
    if not 1 <= R <= MAX_RINGS or not 4 <= S <= MAX_SECTORS or S % 2:
        raise ValueError("grid")
    if ring_edge is not None:
        e = [float(v) for v in ring_edge]
        if len(e) != R + 1 or not all(math.isfinite(v) for v in e) or e[0] < 0 or any(not e[i + 1] > e[i] for i in range(R)):
            raise ValueError("ring_edge")
    if not 1 <= P["n_lpr"] <= 64 or not 1 <= P["n_iter"] <= 8 or P["min_points"] < 3 or not 0 <= P["elevation_rings"] <= R:
        raise ValueError("a count")
    if not 0.0 < P["min_cos"] <= 1.0 or not P["th_dist"] > 0 or not P["th_seeds"] > 0 or P["max_thickness"] < 0:
        raise ValueError("a threshold")
    if len(P["ignore"]) > MAX_IGNORE or (labels is None and len(P["ignore"])) or P["select"] not in (0, 1, 2):
        raise ValueError("ignore / select")


def make_tables(R, S, min_range, max_range, ring_edge=None):
    """rule 2: {"edge2": [R+1], "cos_half": [S/2], "sin_half": [S/2]} in float64, element by element with libm"""
    ring_step = (float(max_range) - float(min_range)) / float(R)
    sector_step = TWO_PI / float(S)
    edge = [float(ring_edge[i]) if ring_edge is not None else float(min_range) + float(i) * ring_step for i in range(R + 1)]
    return {"edge2": np.array([b * b for b in edge], np.float64),
            "cos_half": np.array([math.cos(float(j) * sector_step) for j in range(S // 2)], np.float64),
            "sin_half": np.array([math.sin(float(j) * sector_step) for j in range(S // 2)], np.float64)}


def ordered_bits(z32):
    """rule 3: the order-preserving map of float32 bits"""
    b = np.ascontiguousarray(z32, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def cells_of(d, tables, R, S):
    """rules 1 and 2 for the rows of d (float64, finite): (inside[n], cell[n] with -1 outside)"""
    edge2, cos_half, sin_half = tables["edge2"], tables["cos_half"], tables["sin_half"]
    dx, dy = d[:, 0], d[:, 1]
    r2 = dx * dx + dy * dy
    inside = (r2 >= edge2[0]) & (r2 < edge2[R])
    ring = (r2[:, None] >= edge2[None, 1:R]).sum(axis=1)
    lower = ~((dy > 0) | ((dy == 0) & (dx > 0)))
    xp, yp = np.where(lower, -dx, dx), np.where(lower, -dy, dy)
    sector = ((cos_half[None, 1:] * yp[:, None] - sin_half[None, 1:] * xp[:, None]) >= 0.0).sum(axis=1) + np.where(lower, S // 2, 0)
    return inside, np.where(inside, ring * S + sector, -1).astype(np.int64)


def set_sums(terms, in_set):
    """rule 5's sum of every column of terms [m, k] over the members with in_set [m]: the lanes, then the pairs"""
    m, k = terms.shape
    rows = (m + 63) // 64
    t = np.zeros((rows * 64 + 64, k), np.float64)  # (row 0: every lane begins at +0.0)
    t[64:64 + m] = np.where(in_set[:, None], terms, 0.0)
    T = np.cumsum(t.reshape(rows + 1, 64, k), axis=0)[-1]
    lane = np.arange(64)
    for step in range(6):
        T = T + T[lane ^ (1 << step)]
    return T[0]


def smallest_eigenpair(Q):
    """rule 5: Q = (xx, yx, yy, zx, zy, zz) -> (the eigenvector column of smallest |eigenvalue|, the last one at ties, and the
    diagonal entry of that column)"""
    Q = [float(v) for v in Q]
    A = [[Q[0], Q[1], Q[3]], [Q[1], Q[2], Q[4]], [Q[3], Q[4], Q[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(30):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2]
        if off <= 1e-300 or off <= 1e-34 * dia:
            break
        plane_ref.jacobi_rotate(A, V, 0, 1)
        plane_ref.jacobi_rotate(A, V, 0, 2)
        plane_ref.jacobi_rotate(A, V, 1, 2)
    col, em = 0, abs(A[0][0])
    for c in (1, 2):
        if abs(A[c][c]) <= em:
            em, col = abs(A[c][c]), c
    return [V[0][col], V[1][col], V[2][col]], A[col][col]


def plane_distance(d, u, g):
    e = d - np.array(g, np.float64)
    return (u[0] * e[:, 0] + u[1] * e[:, 1]) + u[2] * e[:, 2]


def fit_cell(d, ring, P):
    """rules 4 - 6 for one cell's members d [m, 3] (float64, in segment order): (status, lpr, u, g, lambda_min, n_fit, ground[m])"""
    m = len(d)
    L = min(P["n_lpr"], m)
    s = 0.0
    for k in range(L):
        s = s + float(d[k, 2])
    lpr = s / float(L)
    in_set = d[:, 2] < (lpr + float(P["th_seeds"]))
    none = np.zeros(m, bool)
    u = g = lam = None
    n_fit = 0
    for _ in range(P["n_iter"]):
        count = int(in_set.sum())
        if count < P["min_points"]:
            return TOO_FEW, lpr, None, None, None, 0, none
        S = set_sums(d, in_set)
        g = [float(S[0]) / float(count), float(S[1]) / float(count), float(S[2]) / float(count)]
        e = d - np.array(g, np.float64)
        Q = set_sums(np.stack([e[:, 0] * e[:, 0], e[:, 1] * e[:, 0], e[:, 1] * e[:, 1], e[:, 2] * e[:, 0], e[:, 2] * e[:, 1], e[:, 2] * e[:, 2]], axis=1), in_set)
        u, lam = smallest_eigenpair(Q)
        if u[2] < 0.0:
            u = [-u[0], -u[1], -u[2]]
        n_fit = count
        in_set = plane_distance(d, u, g) < float(P["th_dist"])
    mt = float(P["max_thickness"])
    if not u[2] >= float(P["min_cos"]):
        status = NOT_UPRIGHT
    elif ring < P["elevation_rings"] and g[2] >= -float(P["sensor_height"]) + float(P["max_elevation"]):
        status = TOO_HIGH
    elif mt > 0.0 and lam > (mt * mt) * float(n_fit):
        status = TOO_THICK
    else:
        return GROUND, lpr, u, g, lam, n_fit, in_set
    return status, lpr, None, None, None, 0, none


def segment_ground(xyz, labels=None, mask=None, sensor_origin=None, ring_edge=None, **params):
    """the call: the per-point and per-cell arrays of rule 8, the counts of sicp_ground_info ("cells": per status), and "selected":
    the caller indices select hands to dst (None with select = 0)"""
    P = dict(DEFAULTS, **params)
    P["ignore"] = tuple(int(v) for v in P["ignore"])
    check_params(P, labels, ring_edge)
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_points = len(xyz)
    R, S = P["n_rings"], P["n_sectors"]
    origin = np.zeros(3) if sensor_origin is None else np.asarray(sensor_origin, np.float64)
    tables = make_tables(R, S, P["min_range"], P["max_range"], ring_edge)
    finite = np.isfinite(xyz).all(axis=1)
    d = np.where(finite[:, None], xyz, np.float32(0)).astype(np.float64) - origin[None, :]
    inside, cell = cells_of(d, tables, R, S)
    inside &= finite
    cell = np.where(inside, cell, -1)
    ok = inside.copy()
    if mask is not None:
        ok &= np.asarray(mask).reshape(n_points) != 0
    if labels is not None and len(P["ignore"]):
        ok &= ~np.isin(np.asarray(labels, np.uint32), np.asarray(P["ignore"], np.uint32))
    bound = -(float(P["sensor_height"]) + float(P["max_below"]))
    cand = ok & (d[:, 2] >= bound)
    n_below = int((ok & ~cand).sum())
    # rule 3
    idx = np.flatnonzero(cand)
    key = (cell[idx].astype(np.uint64) << np.uint64(32)) | ordered_bits(xyz[idx, 2]).astype(np.uint64)
    order = idx[np.argsort(key, kind="stable")]
    members = np.bincount(cell[order], minlength=R * S).astype(np.int64) if len(order) else np.zeros(R * S, np.int64)
    begin = np.concatenate([[0], np.cumsum(members)])
    nan = float("nan")
    out = {"ground": np.zeros(n_points, np.uint8), "cell": cell.astype(np.int32), "height": np.full(n_points, nan, np.float64),
           "status": np.zeros(R * S, np.uint8), "n_members": members.astype(np.int32), "n_ground": np.zeros(R * S, np.int32),
           "n_fit": np.zeros(R * S, np.int32), "normal": np.full((R * S, 3), nan), "centroid": np.full((R * S, 3), nan),
           "lambda_min": np.full(R * S, nan), "lpr": np.full(R * S, nan)}
    model = {}
    for c in np.flatnonzero(members):
        seg = order[begin[c]:begin[c + 1]]
        status, lpr, u, g, lam, n_fit, ground = fit_cell(d[seg], int(c) // S, P)
        out["status"][c], out["lpr"][c] = status, lpr
        if status == GROUND:
            out["ground"][seg[ground]] = 1
            out["n_ground"][c], out["n_fit"][c] = int(ground.sum()), n_fit
            out["normal"][c], out["lambda_min"][c] = u, lam
            out["centroid"][c] = [g[k] + float(origin[k]) for k in range(3)]
            model[int(c)] = (u, g)
    # rule 7
    for s in range(S):
        found = None
        for r in range(R):
            found = model.get(r * S + s, found)
            if found is not None:
                at = np.flatnonzero(cell == r * S + s)
                out["height"][at] = plane_distance(d[at], *found)
    selected = None
    if P["select"]:
        selected = np.flatnonzero(finite & ((out["ground"] != 0) == (P["select"] == 2)))
    out.update(n_points=n_points, n_finite=int(finite.sum()), n_candidates=int(cand.sum()), n_below=n_below,
               n_ground_total=int(out["ground"].sum()), n_cells=R * S, cells=np.bincount(out["status"], minlength=6).tolist(),
               selected=selected, tables=tables)
    return out
