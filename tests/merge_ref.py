"""numpy restatement of sicp_merge_clouds (include/sicp.h): the finite points of every part in caller order, transformed by
np_ref.transform_points with np_ref.qt_to_mat (double, no contraction, one rounding to float32), cropped in float32 about the
float32 centre, keyed by floor(p * (1.0f / leaf)) on an absolute grid, and per voxel -- ascending (vz, vy, vx) -- the
sequential float64 sum in ascending global index divided by the count, the count, and the most frequent label (ties to the
smallest).  Beside it: an independent slow restatement (a dict keyed by voxel, collections.Counter labels) and a line-by-line
transcription of exec/filter_range.h.  numpy only: no library, no GPU."""
from __future__ import annotations

import collections

import numpy as np

import np_ref

IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
LIMIT = 1 << 20  # |voxel coordinate| the grid refuses


class GridOverflow(ValueError):
    pass


def gather(parts, qts=None):
    """the input of the grid: transformed finite points [n_in, 3] float32 and labels (uint32 or None) in global index order"""
    pts, labs = [], []
    for i, (xyz, lab) in enumerate(parts):
        xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
        fin = np.isfinite(xyz).all(axis=1)
        qt = IDENT if qts is None else np.asarray(qts, dtype=np.float64).reshape(-1, 7)[i]
        pts.append(np_ref.transform_points(np_ref.qt_to_mat(qt), xyz[fin]))
        labs.append(None if lab is None else np.asarray(lab, dtype=np.uint32)[fin])
    with_labels = [l is not None for l in labs]
    if any(with_labels) and not all(with_labels):
        raise ValueError("labelled and unlabelled parts")
    p = np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)
    return p, (np.concatenate(labs) if pts and all(with_labels) else None)


def crop_mask(p, center, crop_range):
    if not crop_range > 0:
        return np.ones(len(p), dtype=bool)
    c32 = np.asarray(center, dtype=np.float64).astype(np.float32)
    d = (p - c32).astype(np.float32)
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    with np.errstate(over="ignore"):
        return d2.astype(np.float64) <= np.float64(crop_range) * np.float64(crop_range)


def voxel_coords(p, leaf):
    inv = np.float32(1.0) / np.float32(leaf)
    v = np.floor((p * inv).astype(np.float32))
    if len(v) and not (np.abs(v) < LIMIT).all():
        raise GridOverflow(f"leaf size {leaf}: a voxel coordinate reaches 2^20")
    return v.astype(np.int64)


def merge(parts, qts=None, leaf=0.2, center=(0.0, 0.0, 0.0), crop_range=0.0):
    """{"xyz", "labels" (None without), "count", "n_in", "n_kept", "n_out", "max_voxel_points", "has_label", "voxels" [n_out, 3]}"""
    p, lab = gather(parts, qts)
    keep = crop_mask(p, center, crop_range)
    n_in, n_kept = len(p), int(keep.sum())
    p = p[keep]
    lab = None if lab is None else lab[keep]
    out = dict(n_in=n_in, n_kept=n_kept, has_label=int(lab is not None))
    if not leaf > 0:
        out.update(xyz=p.copy(), labels=None if lab is None else lab.copy(), count=np.ones(n_kept, np.uint32), n_out=n_kept,
                   max_voxel_points=1 if n_kept else 0, voxels=None)
        return out
    v = voxel_coords(p, leaf)
    order = np.lexsort((np.arange(len(p)), v[:, 0], v[:, 1], v[:, 2]))  # (vz, vy, vx), then global index
    vs, ps = v[order], p[order].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, (vs[1:] != vs[:-1]).any(axis=1)]) if len(vs) else np.zeros(0, np.int64)
    counts = np.diff(np.r_[starts, len(vs)]).astype(np.int64)
    acc = np.zeros((len(starts), 3))
    for j in range(int(counts.max()) if len(counts) else 0):  # sequential per voxel
        live = counts > j
        acc[live] += ps[starts[live] + j]
    xyz = (acc / counts[:, None]).astype(np.float32)
    labels = None
    if lab is not None:
        ls = lab[order]
        labels = np.empty(len(starts), np.uint32)
        for k, (b, c) in enumerate(zip(starts, counts)):
            u, n = np.unique(ls[b:b + c], return_counts=True)  # ascending labels: argmax takes the smallest of equal counts
            labels[k] = u[np.argmax(n)]
    out.update(xyz=xyz, labels=labels, count=counts.astype(np.uint32), n_out=len(starts),
               max_voxel_points=int(counts.max()) if len(counts) else 0, voxels=vs[starts] if len(vs) else np.zeros((0, 3), np.int64))
    return out


def merge_slow(parts, qts=None, leaf=0.2, center=(0.0, 0.0, 0.0), crop_range=0.0):
    """the same rules point by point: python floats for the sums, a dict keyed by voxel, collections.Counter for the labels"""
    p, lab = gather(parts, qts)
    c32 = np.asarray(center, dtype=np.float64).astype(np.float32)
    inv = np.float32(1.0) / np.float32(leaf) if leaf > 0 else None
    cells = collections.OrderedDict()
    kept = 0
    for g in range(len(p)):
        q = p[g]
        if crop_range > 0:
            dx, dy, dz = np.float32(q[0] - c32[0]), np.float32(q[1] - c32[1]), np.float32(q[2] - c32[2])
            d2 = np.float32(np.float32(np.float32(dx * dx) + np.float32(dy * dy)) + np.float32(dz * dz))
            if not float(d2) <= float(crop_range) * float(crop_range):
                continue
        kept += 1
        if inv is None:
            key = (0, 0, g)
        else:
            key = tuple(int(np.floor(np.float32(q[a] * inv))) for a in (2, 1, 0))
        cell = cells.setdefault(key, [0.0, 0.0, 0.0, 0, collections.Counter()])
        cell[0] += float(q[0]); cell[1] += float(q[1]); cell[2] += float(q[2])
        cell[3] += 1
        if lab is not None:
            cell[4][int(lab[g])] += 1
    keys = sorted(cells)
    xyz = np.array([[np.float32(cells[k][a] / cells[k][3]) for a in range(3)] for k in keys], dtype=np.float32).reshape(-1, 3)
    count = np.array([cells[k][3] for k in keys], dtype=np.uint32)
    labels = None
    if lab is not None:
        labels = np.array([min(cells[k][4].items(), key=lambda kv: (-kv[1], kv[0]))[0] for k in keys], dtype=np.uint32)
    return dict(xyz=xyz, labels=labels, count=count, n_in=len(p), n_kept=kept, n_out=len(keys),
                max_voxel_points=int(count.max()) if len(count) else 0, has_label=int(lab is not None))


def filter_range(points, rng):
    """exec/filter_range.h:5-18 line by line on a list of (x, y, z, label) with float32 coordinates: a point is erased when
    pt.x*pt.x + pt.y*pt.y + pt.z*pt.z (float32, left to right) > range*range (double)"""
    cloud = list(points)
    it = 0
    while it != len(cloud):
        pt = cloud[it]
        x, y, z = np.float32(pt[0]), np.float32(pt[1]), np.float32(pt[2])
        if float(np.float32(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z))) > float(rng) * float(rng):
            del cloud[it]
        else:
            it += 1
    return cloud
