"""numpy restatement of the persistent voxel map (sicp_map_*, include/sicp.h) on top of tests/merge_ref.py's gather, crop_mask
and voxel_coords: per voxel the 63-bit key, the float64 sums, the count and the label histogram, in arrays sorted by key.  An
integrate continues every touched voxel's sums from the stored value with the scan's points in ascending point index, one add
per point -- the left fold that merge_ref.merge runs from zero, resumed.  Beside it MapSlow: the same rules point by point with
python floats, a dict keyed by voxel and collections.Counter.  numpy only: no library, no GPU."""
from __future__ import annotations

import collections

import numpy as np

import merge_ref

BIAS = merge_ref.LIMIT


class BadLabel(ValueError):
    pass


def keys_of(v):
    """three biased 21-bit coordinates, z highest (merge_key_kernel's key)"""
    v = np.asarray(v, dtype=np.int64)
    return ((v[:, 2] + BIAS) << 42) | ((v[:, 1] + BIAS) << 21) | (v[:, 0] + BIAS)


def _scan_points(xyz, labels, qt, center, crop_range, leaf, num_classes):
    """the kept points of a scan in point order: positions float32, labels (None when the map keeps none), voxel coordinates.
    Refusals in the library's order: no labels, grid range, label range."""
    if num_classes > 0 and labels is None:
        raise ValueError("a cloud without labels into a map that keeps labels")
    p, lab = merge_ref.gather([(xyz, labels)], None if qt is None else [qt])
    n_in = len(p)
    keep = merge_ref.crop_mask(p, center, crop_range)
    p = p[keep]
    lab = lab[keep] if (lab is not None and num_classes > 0) else None
    v = merge_ref.voxel_coords(p, leaf)
    if lab is not None and len(lab) and int(lab.max()) > num_classes:
        raise BadLabel(f"label {int(lab.max())} above num_classes {num_classes}")
    return n_in, p, lab, v


class Map:
    def __init__(self, leaf=0.2, num_classes=0):
        self.leaf, self.C = leaf, num_classes
        self.clear()

    def clear(self):
        self.key = np.zeros(0, np.int64)
        self.s = np.zeros((0, 3), np.float64)
        self.cnt = np.zeros(0, np.int64)
        self.hist = np.zeros((0, self.C + 1), np.uint32)

    def size(self):
        return len(self.key), int(self.cnt.sum())

    def integrate(self, xyz, labels=None, qt=None, center=(0.0, 0.0, 0.0), crop_range=0.0):
        """{"n_in", "n_kept", "n_scan_voxels", "n_new_voxels", "n_voxels"}; a refusal raises before anything changes"""
        n_in, p, lab, v = _scan_points(xyz, labels, qt, center, crop_range, self.leaf, self.C)
        info = dict(n_in=n_in, n_kept=len(p), n_scan_voxels=0, n_new_voxels=0, n_voxels=len(self.key))
        if not len(p):
            return info
        k = keys_of(v)
        order = np.argsort(k, kind="stable")  # by key, then point index
        ks, ps = k[order], p[order].astype(np.float64)
        uniq, starts, counts = np.unique(ks, return_index=True, return_counts=True)
        keys = np.union1d(self.key, uniq)
        old = np.searchsorted(keys, self.key)
        s, cnt, hist = np.zeros((len(keys), 3)), np.zeros(len(keys), np.int64), np.zeros((len(keys), self.C + 1), np.uint32)
        s[old], cnt[old], hist[old] = self.s, self.cnt, self.hist
        rows = np.searchsorted(keys, uniq)
        acc = s[rows]
        for j in range(int(counts.max())):  # sequential per voxel, from the stored value
            live = counts > j
            acc[live] += ps[starts[live] + j]
        s[rows] = acc
        cnt[rows] += counts
        if lab is not None:
            np.add.at(hist, (np.repeat(rows, counts), lab[order].astype(np.int64)), 1)
        info.update(n_scan_voxels=len(uniq), n_new_voxels=len(keys) - len(self.key), n_voxels=len(keys))
        self.key, self.s, self.cnt, self.hist = keys, s, cnt, hist
        return info

    def centroids(self):
        return (self.s / self.cnt[:, None]).astype(np.float32)

    def prune(self, center, crop_range):
        keep = merge_ref.crop_mask(self.centroids(), center, crop_range)
        removed = int((~keep).sum())
        self.key, self.s, self.cnt, self.hist = self.key[keep], self.s[keep], self.cnt[keep], self.hist[keep]
        return removed

    def extract(self, min_count=1, center=(0.0, 0.0, 0.0), crop_range=0.0):
        """{"xyz", "labels" (None without), "count", "hist" (None without), "n_out", "max_voxel_points", "has_label", "n_voxels"}"""
        c = self.centroids()
        sel = (self.cnt >= min_count) & merge_ref.crop_mask(c, center, crop_range)
        count = self.cnt[sel].astype(np.uint32)
        hist = self.hist[sel].copy() if self.C > 0 else None
        return dict(xyz=c[sel], labels=None if hist is None else np.argmax(hist, axis=1).astype(np.uint32), count=count, hist=hist,
                    n_out=int(sel.sum()), max_voxel_points=int(count.max()) if len(count) else 0, has_label=int(self.C > 0),
                    n_voxels=len(self.key))


class MapSlow:
    """the same rules point by point: python floats for the sums, a dict keyed by (vz, vy, vx), collections.Counter labels"""

    def __init__(self, leaf=0.2, num_classes=0):
        self.leaf, self.C = leaf, num_classes
        self.cells = {}

    def integrate(self, xyz, labels=None, qt=None, center=(0.0, 0.0, 0.0), crop_range=0.0):
        _, p, lab, v = _scan_points(xyz, labels, qt, center, crop_range, self.leaf, self.C)
        for g in range(len(p)):
            cell = self.cells.setdefault((int(v[g, 2]), int(v[g, 1]), int(v[g, 0])), [0.0, 0.0, 0.0, 0, collections.Counter()])
            cell[0] += float(p[g, 0]); cell[1] += float(p[g, 1]); cell[2] += float(p[g, 2])
            cell[3] += 1
            if lab is not None:
                cell[4][int(lab[g])] += 1

    def extract(self, min_count=1):
        keys = [k for k in sorted(self.cells) if self.cells[k][3] >= min_count]
        xyz = np.array([[np.float32(self.cells[k][a] / self.cells[k][3]) for a in range(3)] for k in keys], dtype=np.float32).reshape(-1, 3)
        count = np.array([self.cells[k][3] for k in keys], dtype=np.uint32)
        labels = None
        if self.C > 0:
            labels = np.array([min(self.cells[k][4].items(), key=lambda kv: (-kv[1], kv[0]))[0] for k in keys], dtype=np.uint32)
        return dict(xyz=xyz, labels=labels, count=count, n_out=len(keys), max_voxel_points=int(count.max()) if len(count) else 0)


def chained_merge(scans, qts=None, leaf=0.2, center=(0.0, 0.0, 0.0), crop_range=0.0):
    """the rolling-map recipe the map replaces: map = merge(map, scan), the map going back in as a part at the identity -- every
    map point then counts as ONE observation, whatever its voxel's count was"""
    out = None
    for i, scan in enumerate(scans):
        q = merge_ref.IDENT if qts is None else np.asarray(qts, dtype=np.float64).reshape(-1, 7)[i]
        parts = [scan] if out is None else [(out["xyz"], out["labels"]), scan]
        pose = np.stack([q]) if out is None else np.stack([merge_ref.IDENT, q])
        out = merge_ref.merge(parts, pose, leaf, center, crop_range)
    return out
