"""numpy restatement of the voxel map's label fusion (sicp_map_set_confusion / _extract_fused / _fused_labels, include/sicp.h) on
top of tests/map_ref.py's Map.  L[r][s] = math.log(cm[r][s]) per entry (glibc's log, the one std::log calls; -inf for 0).  A
histogram row's score of class s continues from 0.0 over the non-zero bins r = 1..C in ascending r with
(double)h[r] * L[r-1][s-1] -- numpy multiplies and adds in separate steps, so product and sum are rounded once each -- and the
point's own label, when it counts, is added last.  The fused label is the first arg-max; the confidence 1 / sum_s exp(score_s -
max) summed in ascending s (the library sums in a fixed tree: the two agree to a few ulp).  Beside it a slow restatement: one
voxel at a time with python floats.  numpy only: no library, no GPU."""
from __future__ import annotations

import math

import numpy as np

import map_ref
import merge_ref
import np_ref

NINF = -math.inf


class BadLabel(ValueError):
    pass


def log_matrix(cm):
    cm = np.asarray(cm, dtype=np.float64)
    assert cm.ndim == 2 and cm.shape[0] == cm.shape[1] and np.isfinite(cm).all() and (cm >= 0).all()
    return np.array([[NINF if v == 0.0 else math.log(v) for v in row] for row in cm.tolist()], dtype=np.float64)


def scores(hist, L, own=None):
    """hist [n, C + 1]; own [n] labels added last where they are in 1..C (None: no such term) -> (scores [n, C], added [n])"""
    hist = np.asarray(hist)
    n, C = hist.shape[0], L.shape[0]
    sc, added = np.zeros((n, C), np.float64), np.zeros(n, bool)
    for r in range(1, C + 1):
        live = hist[:, r] > 0
        if live.any():
            prod = hist[live, r].astype(np.float64)[:, None] * L[r - 1][None, :]
            sc[live] = sc[live] + prod
            added |= live
    if own is not None:
        own = np.asarray(own, dtype=np.int64)
        live = (own >= 1) & (own <= C)
        sc[live] = sc[live] + L[own[live] - 1]
        added |= live
    return sc, added


def posterior(sc, added):
    """(label uint32 -- 0 without evidence --, confidence, evidence)"""
    n, C = sc.shape
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float64), np.zeros(0, bool)
    best = sc.max(axis=1)
    evidence = added & (best > NINF)
    safe = np.where(evidence, best, 0.0)
    t = np.zeros(n, np.float64)
    for s in range(C):
        t = t + np.exp(sc[:, s] - safe)
    label = np.where(evidence, np.argmax(sc, axis=1) + 1, 0).astype(np.uint32)  # (the first of equal maxima: the smallest class)
    with np.errstate(divide="ignore"):
        conf = np.where(evidence, 1.0 / t, 0.0)
    return label, conf, evidence


def gaps(sc, evidence):
    """per row with evidence and at least two classes: the relative gap between its two best scores (inf when the runner-up is
    -inf), and whether the two are exactly equal"""
    s = np.sort(sc[evidence], axis=1)
    if s.shape[1] < 2 or not len(s):
        return np.zeros(0), np.zeros(0, bool)
    a, b = s[:, -1], s[:, -2]
    tie = a == b
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(np.isinf(b), np.inf, (a - b) / np.maximum(np.abs(a), np.abs(b)))
    g = np.where(tie, 0.0, g)
    return g, tie


def extract_fused(m: map_ref.Map, L, min_count=1, center=(0.0, 0.0, 0.0), crop_range=0.0):
    """Map.extract under the same selection with "labels" the fused ones and "confidence" beside them"""
    out = m.extract(min_count, center, crop_range)
    label, conf, _ = posterior(*scores(out["hist"], L))
    out["labels"], out["confidence"] = label, conf
    return out


def fused_labels(m: map_ref.Map, L, xyz, labels=None, qt=None, include_own=True, min_count=1):
    """(labels uint32 [n], confidence [n]) for every point of the scan in caller order; BadLabel when include_own and a finite
    point's label is above the classes"""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n, C = len(xyz), m.C
    fin = np.isfinite(xyz).all(axis=1)
    lab = None if labels is None else np.asarray(labels, dtype=np.uint32)
    if include_own and lab is not None and fin.any() and int(lab[fin].max()) > C:
        raise BadLabel(f"label {int(lab[fin].max())} above num_classes {C}")
    p = np_ref.transform_points(np_ref.qt_to_mat(merge_ref.IDENT if qt is None else np.asarray(qt, dtype=np.float64)), xyz[fin])
    inv = np.float32(1.0) / np.float32(m.leaf)
    v = np.floor((p * inv).astype(np.float32))
    in_grid = (np.abs(v) < merge_ref.LIMIT).all(axis=1)  # (beyond the key's range: not in the map)
    hist = np.zeros((len(p), C + 1), np.uint32)
    if len(m.key) and in_grid.any():
        k = map_ref.keys_of(v[in_grid].astype(np.int64))
        r = np.searchsorted(m.key, k)
        rc = np.minimum(r, len(m.key) - 1)
        found = (r < len(m.key)) & (m.key[rc] == k) & (m.cnt[rc] >= min_count)
        rows = np.flatnonzero(in_grid)[found]
        hist[rows] = m.hist[rc[found]]
    own_raw = np.zeros(len(p), np.uint32) if lab is None else lab[fin]
    own = own_raw if (include_own and lab is not None) else None
    label, conf, evidence = posterior(*scores(hist, L, own))
    out_l, out_c = np.zeros(n, np.uint32), np.zeros(n, np.float64)
    out_l[fin] = np.where(evidence, label, own_raw)
    out_c[fin] = conf
    return out_l, out_c


# ---- the slow restatement: one voxel at a time, python floats ---------------------------------------------------------------
def fuse_slow(row, L, own=0):
    """(label, confidence) of one histogram row (a sequence of C + 1 counts) with the own label added last"""
    C = len(L)
    sc, added = [0.0] * C, False
    for r in range(1, C + 1):
        if row[r] > 0:
            for s in range(C):
                sc[s] = sc[s] + float(int(row[r])) * float(L[r - 1][s])
            added = True
    if 1 <= own <= C:
        for s in range(C):
            sc[s] = sc[s] + float(L[own - 1][s])
        added = True
    best = max(sc)
    if not added or best == NINF:
        return 0, 0.0
    t = 0.0
    for s in range(C):
        t = t + math.exp(sc[s] - best)
    return sc.index(best) + 1, 1.0 / t
