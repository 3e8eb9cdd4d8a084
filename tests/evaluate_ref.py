"""numpy restatement of sicp_evaluate (include/sicp.h): the nearest target of every transformed finite source point in the
whole target cloud (search_cases.np_knn on np_ref.transform_points output: float32 d^2, ties to the lower caller index), the
strict float32 gate, and over the inliers the counts, math.fsum of the d^2 and the label confusion table -- plus a literal
transcription of the loop it answers for, ROCMetrics::evaluate (exec/roc_metrics.h:21-41).  numpy only: no library, no GPU."""
from __future__ import annotations

import math

import numpy as np

import np_ref
import search_cases


def finite_rows(xyz):
    return np.isfinite(np.asarray(xyz, dtype=np.float32)).all(axis=1)


def nearest(src, tgt, qt):
    """per source point, caller order: (caller index of the nearest finite target, float32 d^2); (-1, NaN) for a non-finite
    source point.  No gate yet."""
    src, tgt = np.asarray(src, dtype=np.float32), np.asarray(tgt, dtype=np.float32)
    fs, ft = finite_rows(src), finite_rows(tgt)
    t_ids = np.nonzero(ft)[0]
    idx = np.full(len(src), -1, dtype=np.int32)
    d2 = np.full(len(src), np.nan, dtype=np.float32)
    if fs.any():
        q = np_ref.transform_points(np_ref.qt_to_mat(qt), src[fs])
        i, d = search_cases.np_knn(q, tgt[ft], 1)
        idx[fs] = t_ids[i[:, 0]]
        d2[fs] = d[:, 0]
    return idx, d2


def gate(idx, d2, max_dist_sq):
    """the per-point outputs of sicp_evaluate from nearest(): -1 where d^2 < (float) max_dist_sq does not hold, d^2 kept"""
    keep = d2 < np.float32(max_dist_sq)  # (False for the NaN of a dropped point)
    return np.where(keep, idx, -1).astype(np.int32), d2


def reduce(nn_idx, nn_d2, src_labels=None, tgt_labels=None, num_classes=None):
    """the fields of sicp_evaluate_result (and `confusion` when num_classes is given) from the per-point outputs"""
    nn_idx, nn_d2 = np.asarray(nn_idx), np.asarray(nn_d2, dtype=np.float32)
    queries = ~np.isnan(nn_d2)
    inl = nn_idx >= 0
    assert not (inl & ~queries).any()
    n_source, inliers = int(queries.sum()), int(inl.sum())
    sum_d2 = math.fsum(float(v) for v in nn_d2[inl])
    out = dict(n_source=n_source, inliers=inliers, label_agree=0, label_outside=0, sum_d2=sum_d2,
               fitness=(inliers / n_source if n_source else 0.0),
               inlier_rmse=(math.sqrt(sum_d2 / inliers) if inliers else math.nan))
    if src_labels is not None and tgt_labels is not None:
        ls = np.asarray(src_labels, dtype=np.int64)[inl]
        lt = np.asarray(tgt_labels, dtype=np.int64)[nn_idx[inl]]
        out["label_agree"] = int((ls == lt).sum())
        if num_classes is not None:
            C = int(num_classes)
            inside = (ls >= 1) & (ls <= C) & (lt >= 1) & (lt <= C)
            conf = np.zeros((C, C), dtype=np.int64)
            np.add.at(conf, (ls[inside] - 1, lt[inside] - 1), 1)
            out["confusion"] = conf
            out["label_outside"] = int((~inside).sum())
    return out


def evaluate(src, tgt, qt, max_dist_sq, src_labels=None, tgt_labels=None, num_classes=None):
    """sicp_evaluate as a whole: the result fields, `nn_idx`, `nn_d2`, and `confusion` when num_classes is given"""
    idx, d2 = gate(*nearest(src, tgt, qt), max_dist_sq)
    out = reduce(idx, d2, src_labels, tgt_labels, num_classes)
    out["nn_idx"], out["nn_d2"] = idx, d2
    return out


def roc_metrics_loop(source_xyz, source_labels, target_xyz, target_labels, threshold=25.0):
    """exec/roc_metrics.h:28-40, line by line, on an already transformed source (the driver transforms it before the call):
    for every source point the one nearest target (a brute-force scan in the place of the kd-tree, float32 squared distances,
    the first of equal ones), and when nn_dist_sq[0] < 25.0 the two labels -- the lines the reference writes to its stream."""
    lines = []
    target_xyz = np.asarray(target_xyz, dtype=np.float32)
    for p, label_source in zip(np.asarray(source_xyz, dtype=np.float32), source_labels):
        d = target_xyz - p
        dist_sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        nn_index = int(np.argmin(dist_sq))  # nearestKSearch(p, 1, ...)
        if dist_sq[nn_index] < threshold:
            lines.append((int(label_source), int(target_labels[nn_index])))
    return lines
