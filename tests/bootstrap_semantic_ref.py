"""numpy restatement of the label-aware initial alignment (sicp_bootstrap_semantic; INTEGRATION.md "Bootstrap", "With
labels") on top of tests/bootstrap_ref.py, which it imports and leaves alone: the ignore list beside the box filter, the
label vote of every voxel, the feature k-NN among the target keypoints of the source keypoint's label, SAC-IA's sampling
over the keypoints that have such a neighbour, and the truncated error that takes a neighbour of another label for an
outlier.  Test-only."""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

import bootstrap_ref as R


def kept(xyz, labels, box_max=35.0, ignore=()):
    """the points the voxel grid sees: finite, inside the box, label not ignored -- (xyz f32, labels uint32), caller order"""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    l = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert len(p) == len(l)
    ok = np.isfinite(p).all(axis=1)
    ok &= (p[:, 0].astype(np.float64) < box_max) & (p[:, 1].astype(np.float64) < box_max) & (p[:, 2].astype(np.float64) < box_max)
    if len(ignore):
        ok &= ~np.isin(l, np.asarray(list(ignore), dtype=np.uint32))
    return p[ok], l[ok]


def voxel_ids(p, leaf=0.4):
    """the voxel index of every kept point (bootstrap_ref.voxel_keypoints' own rule) -- ascending index = keypoint order"""
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(p * inv).astype(np.int64)
    mn = np.floor(p.min(axis=0) * inv).astype(np.int64)
    mx = np.floor(p.max(axis=0) * inv).astype(np.int64)
    div = mx - mn + 1
    rel = ijk - mn
    return rel[:, 0] + rel[:, 1] * div[0] + rel[:, 2] * div[0] * div[1]


def vote(vid, labels):
    """per occupied voxel in ascending index: the most frequent label, ties to the smallest; and the voxels' point counts"""
    order = np.argsort(vid, kind="stable")
    vs, ls = vid[order], labels[order]
    starts = np.flatnonzero(np.r_[True, vs[1:] != vs[:-1]])
    counts = np.diff(np.r_[starts, len(vs)])
    out = np.empty(len(starts), np.uint32)
    for k, (b, c) in enumerate(zip(starts, counts)):
        u, n = np.unique(ls[b:b + c], return_counts=True)  # ascending labels: argmax takes the smallest of equal counts
        out[k] = u[np.argmax(n)]
    return out, counts


def voxel_keypoints(xyz, labels, box_max=35.0, leaf=0.4, ignore=(), stats=None):
    """(keypoints f32 [m, 3], their labels uint32 [m]): bootstrap_ref's centroids over the kept points, and the vote.
    `stats` receives "counts" (points per voxel), "ties" (voxels whose two most frequent labels are level) and
    "n_labels" (distinct labels per voxel)."""
    p, l = kept(xyz, labels, box_max, ignore)
    if len(p) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.uint32)
    kp = R.voxel_keypoints(p, box_max=box_max, leaf=leaf)
    vid = voxel_ids(p, leaf)
    kl, counts = vote(vid, l)
    assert len(kl) == len(kp)
    if stats is not None:
        order = np.argsort(vid, kind="stable")
        starts = np.r_[0, np.cumsum(counts)]
        ties, n_labels = [], []
        for k in range(len(counts)):
            _, n = np.unique(l[order][starts[k]:starts[k + 1]], return_counts=True)
            n = np.sort(n)[::-1]
            ties.append(len(n) > 1 and n[0] == n[1])
            n_labels.append(len(n))
        stats.update(counts=counts, ties=np.array(ties), n_labels=np.array(n_labels), voxel_ids=np.unique(vid))
    return kp, kl


def feature_knn(sf, tf, k, sl, tl):
    """row i: the k nearest target features among the target keypoints with a feature and label sl[i] (bootstrap_ref's
    distance, order and ties); -1 beyond them, and everywhere for a source keypoint without a feature"""
    out = np.full((len(sf), k), -1, np.int32)
    for lab in np.unique(sl):
        rows = np.flatnonzero(sl == lab)
        masked = tf.copy()
        masked[tl != lab] = np.nan  # (a row without a feature is NaN in every bin: bootstrap_ref passes it over)
        out[rows] = R.feature_knn(sf[rows], masked, k)
    return out


def truncated_error(M, src_kp, src_l, tgt_tree, tgt_kp, tgt_l, t, same_label=True):
    """(error, the keypoints within t whose nearest target keypoint has another label)"""
    q = R.transform_f32(M, src_kp)
    _, j = tgt_tree.query(q.astype(np.float64))
    e = R.d2_f32(q, tgt_kp[j]).astype(np.float64)
    t = float(np.float32(t))
    inl = e <= t
    wrong = inl & (tgt_l[j] != src_l)
    if same_label:
        inl = inl & ~wrong
    return float(np.sum(np.where(inl, e / t, 1.0))), int(wrong.sum())


def sac_ia(src_kp, src_f, src_l, tgt_kp, tgt_f, tgt_l, match_same_label=True, score_same_label=True, knn=None, stats=None, **kw):
    """bootstrap_ref.sac_ia with the label rules: (best iteration, its error, all errors, all matrices).  `stats` receives
    bootstrap_ref's entries ("halvings", "draws", "samples", "ambiguous") and "k_eff" (per source keypoint with
    match_same_label, else the one number), "sampleable" (the keypoints selectSamples runs over), "short_rows" (sampleable
    rows with fewer than k neighbours), "unsampleable" (keypoints with a feature and no neighbour of their label) and
    "label_rejects" (per hypothesis: keypoints within the threshold of a target keypoint of another label)."""
    P = dict(R.DEFAULTS, **kw)
    halvings = draws = 0
    samples, ambiguous, rejects = [], [], []
    k, nr = P["k_correspondences"], P["nr_samples"]
    has_f = ~np.isnan(src_f[:, 0])
    if match_same_label:
        if knn is None:
            knn = feature_knn(src_f, tgt_f, k, src_l, tgt_l)
        row_k = (knn >= 0).sum(axis=1)
        valid = np.flatnonzero(has_f & (row_k >= 1))
    else:
        if knn is None:
            knn = R.feature_knn(src_f, tgt_f, k)
        row_k = np.full(len(src_f), min(k, int((~np.isnan(tgt_f[:, 0])).sum())))
        valid = np.flatnonzero(has_f)
    rng = R.SplitMix64(P["seed"])
    tree = cKDTree(tgt_kp.astype(np.float64))
    errs, Ms = [], []
    nv = len(valid)
    if nv < nr:
        raise ValueError(f"{nv} source keypoints can be sampled")
    for _ in range(P["max_iterations"]):
        smp, fails, min_d = [], 0, np.float32(P["min_sample_distance"])
        while len(smp) < nr:
            si = int(valid[rng.index(nv)])
            draws += 1
            ok = True
            for sj in smp:
                d = src_kp[si] - src_kp[sj]
                dist = np.sqrt(np.float32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                if si == sj or dist < min_d:
                    ok = False
                    break
            if ok:
                smp.append(si)
                fails = 0
            else:
                fails += 1
            if fails >= 3 * nv:
                min_d = np.float32(min_d * np.float32(0.5))
                fails = 0
                halvings += 1
        tj = [int(knn[s, rng.index(int(row_k[s]))]) for s in smp]
        M = R.umeyama(src_kp[smp], tgt_kp[tj])
        samples.append((list(smp), tj))
        if R.fit_rank_ratio(src_kp[smp], tgt_kp[tj]) < 1e-6:
            ambiguous.append(len(Ms))
        Ms.append(M)
        e, w = truncated_error(M, src_kp, src_l, tree, tgt_kp, tgt_l, P["max_corr_distance"], score_same_label)
        errs.append(e)
        rejects.append(w)
    if stats is not None:
        stats.update(halvings=halvings, k_eff=row_k if match_same_label else int(row_k[0]) if len(row_k) else 0, draws=draws,
                     samples=samples, ambiguous=ambiguous, sampleable=valid,
                     short_rows=int(((row_k[valid] < k)).sum()), unsampleable=int((has_f & (row_k < 1)).sum()),
                     label_rejects=rejects)
    errs = np.array(errs)
    best = int(np.argmin(errs))
    return best, float(errs[best]), errs, np.array(Ms)
