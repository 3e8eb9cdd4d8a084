"""Inputs of the label-aware bootstrap tests (tests/test_bootstrap_semantic_cpu.py, tests/test_gpu_bootstrap_semantic.py):
the scene whose geometry is symmetric under a half turn and whose labels are not, a cloud crafted for the label vote and
the ignore list, and a lidar pair relabelled keypoint by keypoint for the label rules of the feature k-NN and of the score.
Every case is built so that a branch is reached; the CPU tests count that in the restatement.  numpy / scipy only."""
from __future__ import annotations

import functools

import numpy as np
from scipy.spatial.transform import Rotation

import bootstrap_cases as C
import bootstrap_ref as R
import bootstrap_semantic_ref as S

SEED = 1  # the SAC-IA seed at which the label-blind bootstrap returns the flipped pose of the symmetric scene
LEAF = np.float32(0.4)


def mat_delta(A, B):
    """(degrees, metres) between two 4x4 poses"""
    D = np.linalg.inv(A) @ B
    return float(np.degrees(np.linalg.norm(Rotation.from_matrix(D[:3, :3]).as_rotvec()))), float(np.linalg.norm(D[:3, 3]))


def mat4(M34):
    return np.vstack([np.asarray(M34, np.float64).reshape(3, 4), [0, 0, 0, 1]])


@functools.lru_cache(maxsize=None)
def symmetric_scene():
    """(source, source labels, target, target labels, T_gt).  The target is a half of a lidar sweep (label 1) and its copy
    turned by 180 degrees about z (label 2): the geometry maps onto itself under that half turn, the labels do not.  The
    source is an independent sampling of the same scene (permuted, thinned to 70 %, 3 cm of noise) moved by the inverse of
    T_gt (40 degrees of yaw, t = (2, -1, 0.1))."""
    _, _, tgt, _, _ = C.lidar_sub(6000)
    half = tgt[tgt[:, 1] > 1.0]
    target = np.concatenate([half, half @ np.diag([-1.0, -1.0, 1.0]).T]).astype(np.float32)
    tl = np.r_[np.full(len(half), 1, np.uint32), np.full(len(half), 2, np.uint32)]
    T = np.eye(4)
    T[:3, :3] = Rotation.from_euler("z", 40.0, degrees=True).as_matrix()
    T[:3, 3] = [2.0, -1.0, 0.1]
    Ti = np.linalg.inv(T)
    rng = np.random.default_rng(0)
    s = target.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]
    n = len(s)
    perm = rng.permutation(n)
    s, sl = s[perm], tl[perm]
    keep = rng.random(n) < 0.7
    s, sl = s[keep], sl[keep]
    s = (s + rng.normal(0.0, 0.03, size=s.shape)).astype(np.float32)
    return s, np.ascontiguousarray(sl), target, tl, T


@functools.lru_cache(maxsize=None)
def symmetric_reference():
    """the restatement on the symmetric scene: keypoints, labels, features of both clouds, and SAC-IA label-blind and
    label-aware at SEED (each with its stats) -- computed once for all the tests that need it, and left unchanged"""
    s, sl, t, tl, T = symmetric_scene()
    skp, skl = S.voxel_keypoints(s, sl)
    tkp, tkl = S.voxel_keypoints(t, tl)
    sf, tf = R.features(skp)["fpfh"], R.features(tkp)["fpfh"]
    blind_stats, aware_stats = {}, {}
    blind = R.sac_ia(skp, sf, tkp, tf, seed=SEED, stats=blind_stats)
    aware = S.sac_ia(skp, sf, skl, tkp, tf, tkl, seed=SEED, stats=aware_stats)
    return dict(skp=skp, skl=skl, tkp=tkp, tkl=tkl, sf=sf, tf=tf, blind=blind, blind_stats=blind_stats, aware=aware,
                aware_stats=aware_stats, T=T)


# ---- the label vote and the ignore list -----------------------------------------------------------------------------
IGNORED = 9
BIG = 0xFFFFFFFF


def _in_voxel(rng, i, j, k, n):
    """n points well inside voxel (i, j, k) of the leaf-0.4 grid"""
    return (np.array([i, j, k]) + rng.uniform(0.1, 0.9, size=(n, 3))) * float(LEAF)


@functools.lru_cache(maxsize=None)
def vote_cloud():
    """(cloud, labels, dict of the crafted voxels' (i, j, k) coordinates).  Holds: `tie`, four points labelled 7 7 3 3 (the
    vote is 3); `crowd`, 300 points of the labels 5 (120), 6 (100) and 2 (80); `extremes`, labels 0 0 BIG and `top`, BIG BIG
    0; `emptied`, only IGNORED points (gone when they are ignored); `swayed`, 9 9 9 5 5 4 (9 with, 5 without the ignored
    points); `pair`, two points labelled 8 and 2 (the vote is 2); `edge`, 65 points (one more than a wave has lanes), 32 of
    label 1 and 33 of label 4; NaN points with labels of their own; 200 scattered points of labels 1..4 around them, all
    permuted together."""
    rng = np.random.default_rng(5)
    vox = dict(tie=(3, 2, 1), crowd=(-4, 5, 0), extremes=(7, -3, 2), top=(8, -3, 2), emptied=(-9, -8, -2), swayed=(1, 9, 3),
               pair=(-2, -7, 4), edge=(10, 10, -3))
    parts = [(_in_voxel(rng, *vox["tie"], 4), [7, 7, 3, 3]),
             (_in_voxel(rng, *vox["crowd"], 300), [5] * 120 + [6] * 100 + [2] * 80),
             (_in_voxel(rng, *vox["extremes"], 3), [0, 0, BIG]),
             (_in_voxel(rng, *vox["top"], 3), [BIG, BIG, 0]),
             (_in_voxel(rng, *vox["emptied"], 5), [IGNORED] * 5),
             (_in_voxel(rng, *vox["swayed"], 6), [9, 9, 9, 5, 5, 4]),
             (_in_voxel(rng, *vox["pair"], 2), [8, 2]),
             (_in_voxel(rng, *vox["edge"], 65), [1] * 32 + [4] * 33),
             (np.full((7, 3), np.nan), [3, IGNORED, 0, BIG, 1, 2, 6]),
             (rng.uniform(-6.0, 6.0, size=(200, 3)), rng.integers(1, 5, size=200))]
    xyz = np.concatenate([p for p, _ in parts]).astype(np.float32)
    lab = np.concatenate([np.asarray(l, dtype=np.uint32) for _, l in parts])
    xyz[len(xyz) - 200 + 3, 0] = np.inf  # one non-finite point that is not NaN
    o = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[o]), np.ascontiguousarray(lab[o]), vox


def keypoint_at(kp, ijk):
    """index of the keypoint inside voxel (i, j, k) of the leaf-0.4 grid, or None"""
    hit = np.flatnonzero((np.floor(kp * (np.float32(1) / LEAF)).astype(np.int64) == np.array(ijk)).all(axis=1))
    assert len(hit) <= 1
    return int(hit[0]) if len(hit) else None


# ---- a pair relabelled keypoint by keypoint -------------------------------------------------------------------------
def labels_by_keypoint(cloud, kp_labels, fill=77):
    """point labels under which every point of keypoint k's voxel carries kp_labels[k] (so the vote returns kp_labels);
    points the box filter drops get `fill`"""
    p = np.asarray(cloud, np.float32)
    ok = np.isfinite(p).all(axis=1) & (p.astype(np.float64) < 35.0).all(axis=1)
    rank = np.unique(S.voxel_ids(p[ok], float(LEAF)), return_inverse=True)[1]
    out = np.full(len(p), fill, np.uint32)
    out[ok] = np.asarray(kp_labels, np.uint32)[rank]
    return out


ABSENT, RARE, STRADDLE, REST = 40, 20, 10, 30


@functools.lru_cache(maxsize=None)
def relabelled_pair():
    """lidar_sub(3000) with labels chosen per keypoint: in the target, STRADDLE on the keypoints 40..199 (LDS tiles 0..3 of
    the feature k-NN, none of them whole), RARE on exactly three keypoints with a feature (tiles apart), REST elsewhere; in
    the source, the labels ABSENT (not in the target), RARE, STRADDLE and REST in turn.  Returns a dict with the clouds, the
    point labels, and the restatement's keypoints, labels and features."""
    src, _, tgt, _, _ = C.lidar_sub(3000)
    skp, tkp = R.voxel_keypoints(src), R.voxel_keypoints(tgt)
    sf, tf = R.features(skp)["fpfh"], R.features(tkp)["fpfh"]
    tkl = np.full(len(tkp), REST, np.uint32)
    tkl[40:200] = STRADDLE
    with_f = np.flatnonzero(~np.isnan(tf[:, 0]))
    rare = [int(with_f[with_f >= a][0]) for a in (210, 300, len(tkp) - 70)]
    tkl[rare] = RARE
    skl = np.array([ABSENT, RARE, STRADDLE, REST], np.uint32)[np.arange(len(skp)) % 4]
    return dict(src=src, sl=labels_by_keypoint(src, skl), tgt=tgt, tl=labels_by_keypoint(tgt, tkl), skp=skp, tkp=tkp, skl=skl,
                tkl=tkl, sf=sf, tf=tf, rare=rare)


def near_identity_samples(skp, tkp, n=8, seed=2):
    """n hypotheses (source triples, target triples) each pairing three source keypoints with their nearest target
    keypoints: poses near the pair's small true motion, under which many source keypoints lie within the threshold of a
    target keypoint -- of any label"""
    rng = np.random.default_rng(seed)
    a = np.array([rng.choice(len(skp), size=3, replace=False) for _ in range(n)])
    b = R.cKDTree(tkp.astype(np.float64)).query(skp[a.ravel()].astype(np.float64))[1].reshape(n, 3)
    return a.astype(np.int32), b.astype(np.int32)


def too_few_pair():
    """a labelled pair whose source has two keypoints near each other and one outside the box: TOO_FEW_POINTS"""
    _, _, tgt, tl, _ = C.lidar_sub(2000)
    tiny = np.array([[0, 0, 0], [0.1, 0, 0], [40, 40, 40]], np.float32)
    return tiny, np.array([1, 1, 2], np.uint32), tgt, tl
