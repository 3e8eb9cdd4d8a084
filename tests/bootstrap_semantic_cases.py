"""Inputs of the label-aware bootstrap tests (tests/test_bootstrap_semantic_cpu.py, tests/test_gpu_bootstrap_semantic.py):
the scene whose geometry is symmetric under a half turn and whose labels are not, a cloud crafted for the label vote and
the ignore list, and a lidar pair relabelled keypoint by keypoint for the label rules of the feature k-NN and of the score.
The second half holds the inputs of the edge tests (tests/test_bootstrap_semantic_edges_cpu.py,
tests/test_gpu_bootstrap_semantic_edges.py): voxels at the point counts, label counts and unsigned ties where the vote's wave
can go wrong, a full ignore list, label patterns for the feature k-NN at keypoint counts around its tile and workgroup, crops
for the label-aware error around its 256-lane stride, and pairs the whole call must refuse.
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


# ==== the edges of the label kernels (tests/test_gpu_bootstrap_semantic_edges.py, tests/test_bootstrap_semantic_edges_cpu.py) =====
def labels_of_keypoints(cloud, kp_labels, leaf, fill=77):
    """labels_by_keypoint on a grid of another leaf"""
    p = np.asarray(cloud, np.float32)
    ok = np.isfinite(p).all(axis=1) & (p.astype(np.float64) < 35.0).all(axis=1)
    rank = np.unique(S.voxel_ids(p[ok], float(np.float32(leaf))), return_inverse=True)[1]
    out = np.full(len(p), fill, np.uint32)
    out[ok] = np.asarray(kp_labels, np.uint32)[rank]
    return out


def _voxel_walk():
    """voxel coordinates three voxels apart from each other, inside the box"""
    n = 0
    while True:
        yield (3 * (n % 10) - 15, 3 * ((n // 10) % 10) - 15, n // 100)
        n += 1


def _assemble(parts, rng, nan_rows=0, scatter=0):
    """cloud, labels and {name: (voxel, expected label)} of parts (name, labels in caller order, expected): a voxel each, the
    points of one voxel in the given order (the voxel sort is stable in the caller index, so a voxel's last point in caller
    order is its last sorted position) and the voxels one after the other; `nan_rows` NaN points spread among them"""
    walk = _voxel_walk()
    xyz, lab, vox = [], [], {}
    for name, labels, expected in parts:
        ijk = next(walk)
        xyz.append(_in_voxel(rng, *ijk, len(labels)))
        lab.append(np.asarray(labels, np.uint32))
        vox[name] = (ijk, expected)
    if scatter:
        xyz.append(rng.uniform(20.0, 30.0, size=(scatter, 3)))
        lab.append(rng.integers(1, 5, size=scatter).astype(np.uint32))
    xyz, lab = np.concatenate(xyz).astype(np.float32), np.concatenate(lab)
    if nan_rows:
        at = np.linspace(1, len(xyz) - 1, nan_rows).astype(np.int64)
        xyz = np.insert(xyz, at, np.nan, axis=0)
        lab = np.insert(lab, at, lab[at])
    return np.ascontiguousarray(xyz), np.ascontiguousarray(lab), vox


VOTE_COUNTS = (1, 63, 64, 65, 128, 129, 1001)
MID, HIGH = 0x7FFFFFFF, 0x80000000


def _two_labels(n, lo=11, hi=12, third=13):
    """n labels: hi once more than lo, alternating, hi's surplus point last; an even n has one point of `third` as well
    (two counts that differ by one have an odd sum)"""
    m = (n - 1) // 2
    return [hi, lo] * m + ([third] if n % 2 == 0 else []) + [hi]


@functools.lru_cache(maxsize=None)
def vote_edge_cloud(distinct=True, nan_rows=0):
    """(cloud, labels, {name: (voxel, expected label)}): voxels of VOTE_COUNTS points with two labels whose counts differ by
    one, the winner the larger label and its surplus point at the voxel's last sorted position (a walk that stops one point
    early sees a tie and returns the smaller); `distinct`: voxels of 64 and of 65 labels once each (the smallest wins) and
    of 200 labels once each but one twice; three exact ties which the unsigned order decides: MID / HIGH either side of
    2^31, BIG - 1 / BIG, 0 / BIG."""
    rng = np.random.default_rng(17)
    parts = [(f"count{n}", _two_labels(n), 12) for n in VOTE_COUNTS]
    if distinct:
        parts += [("distinct64", rng.permutation(np.arange(100, 164)), 100),
                  ("distinct65", rng.permutation(np.arange(200, 265)), 200),
                  ("twice", rng.permutation(np.r_[np.arange(1000, 1200), 1100]), 1100)]
    parts += [("mid", [HIGH, MID, HIGH, MID], MID), ("high", [BIG, BIG - 1, BIG, BIG - 1], BIG - 1), ("ends", [BIG, 0, 0, BIG], 0)]
    return _assemble(parts, rng, nan_rows=nan_rows)


def small_vote_cloud(n_kp):
    """a cloud of exactly n_kp keypoints: voxels of three points (a 2:1 vote for the larger label) and of two (a tie)"""
    rng = np.random.default_rng(n_kp)
    parts = [(f"v{j}", [j + 2, j + 1, j + 2], j + 2) if j % 2 == 0 else (f"v{j}", [j + 5, j + 1], j + 1) for j in range(n_kp)]
    return _assemble(parts, rng)


FULL_IGNORE = tuple([0, BIG, IGNORED, IGNORED] + list(range(100, 160)))  # 64 entries: 0, 2^32 - 1, a duplicate; 159 last


@functools.lru_cache(maxsize=None)
def full_ignore_cloud():
    """(cloud, labels, {name: (voxel, label with FULL_IGNORE, label without)}); the voxel `gone` holds ignored points only"""
    rng = np.random.default_rng(23)
    parts = [("tie_after", [9, 9, 9, 8, 8, 5, 5], (5, 9)),      # a tie only once the ignored points are gone
             ("last_entry", [159, 159, 159, 7], (7, 159)),        # the list's 64th entry
             ("zero_big", [0, 0, BIG, BIG, BIG, 6], (6, BIG)),
             ("beside", [99, 99, 160, 160, 160, 130], (160, 160)),  # the labels next to the listed range stay
             ("gone", [0, BIG, 100, 9], (None, 0))]
    cloud, lab, vox = _assemble(parts, rng, nan_rows=3, scatter=40)
    return cloud, lab, vox


# ---- the label k-NN at chosen keypoint counts -------------------------------------------------------------------------
KNN_PATTERNS = ("alternate", "last_tile", "tile0", "exact", "featureless", "absent", "extremes")
_FEW, _SOME, _ALL = ("alternate", "absent"), ("alternate", "exact", "absent"), KNN_PATTERNS
# tests/test_gpu_bootstrap_edges.py's KNN_CASES (ns, nt, k, keypoints without a feature) -> the patterns with something to show
# there (knn_label_case returns None for the others; tests/test_bootstrap_semantic_edges_cpu.py holds the two against each other)
KNN_APPLIES = {(255, 63, 10, 0): _SOME, (256, 64, 1, 0): _SOME, (257, 65, 16, 2): _ALL, (257, 129, 10, 3): _ALL, (300, 1, 10, 0): _FEW,
               (200, 5, 10, 0): _FEW, (1, 64, 10, 0): _SOME, (256, 129, 16, 0): tuple(p for p in _ALL if p != "featureless")}
KNN_LABEL_CASES = [c + (p,) for c, ps in KNN_APPLIES.items() for p in ps]


@functools.lru_cache(maxsize=None)
def knn_crops(ns, nt, iso):
    """the clouds of tests/test_gpu_bootstrap_edges.py's KNN_CASES with the restatement's keypoints and features"""
    src, _, tgt, _, _ = C.lidar()
    s = C.crop_to_keypoints(src, ns, n_isolated=min(iso, max(ns - 1, 0)))
    t = C.crop_to_keypoints(tgt, nt, n_isolated=min(iso, max(nt - 1, 0)))
    skp, tkp = R.voxel_keypoints(s), R.voxel_keypoints(t)
    return dict(s=s, t=t, skp=skp, tkp=tkp, sf=R.features(skp)["fpfh"], tf=R.features(tkp)["fpfh"])


def knn_label_case(ns, nt, k, iso, pattern):
    """the pair of knn_crops(ns, nt, iso) labelled keypoint by keypoint in one of KNN_PATTERNS, or None where the counts
    leave the pattern nothing to show.  Returns the clouds, the point labels and the keypoint labels."""
    c = knn_crops(ns, nt, iso)
    tv = np.flatnonzero(~np.isnan(c["tf"][:, 0]))
    i_s, i_t = np.arange(ns), np.arange(nt)
    t_last = (nt - 1) // 64 * 64  # the first row of the last tile
    if pattern == "alternate":  # every tile is mixed
        skl, tkl = 1 + i_s % 2, 1 + i_t % 2
    elif pattern == "last_tile":  # a label of the last, partial tile alone
        if nt % 64 == 0 or nt < 64:
            return None
        skl, tkl = 5 + i_s % 2, np.where(i_t >= t_last, 5, 6)
    elif pattern == "tile0":  # a label of tile 0 alone (every second row of it)
        if nt <= 64:
            return None
        skl, tkl = 5 + i_s % 2, np.where((i_t < 64) & (i_t % 2 == 0), 5, 6)
    elif pattern == "exact":  # labels with exactly k - 1, k and k + 1 target keypoints that have a feature
        if len(tv) < 3 * k + 1:
            return None
        pick = np.random.default_rng(k).permutation(tv)
        tkl = np.full(nt, 14)
        tkl[pick[:k - 1]], tkl[pick[k - 1:2 * k - 1]], tkl[pick[2 * k - 1:3 * k]] = 11, 12, 13
        skl = 11 + i_s % 4
    elif pattern == "featureless":  # a label on every target keypoint without a feature and on two with one
        if iso == 0 or len(tv) < 3:
            return None
        tkl = np.full(nt, 5)
        tkl[tv] = 6
        tkl[tv[[0, -1]]] = 5
        skl = 5 + i_s % 2
    elif pattern == "absent":  # a source label the target does not have
        skl, tkl = np.where(i_s % 2 == 0, ABSENT, 1), np.full(nt, 1)
    elif pattern == "extremes":  # 0 on three target keypoints with a feature and on the last keypoint, 2^32 - 1 elsewhere
        if nt not in (65, 129) or len(tv) < 4:
            return None
        tkl = np.full(nt, BIG, np.uint32)
        tkl[tv[[0, len(tv) // 2, -1]]] = 0
        tkl[nt - 1] = 0  # (the one row of the last tile, with a feature or without)
        skl = np.where(i_s % 2 == 0, 0, BIG)
    else:
        raise ValueError(pattern)
    skl, tkl = np.asarray(skl, np.uint32), np.asarray(tkl, np.uint32)
    return dict(c, skl=skl, tkl=tkl, sl=labels_by_keypoint(c["s"], skl), tl=labels_by_keypoint(c["t"], tkl))


@functools.lru_cache(maxsize=None)
def tie_label_case(kind):
    """tests/test_gpu_bootstrap_edges.py's tie clouds (the target two copies of one patch, keypoint i + m the twin of keypoint
    i) with labels: "same" -- one label everywhere; "split" -- the first copy 1, the second 2, the source keypoints 1 and 2 in
    turn"""
    tgt, m = C.tie_patches(seed=0, copies=2)
    src, ms = C.tie_patches(seed=1, copies=1)
    leaf = C.TIE_PARAMS["leaf_size"]
    if kind == "same":
        skl, tkl = np.full(ms, 3, np.uint32), np.full(2 * m, 3, np.uint32)
    else:
        skl, tkl = (1 + np.arange(ms) % 2).astype(np.uint32), np.r_[np.full(m, 1), np.full(m, 2)].astype(np.uint32)
    return dict(src=src, tgt=tgt, m=m, skl=skl, tkl=tkl, sl=labels_of_keypoints(src, skl, leaf), tl=labels_of_keypoints(tgt, tkl, leaf))


# ---- the label-aware error at chosen source keypoint counts ----------------------------------------------------------
ERROR_COUNTS = (1, 255, 256, 257, 600)
ERROR_PATTERNS = ("scatter", "wrong")


def crop_near(cloud, centre, want):
    """bootstrap_cases.crop_to_keypoints about a given centre: the points nearest to it that make exactly `want` keypoints"""
    order = np.argsort(((cloud.astype(np.float64) - np.asarray(centre, np.float64)) ** 2).sum(axis=1), kind="stable")
    count = lambda m: len(R.voxel_keypoints(cloud[np.sort(order[:m])]))
    lo, hi = want, len(cloud)
    while lo < hi:
        mid = (lo + hi) // 2
        if count(mid) >= want:
            hi = mid
        else:
            lo = mid + 1
    out = np.ascontiguousarray(cloud[np.sort(order[:lo])], np.float32)
    assert len(R.voxel_keypoints(out)) == want
    return out


@functools.lru_cache(maxsize=None)
def error_crops(ns):
    """a crop of the lidar source with exactly ns keypoints and the target's 300 keypoints (500 for the largest source) about
    the same place; the source's nearest target keypoint of every source keypoint"""
    src, _, tgt, _, _ = C.lidar()
    s = C.crop_to_keypoints(src, ns)
    t = crop_near(tgt, src[len(src) // 3], 300 if ns <= 300 else 500)
    skp, tkp = R.voxel_keypoints(s), R.voxel_keypoints(t)
    near = R.cKDTree(tkp.astype(np.float64)).query(skp.astype(np.float64))[1]
    return dict(s=s, t=t, skp=skp, tkp=tkp, near=near)


def error_label_case(ns, pattern):
    """error_crops(ns) with the target keypoints labelled 1..3 at random -- scattered in space, so that the caller order and
    the two trees' device orders all differ -- and every source keypoint labelled as its nearest target keypoint, but for
    30 % of them ("scatter") or 90 % ("wrong"), which carry another label; "absent": labels the target does not have;
    "one": one label everywhere"""
    c = error_crops(ns)
    rng = np.random.default_rng(ns)
    nt = len(c["tkp"])
    tkl = rng.integers(1, 4, size=nt).astype(np.uint32)
    skl = tkl[c["near"]].copy()
    if pattern in ERROR_PATTERNS:
        flip = rng.random(ns) < (0.3 if pattern == "scatter" else 0.9)
        if ns == 1:  # (the one keypoint: right in the one pattern, wrong in the other)
            flip[:] = pattern == "wrong"
        skl[flip] = skl[flip] % 3 + 1
    elif pattern == "absent":
        skl = skl + 10
    elif pattern == "one":
        skl[:], tkl[:] = 2, 2
    else:
        raise ValueError(pattern)
    return dict(c, skl=skl, tkl=tkl, sl=labels_by_keypoint(c["s"], skl), tl=labels_by_keypoint(c["t"], tkl))


def near_samples(skp, tkp, nr, n=8, seed=2):
    """near_identity_samples with nr pairs a hypothesis (a source of fewer than nr keypoints names some of them twice)"""
    rng = np.random.default_rng(seed)
    a = np.array([rng.choice(len(skp), size=nr, replace=len(skp) < nr) for _ in range(n)])
    b = R.cKDTree(tkp.astype(np.float64)).query(skp[a.ravel()].astype(np.float64))[1].reshape(n, nr)
    return a.astype(np.int32), b.astype(np.int32)


# ---- the whole call on ragged rows ------------------------------------------------------------------------------------
SAC_SAMPLES, SAC_KS, SAC_SEEDS, SAC_ITERATIONS = (6, 8), (1, 3, 10, 16), (1, 2, 3, 7), 60
FLAG_SETS = ((1, 1), (1, 0), (0, 1))  # (match_same_label, score_same_label)


def unsampleable_pair(nr):
    """relabelled_pair's clouds, every target keypoint REST, every source keypoint ABSENT but nr - 1 with a feature: one
    keypoint too few can be sampled, hundreds have a feature"""
    c = relabelled_pair()
    skl = np.full(len(c["skp"]), ABSENT, np.uint32)
    with_f = np.flatnonzero(~np.isnan(c["sf"][:, 0]))
    skl[with_f[np.linspace(0, len(with_f) - 1, nr - 1).astype(np.int64)]] = REST
    tkl = np.full(len(c["tkp"]), REST, np.uint32)
    return dict(src=c["src"], tgt=c["tgt"], skl=skl, tkl=tkl, sl=labels_by_keypoint(c["src"], skl), tl=labels_by_keypoint(c["tgt"], tkl),
                skp=c["skp"], tkp=c["tkp"], sf=c["sf"], tf=c["tf"])


def disjoint_pair():
    """relabelled_pair's clouds, the source all of one label and the target all of another"""
    c = relabelled_pair()
    return dict(src=c["src"], tgt=c["tgt"], sl=np.full(len(c["src"]), 1, np.uint32), tl=np.full(len(c["tgt"]), 2, np.uint32),
                skp=c["skp"], tkp=c["tkp"], sf=c["sf"], tf=c["tf"])


def increasing_map(*label_arrays):
    """l -> 1000 l + 7, the largest label of all the arrays -> 2^32 - 1: strictly increasing on them.  Returns the mapped arrays."""
    top = max(int(a.max()) for a in label_arrays)
    assert 1000 * top + 7 < BIG
    return [np.where(a == top, BIG, a.astype(np.uint64) * 1000 + 7).astype(np.uint32) for a in label_arrays]
