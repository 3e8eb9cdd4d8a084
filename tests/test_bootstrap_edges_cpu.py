"""CPU tests behind tests/test_gpu_bootstrap_edges.py: the branches of the numpy restatement tests/bootstrap_ref.py that only
the edge cases reach, pinned against plain loops and planted answers that do not use it, and the inputs of
tests/bootstrap_cases.py shown to reach the branch each was built for.  No library, no GPU."""
import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import bootstrap_cases as K
import bootstrap_ref as R


def _brute_lists(kp, r):
    """neighbour lists by the definition: every pair, f32 arithmetic written out, no search structure"""
    r2 = np.float32(r * r)
    off, idx, dd = [0], [], []
    for i in range(len(kp)):
        dx, dy, dz = (kp[:, 0] - kp[i, 0]).astype(np.float32), (kp[:, 1] - kp[i, 1]).astype(np.float32), (kp[:, 2] - kp[i, 2]).astype(np.float32)
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        row = sorted((float(d[j]), j) for j in range(len(kp)) if d[j] < r2)
        idx += [j for _, j in row]
        dd += [v for v, _ in row]
        off.append(len(idx))
    return np.array(off, np.int64), np.array(idx, np.int32), np.array(dd, np.float32)


@pytest.mark.parametrize("r,pairs", list(zip(K.LATTICE_RADII, (3510, 6048, 2964))))
def test_lattice_lists_match_a_brute_force_loop_with_pairs_exactly_on_the_radius(r, pairs):
    lat = K.lattice(K.LATTICE_S)
    vk, _ = K.ref_args(K.LATTICE_PARAMS(r))
    kp = R.voxel_keypoints(lat, **vk)
    assert len(kp) == 676 and np.array_equal(kp.view(np.uint32), lat.view(np.uint32))  # the keypoints are the lattice
    assert K.boundary_pairs(kp, r) == pairs
    assert np.float32(r * r) in (np.float32(0.25), np.float32(0.5), np.float32(1.0))  # (0.5 sqrt 2)^2 rounds to 0.5 exactly
    off, idx, d2 = R.radius_lists(kp, r)
    boff, bidx, bd2 = _brute_lists(kp, r)
    assert np.array_equal(off, boff) and np.array_equal(idx, bidx) and np.array_equal(d2.view(np.uint32), bd2.view(np.uint32))
    # with `<=` the lists would be longer by exactly the pairs on the radius
    loose = sum(int((R.d2_f32(kp, kp[i]) <= np.float32(r * r)).sum()) for i in range(len(kp)))
    assert loose == len(idx) + pairs


def test_lists_match_the_brute_force_loop_on_a_scan_crop_with_unequal_radii():
    kp = R.voxel_keypoints(K.compact(K.lidar()[0], 3000))
    assert 100 < len(kp) < 800
    for r in (0.3, 1.5, 3.0):
        off, idx, d2 = R.radius_lists(kp, r)
        boff, bidx, bd2 = _brute_lists(kp, r)
        assert np.array_equal(off, boff) and np.array_equal(idx, bidx) and np.array_equal(d2, bd2)
    # features(): the lists returned are the feature radius', the normals come from the normal radius' own
    f = R.features(kp, normal_radius=1.5, feature_radius=3.0)
    assert np.array_equal(f["off"], R.radius_lists(kp, 3.0)[0])
    n_small, _ = R.normals(kp, *R.radius_lists(kp, 1.5)[:2])
    n_large, _ = R.normals(kp, *R.radius_lists(kp, 3.0)[:2])
    assert np.array_equal(f["normals"], n_small, equal_nan=True) and not np.array_equal(n_small, n_large, equal_nan=True)


@pytest.mark.parametrize("n", [3, 4, 8])
def test_umeyama_recovers_a_planted_transform_from_n_pairs(n):
    rng = np.random.default_rng(n)
    for _ in range(20):
        s = rng.uniform(-20, 20, size=(n, 3))
        Rm = Rotation.from_rotvec(rng.normal(size=3)).as_matrix()
        t = rng.uniform(-5, 5, size=3)
        M = R.umeyama(s, s @ Rm.T + t)
        assert np.abs(M[:, :3] - Rm).max() < 1e-12 and np.abs(M[:, 3] - t).max() < 1e-11
        assert R.fit_rank_ratio(s, s @ Rm.T + t) > 1e-4
    # noisy pairs: a proper rotation, and no worse than the planted transform or than small turns away from the answer
    s = rng.uniform(-20, 20, size=(n, 3))
    Rm = Rotation.from_rotvec([0.3, -0.8, 1.1]).as_matrix()
    tg = s @ Rm.T + [1.0, 2.0, 3.0] + rng.normal(scale=0.1, size=(n, 3))
    M = R.umeyama(s, tg)
    cost = lambda Rr, tt: float((((s @ Rr.T + tt) - tg) ** 2).sum())
    assert abs(np.linalg.det(M[:, :3]) - 1.0) < 1e-12 and np.abs(M[:, :3] @ M[:, :3].T - np.eye(3)).max() < 1e-12
    best = cost(M[:, :3], M[:, 3])
    assert best <= cost(Rm, np.array([1.0, 2.0, 3.0]))
    for w in rng.normal(scale=1e-3, size=(10, 3)):
        Rw = Rotation.from_rotvec(w).as_matrix() @ M[:, :3]
        assert best <= cost(Rw, tg.mean(axis=0) - Rw @ s.mean(axis=0)) + 1e-12


def test_pairs_that_leave_a_rotation_free_are_told_apart():
    s = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], float)
    t = np.array([[5, 5, 5], [6, 5, 5], [6, 5, 5]], float)  # one target point named twice: two distinct points, a line
    assert R.fit_rank_ratio(s, t) < 1e-12
    assert R.fit_rank_ratio(s, np.repeat(t[:1], 3, axis=0)) == 0.0
    assert R.fit_rank_ratio(s, s[:, [1, 2, 0]] + 3.0) > 0.1
    # both of these are optimal fits of the ambiguous pairs (the same residual), which is why such samples are not compared
    M = R.umeyama(s, t)
    turn = Rotation.from_rotvec([0.7, 0, 0]).as_matrix()  # about the target line's direction
    c = t.mean(axis=0)
    M2 = np.hstack([turn @ M[:, :3], (c - turn @ M[:, :3] @ s.mean(axis=0))[:, None]])
    res = lambda A: float((((s @ A[:, :3].T + A[:, 3]) - t) ** 2).sum())
    assert abs(res(M) - res(M2)) < 1e-12 and np.abs(M - M2).max() > 0.1


def _small_pair():
    src, _, tgt, _, _ = K.lidar()
    s, t = K.crop_to_keypoints(src, 40), K.crop_to_keypoints(tgt, 60)
    skp, tkp = R.voxel_keypoints(s), R.voxel_keypoints(t)
    assert (len(skp), len(tkp)) == (40, 60)
    return skp, R.features(skp)["fpfh"], tkp, R.features(tkp)["fpfh"]


def test_sampling_distance_is_halved_only_when_the_cloud_is_too_small_for_it():
    skp, sf, tkp, tf = _small_pair()
    extent = float(np.linalg.norm(skp.max(axis=0) - skp.min(axis=0)))
    assert extent < 100.0
    far, near = {}, {}
    R.sac_ia(skp, sf, tkp, tf, stats=far, max_iterations=20, min_sample_distance=100.0, nr_samples=6)
    R.sac_ia(skp, sf, tkp, tf, stats=near, max_iterations=20, min_sample_distance=0.0, nr_samples=6)
    nv = int((~np.isnan(sf[:, 0])).sum())
    # 100 halves to below the extent in ceil(log2(100 / extent)) steps at the least, each after 3 nv failed draws in a row
    steps = int(np.ceil(np.log2(100.0 / extent)))
    assert far["halvings"] >= 20 * steps and far["draws"] >= 20 * steps * 3 * nv
    assert near["halvings"] == 0 and near["draws"] < 20 * 6 * 2
    for st in (far, near):
        assert len(st["samples"]) == 20
        for smp, tj in st["samples"]:
            assert len(set(smp)) == 6 and len(tj) == 6 and min(tj) >= 0
    # the samples of the halved run are spread out: further apart than a run that asks for nothing
    spread = lambda st: np.mean([np.min([np.linalg.norm(skp[a] - skp[b]) for a in smp for b in smp if a != b]) for smp, _ in st["samples"]])
    assert spread(far) > 1.5 * spread(near)


def _loop_knn(sf, tf, k):
    """the feature k-NN by the definition: f32 distances summed over the bins in order, sorted by (distance, index)"""
    out = np.full((len(sf), k), -1, np.int32)
    for i in range(len(sf)):
        if np.isnan(sf[i, 0]):
            continue
        cand = []
        for j in range(len(tf)):
            if np.isnan(tf[j, 0]):
                continue
            d = np.float32(0)
            for b in range(33):
                df = np.float32(sf[i, b] - tf[j, b])
                d = np.float32(d + np.float32(df * df))
            cand.append((float(d), j))
        cand.sort()
        for r, (_, j) in enumerate(cand[:k]):
            out[i, r] = j
    return out


@pytest.mark.parametrize("nt,k", [(1, 1), (5, 10), (12, 10), (70, 16), (0, 3)])
def test_feature_knn_with_few_targets_ties_and_rows_without_a_feature(nt, k):
    rng = np.random.default_rng(nt + k)
    sf = rng.uniform(0, 30, size=(23, 33)).astype(np.float32)
    tf = rng.uniform(0, 30, size=(nt, 33)).astype(np.float32)
    if nt >= 5:
        tf[nt // 2:] = tf[:nt - nt // 2]  # every row twice: exact ties, in every list
        tf[1] = np.nan
        tf[-1] = np.nan
    sf[[3, 22]] = np.nan
    got = R.feature_knn(sf, tf, k)
    assert np.array_equal(got, _loop_knn(sf, tf, k))
    valid_t = int((~np.isnan(tf[:, 0])).sum()) if nt else 0
    assert (got[[3, 22]] == -1).all() and (got[:, min(k, valid_t):] == -1).all()
    if nt >= 5:
        rows = np.delete(got, [3, 22], axis=0)
        assert (rows[:, :min(k, valid_t)] >= 0).all()
        # a row and its copy come out together, lower index first, wherever both are listed
        half = nt - nt // 2
        for row in rows:
            lst = row[row >= 0].tolist()
            for a in lst:
                if a + (nt // 2) in lst and a < nt // 2 and a + nt // 2 < nt:
                    assert lst.index(a) + 1 == lst.index(a + nt // 2)
        assert half > 0


def test_tie_patches_give_twin_feature_rows_and_tied_distances():
    tgt, m = K.tie_patches(seed=0, copies=2)
    src, _ = K.tie_patches(seed=1, copies=1)
    vk, fk = K.ref_args(K.TIE_PARAMS)
    tkp, skp = R.voxel_keypoints(tgt, **vk), R.voxel_keypoints(src, **vk)
    assert len(tkp) == 2 * m and len(skp) == m and np.array_equal(tkp[:m], tkp[m:] - np.float32([0, 0, 8]))
    tf, sf = R.features(tkp, **fk)["fpfh"], R.features(skp, **fk)["fpfh"]
    assert not np.isnan(tf).any() and (tf[:m].view(np.uint32) == tf[m:].view(np.uint32)).all(axis=1).mean() > 0.9
    knn = R.feature_knn(sf, tf, 10)
    assert (knn[:, 1::2] == knn[:, 0::2] + m).mean() > 0.9  # twins side by side, the lower index first
    assert len(np.unique(tf[:m], axis=0)) > 0.9 * m  # (and not because all rows are alike)


def test_case_clouds_reach_what_they_were_built_for():
    # sizes asked for, to the keypoint
    src = K.lidar()[0]
    for want, iso in ((1, 0), (5, 0), (63, 0), (64, 2), (65, 0), (129, 3), (255, 0), (256, 0), (257, 2)):
        c = K.crop_to_keypoints(src, want, n_isolated=iso)
        kp = R.voxel_keypoints(c)
        assert len(kp) == want
        if want > 1:
            f = R.features(kp)
            assert int(np.isnan(f["fpfh"][:, 0]).sum()) == iso  # a dense crop: every keypoint but the isolated ones has a feature
    # the box filter can empty a cloud; the restatement answers with empty outputs
    e = K.emptied(src)
    assert len(R.voxel_keypoints(e)) == 0 and len(R.features(R.voxel_keypoints(e))["fpfh"]) == 0
    # 5000 points in one voxel
    cloud = K.one_voxel_cloud()
    inv = np.float32(1) / np.float32(0.4)
    assert ((np.floor(cloud * inv) == 0).all(axis=1)).sum() == 5000 and (np.floor(cloud.min(axis=0) * inv) < 0).all()
    # 1, 2, 3 and 4 neighbours
    c = K.neighbour_count_cloud()
    f = R.features(R.voxel_keypoints(c, leaf=0.1), 1.0, 1.0)
    cnt = np.diff(f["off"])
    assert sorted(cnt.tolist()) == [1, 2, 2, 3, 3, 3, 4, 4, 4, 4] and np.array_equal(np.isnan(f["normals"][:, 0]), cnt < 3)
    # planar and collinear neighbourhoods: gaps far from / exactly at zero
    f = R.features(R.voxel_keypoints(K.plane(0.125), leaf=0.25), 1.0, 1.0)
    assert (f["gap"] > 1e-2).all() and np.abs(np.abs(f["normals"]) - [0, 0, 1]).max() < 1e-12
    f = R.features(R.voxel_keypoints(K.diagonal_line(), leaf=0.25), 1.5, 1.5)
    assert (np.diff(f["off"]) >= 3).all() and (f["gap"] <= K.SMALL_GAP).all()


def test_denormal_pair_cloud_has_two_keypoints_a_denormal_distance_apart():
    cloud, (a, b) = K.denormal_pair_cloud()
    kp = R.voxel_keypoints(cloud, leaf=0.05)
    ja, jb = (int(np.flatnonzero((kp == cloud[i]).all(axis=1))[0]) for i in (a, b))
    d2 = R.d2_f32(kp[ja], kp[jb])
    assert ja != jb and 0 < d2 < np.finfo(np.float32).tiny
    f = R.features(kp, 1.0, 1.0)
    assert f["idx"][f["off"][ja] + 1] == jb and f["idx"][f["off"][jb] + 1] == ja
    assert np.isfinite(f["fpfh"][[ja, jb]]).all() and K.small_gap_share(f) <= K.SMALL_GAP_CAP


def test_hub_cloud_has_neighbours_without_a_normal_and_a_row_without_a_pair():
    cloud, r, who = K.hub_cloud()
    kp = R.voxel_keypoints(cloud, leaf=0.05)
    f = R.features(kp, r, r)
    ok = ~np.isnan(f["normals"][:, 0])
    find = lambda i: int(np.argmin(((kp.astype(np.float64) - cloud[i]) ** 2).sum(axis=1)))
    lst = lambda j: f["idx"][f["off"][j]:f["off"][j + 1]]
    hub = find(who["hub"][0])
    assert ok[hub] and len(lst(hub)) == 7 and not ok[[j for j in lst(hub) if j != hub]].any()
    assert (f["fpfh"][hub] == 0).all()  # no valid pair: nothing summed, thirds of sum 0 left unscaled
    for i in who["t2"]:
        j = find(i)
        assert ok[j] and sorted(ok[[q for q in lst(j) if q != j]].tolist()) == [False, True]
        assert np.isfinite(f["fpfh"][j]).all() and abs(f["fpfh"][j].sum() - 300.0) < 1e-3
    assert K.small_gap_share(f) <= K.SMALL_GAP_CAP


@pytest.mark.parametrize("leaf,nr,fr,which,cap", [(0.4, 0.3, 0.3, 0, K.SMALL_GAP_CAP), (1.0, 3.0, 3.0, 0, 0.0), (2.5, 6.0, 6.0, 0, 0.0),
                                                 (2.5, 6.0, 6.0, 2, 0.0), (0.4, 3.0, 1.5, 2, 0.001)])
def test_share_of_normals_left_out_of_the_angle_check_is_under_the_cap(leaf, nr, fr, which, cap):
    cloud = K.lidar()[which]
    f = R.features(R.voxel_keypoints(cloud, leaf=leaf), nr, fr)
    share = K.small_gap_share(f)
    assert share <= cap, share
    if leaf == 0.4 and nr == 0.3:  # the sparsest case: few keypoints have a normal at all, and the cap still holds
        assert 0.0 < share and (~np.isnan(f["normals"][:, 0])).mean() < 0.1
