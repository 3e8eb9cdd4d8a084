"""GPU tests of the bootstrap (sicp_bootstrap*) away from its defaults, against the numpy restatement
tests/bootstrap_ref.py: other leaves, radii, box limits, seeds, sample and neighbour counts; clouds translated, cropped to
chosen keypoint counts, poisoned with non-finite points, labelled on EM / SEMANTIC handles; and the edges of each kernel --
pairs exactly on the radius, 1 .. 4 neighbours, planar and collinear neighbourhoods, neighbours without a normal, feature
rows without a valid pair, exact feature-distance ties, fewer target features than k, the halved sampling distance.
Every case asserts on the CPU (restatement only) that it reaches the branch it was built for.  The inputs come from
tests/bootstrap_cases.py; the acceptance rules are those of tests/test_gpu_bootstrap.py."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import bootstrap_cases as K
import bootstrap_ref as R
from test_gpu_validation import poison

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")


def _mat(qt):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    return T


def _filler():
    """a small ordinary cloud for the side of a handle a case does not look at"""
    return K.compact(K.lidar()[2], 2000)


def _engine(src, tgt=None, mode=sicp.MODE_GICP, labels=(None, None), cm=None):
    p = sicp.default_params(mode)
    if cm is not None:
        p.num_classes = len(cm)
    e = sicp.Engine(0, p)
    if cm is not None:
        e.set_confusion(cm)
    e.set_source(src, *([labels[0]] if labels[0] is not None else []))
    e.set_target(_filler() if tgt is None else tgt, *([labels[1]] if labels[1] is not None else []))
    return e


def _check_cloud(e, which, cloud, params, degenerate=False, orientation=True, keypoints_only=False):
    """parts 1 - 4 for one cloud of a handle: keypoints bit-equal, lists equal, normals (angle below 1e-9 where the
    restatement's eigenvalue gap exceeds 1e-6, same NaN pattern, same orientation), FPFH from the GPU's own normals.
    `degenerate`: the case is built from neighbourhoods without a unique normal, so the cap on rows left out of the angle
    check does not apply; `orientation=False`: (-p) . n is 0 by construction, the flip rule decides nothing."""
    vk, fk = K.ref_args(params)
    xyz, nrm, f, off, idx = e.bootstrap_keypoints(which, sicp.default_bootstrap_params(**params))
    kp = R.voxel_keypoints(cloud, **vk)
    assert xyz.shape == kp.shape and np.array_equal(xyz.view(np.uint32), kp.view(np.uint32))
    if keypoints_only:
        return dict(kp=kp, xyz=xyz)
    ref = R.features(kp, **fk)
    assert np.array_equal(off, ref["off"]) and np.array_equal(idx, ref["idx"])
    ok = ~np.isnan(ref["normals"][:, 0])
    assert np.array_equal(np.isnan(nrm), np.isnan(ref["normals"]))
    if fk["normal_radius"] == fk["feature_radius"]:
        assert np.array_equal(ok, np.diff(off) >= 3)
    if ok.any():
        assert np.abs(np.linalg.norm(nrm[ok], axis=1) - 1.0).max() < 1e-9
    sel = ok & (ref["gap"] > K.SMALL_GAP)
    if not degenerate:
        assert K.small_gap_share(ref) <= K.SMALL_GAP_CAP, K.small_gap_share(ref)
    if sel.any():
        a, b = nrm[sel], ref["normals"][sel]
        ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum("ij,ij->i", a, b)))
        assert ang.max() < 1e-9, ang.max()
        if orientation:
            assert (np.einsum("ij,ij->i", a, b) > 0).all()
    # FPFH on the GPU's own normals (tests/test_gpu_bootstrap.py); the NaN pattern is exact: whole rows or nothing
    rf = R.fpfh(kp, nrm, off, idx, ref["d2"])
    assert np.array_equal(np.isnan(f), np.isnan(rf))
    assert np.array_equal(np.isnan(f[:, 0]), ~ok)
    assert not np.isnan(f[ok]).any() and not np.isnan(rf[ok]).any()
    if ok.any():
        g, r = f[ok].astype(np.float64), rf[ok].astype(np.float64)
        bad = ~np.isclose(g, r, rtol=1e-6, atol=1e-6)
        close = ~bad.any(axis=1)
        assert close.mean() >= 0.999, close.mean()
        for t in range(3):
            assert (bad[:, 11 * t:11 * t + 11].sum(axis=1) <= 2).all()
    return dict(kp=kp, ref=ref, xyz=xyz, nrm=nrm, f=f, off=off, idx=idx, ok=ok)


def _check_one(cloud, params, **kw):
    with _engine(cloud) as e:
        return _check_cloud(e, sicp.SOURCE, cloud, params, **kw)


# ---- parts 1 - 4 over parameters ------------------------------------------------------------------------------------------
# (leaf, normal radius, feature radius) on the 20 000-point LIDAR pair; leaf 0.4 with both radii 3 is
# tests/test_gpu_bootstrap.py.  Radii follow the leaf where the default 3 would make lists of thousands or of nothing;
# the small-gap share of each was computed beforehand from the restatement (at most 0.3 %; _check_cloud asserts the cap).
LIDAR_SETS = [(0.1, 0.5, 0.5), (0.25, 1.5, 1.5), (0.4, 1.5, 3.0), (0.4, 3.0, 1.5), (1.0, 3.0, 3.0), (2.5, 6.0, 6.0)]


@pytest.mark.parametrize("leaf,nr,fr", LIDAR_SETS)
def test_lidar_pair_over_leaves_and_radii(leaf, nr, fr):
    src, _, tgt, _, _ = K.lidar()
    P = dict(leaf_size=leaf, normal_radius=nr, feature_radius=fr)
    with _engine(src, tgt) as e:
        out = _check_cloud(e, sicp.SOURCE, src, P)
        assert len(out["kp"]) > 200 and out["ok"].mean() > 0.9
        # (the restatement's lists of the two finest grids cost a second per cloud: the target's keypoints only there)
        _check_cloud(e, sicp.TARGET, tgt, P, keypoints_only=leaf < 0.4)


def test_radius_below_the_leaf_gives_lists_of_the_point_alone():
    # (the target cloud of this pair has 2.3 % small-gap rows at these radii, above the cap: the source, 1.2 %, is the case)
    src = K.lidar()[0]
    out = _check_one(src, dict(leaf_size=0.4, normal_radius=0.3, feature_radius=0.3))
    cnt = np.diff(out["off"])
    assert (cnt == 1).mean() > 0.5 and 0.02 < out["ok"].mean() < 0.2


def test_radius_of_ten_gives_lists_of_hundreds():
    src = K.lidar_sub(5000)[0]
    out = _check_one(src, dict(leaf_size=0.8, normal_radius=10.0, feature_radius=10.0))
    longest = np.diff(out["off"]).max()
    assert longest > 320 and longest % 64 != 0  # (several 64-lane passes and a ragged remainder)


@pytest.mark.parametrize("leaf,r", [(0.02, 0.1), (0.05, 0.15), (0.1, 0.5)])
def test_rgbd_frame_at_metre_scale(leaf, r):
    src = K.rgbd()[0]
    out = _check_one(src, dict(leaf_size=leaf, normal_radius=r, feature_radius=r, box_max=35.0))
    assert len(out["kp"]) > 4000


@pytest.mark.parametrize("shift,box", [((-20.0, 15.0, -3.0), 35.0), ((1000.0, -1000.0, 0.0), 1e4)])
def test_translated_cloud_negative_grid_origin_and_coarse_f32_spacing(shift, box):
    src = K.lidar()[0] + np.float32(shift)
    out = _check_one(src, dict(box_max=box))
    inv = np.float32(1) / np.float32(0.4)
    assert (np.floor(src.min(axis=0) * inv) < 0).any()  # a negative min_b
    assert len(out["kp"]) > 2500


@pytest.mark.parametrize("box", [20.0, 5.0])
def test_box_limit_cuts_through_the_cloud(box):
    src = K.lidar()[0]
    out = _check_one(src, dict(box_max=box))
    assert 500 < len(out["kp"]) < len(R.voxel_keypoints(src)) - 100


def test_point_exactly_on_the_box_limit_is_dropped():
    src = K.lidar()[0].copy()
    at = [1000, 1001, 1002]  # one point per axis
    for axis, i in enumerate(at):
        src[i, axis] = 35.0
    kp = R.voxel_keypoints(src)
    # the restatement drops them (the keypoints of the cloud without them) and would not if one were a hair inside
    assert np.array_equal(kp, R.voxel_keypoints(np.delete(src, at, axis=0)))
    for axis, i in enumerate(at):
        inside = src.copy()
        inside[i, axis] = np.nextafter(np.float32(35.0), np.float32(0))
        assert not np.array_equal(kp, R.voxel_keypoints(inside))
    _check_one(src, {})


def test_cloud_the_box_filter_empties():
    src = K.emptied(K.lidar()[0])  # one coordinate beyond the box is enough
    assert len(R.voxel_keypoints(src)) == 0 and (src[:, 1:] < 35).all(axis=1).any()
    with _engine(src) as e:
        xyz, nrm, f, off, idx = e.bootstrap_keypoints(sicp.SOURCE)
        assert len(xyz) == 0 and len(idx) == 0 and off[0] == 0
        with pytest.raises(sicp.SicpError) as ex:
            e.bootstrap()
        assert ex.value.status == sicp.ERR_TOO_FEW_POINTS


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_clouds_around_one_workgroup(n):
    cloud = K.compact(K.lidar()[0], n)
    assert len(cloud) == n
    _check_one(cloud, dict(leaf_size=0.1, normal_radius=1.0, feature_radius=1.0))


def test_cloud_of_100003_points():
    src = K.lidar(100003)[0]
    assert len(src) == 100003
    _check_one(src, {})


def test_thousands_of_points_in_one_voxel():
    cloud = K.one_voxel_cloud()
    inv = np.float32(1) / np.float32(0.4)
    assert ((np.floor(cloud * inv) == 0).all(axis=1)).sum() == 5000
    # sparse by construction (100 scattered points): the share of small gaps is not what this case is about
    _check_one(cloud, {}, degenerate=True)


def test_non_finite_points_are_left_out():
    src, _, tgt, _, _ = K.lidar()
    rng = np.random.default_rng(5)
    ps, ks = poison(src, rng)
    pt, kt = poison(tgt, rng)
    assert (~ks).sum() >= 0.03 * len(src) - 1 and (~kt).sum() >= 0.03 * len(tgt) - 1
    with _engine(ps, pt) as e:
        a = _check_cloud(e, sicp.SOURCE, ps, {})
        b = _check_cloud(e, sicp.TARGET, pt, {})
    # (the restatement drops the same rows: the keypoints of the finite points alone)
    assert np.array_equal(a["kp"], R.voxel_keypoints(src[ks])) and np.array_equal(b["kp"], R.voxel_keypoints(tgt[kt]))


def test_labelled_cloud_gives_the_same_bytes_in_every_mode():
    src, sl, tgt, tl, cm = K.lidar()
    assert len(np.unique(sl)) > 3
    outs = []
    for mode in (sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC):
        with _engine(src, tgt, mode, (sl, tl), cm) as e:
            o = [e.bootstrap_keypoints(w) for w in (sicp.SOURCE, sicp.TARGET)]
            if mode == sicp.MODE_EM:
                _check_cloud(e, sicp.SOURCE, src, {})
            outs.append(o)
    for o in outs[1:]:
        for w in range(2):
            for x, y in zip(o[w], outs[0][w]):
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


# ---- part 2: pairs exactly on the radius ----------------------------------------------------------------------------------
@pytest.mark.parametrize("r,pairs", list(zip(K.LATTICE_RADII, (3510, 6048, 2964))))
def test_lattice_pairs_exactly_on_the_radius_are_outside(r, pairs):
    lat = K.lattice(K.LATTICE_S)
    assert K.boundary_pairs(lat, r) == pairs  # ordered pairs with d^2 == f32(r * r): `<=` would list them
    # a cubic lattice: neighbourhoods of equal eigenvalues by construction
    out = _check_one(lat, K.LATTICE_PARAMS(r), degenerate=True)
    assert np.array_equal(out["xyz"].view(np.uint32), lat.view(np.uint32))  # the keypoints are the lattice itself
    assert len(out["idx"]) == len(R.radius_lists(lat, r)[1])


# ---- part 3: normals ------------------------------------------------------------------------------------------------------
def test_one_to_four_neighbours():
    cloud = K.neighbour_count_cloud()
    out = _check_one(cloud, dict(leaf_size=0.1, normal_radius=1.0, feature_radius=1.0), degenerate=True)
    cnt = np.diff(out["off"])
    assert sorted(cnt.tolist()) == [1, 2, 2, 3, 3, 3, 4, 4, 4, 4]
    assert np.array_equal(np.isnan(out["nrm"][:, 0]), cnt < 3)
    assert (out["ref"]["gap"][cnt >= 3] > 1e-3).all()  # (triangles and a tetrahedron: every normal is compared)


def test_exactly_planar_lattice():
    cloud = K.plane(0.125)
    out = _check_one(cloud, dict(leaf_size=0.25, normal_radius=1.0, feature_radius=1.0))
    assert out["ok"].all() and (out["ref"]["gap"] > 1e-2).all()
    # (0, 0, +-1), and towards the origin: -p . n = -0.125 nz >= 0
    assert np.abs(out["nrm"] - [0.0, 0.0, -1.0]).max() < 1e-12
    assert np.abs(out["ref"]["normals"] - [0.0, 0.0, -1.0]).max() < 1e-12


def test_plane_through_the_origin_keeps_the_unflipped_eigenvector():
    cloud = K.plane(0.0)
    assert (cloud[:, 2] == 0).all()
    out = _check_one(cloud, dict(leaf_size=0.25, normal_radius=1.0, feature_radius=1.0), orientation=False)
    n = out["nrm"]
    assert out["ok"].all() and np.abs(np.abs(n) - [0.0, 0.0, 1.0]).max() < 1e-12
    # (-p) . n is +-0 for every point: `< 0` flips nothing, so every point keeps its solver's eigenvector, and one solver
    # gives every point the same one (the restatement's LAPACK and the engine's Jacobi may differ in that sign)
    assert (np.einsum("ij,ij->i", -out["kp"].astype(np.float64), n) == 0).all()
    assert len(np.unique(np.sign(n[:, 2]))) == 1 and len(np.unique(np.sign(out["ref"]["normals"][:, 2]))) == 1
    # the engine's cyclic Jacobi starts from the identity and rotates nothing in a block that is already diagonal: +z
    assert (n[:, 2] > 0).all()


def test_collinear_neighbourhoods_give_a_unit_vector_across_the_line():
    cloud = K.diagonal_line()
    out = _check_one(cloud, dict(leaf_size=0.25, normal_radius=1.5, feature_radius=1.5), degenerate=True)
    assert out["ok"].all() and (out["ref"]["gap"] <= K.SMALL_GAP).all()  # gap 0: none of them is in the angle check
    n = out["nrm"]
    d = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() < 1e-9 and np.abs(n @ d).max() < 1e-9
    assert (np.einsum("ij,ij->i", -out["kp"].astype(np.float64), n) >= 0).all()


# ---- part 4: neighbours without a normal, rows without a valid pair -----------------------------------------------------
def test_neighbours_without_a_normal_and_a_keypoint_without_a_valid_pair():
    cloud, r, who = K.hub_cloud()
    out = _check_one(cloud, dict(leaf_size=0.05, normal_radius=r, feature_radius=r))
    kp, ok, off, idx = out["kp"], out["ok"], out["off"], out["idx"]

    def find(i):
        d = ((kp.astype(np.float64) - cloud[i]) ** 2).sum(axis=1)
        j = int(np.argmin(d))
        assert d[j] < 1e-10
        return j

    hub = find(who["hub"][0])
    lst = lambda j: idx[off[j]:off[j + 1]]
    # the hub: a normal, six neighbours, none of them with one -> no pair, nothing to sum: an all-zero row (s == 0)
    assert ok[hub] and len(lst(hub)) == 7 and not ok[[j for j in lst(hub) if j != hub]].any()
    assert (out["f"][hub] == 0).all()
    for i in who["spokes"] + who["t3"]:
        assert not ok[find(i)] and np.isnan(out["f"][find(i)]).all()
    for i in who["t2"]:  # a neighbour with a normal and one without in one list
        j = find(i)
        others = [q for q in lst(j) if q != j]
        assert ok[j] and sorted(ok[others].tolist()) == [False, True]
        assert np.isfinite(out["f"][j]).all() and out["f"][j].sum() > 0


def test_two_keypoints_a_denormal_distance_apart():
    cloud, (a, b) = K.denormal_pair_cloud()
    out = _check_one(cloud, dict(leaf_size=0.05, normal_radius=1.0, feature_radius=1.0))
    kp, off, idx = out["kp"], out["off"], out["idx"]
    ja, jb = (int(np.flatnonzero((kp == cloud[i]).all(axis=1))[0]) for i in (a, b))
    d2 = R.d2_f32(kp[ja], kp[jb])
    assert ja != jb and 0 < d2 < np.finfo(np.float32).tiny  # two keypoints, a denormal d^2: not 0, and not flushed to it
    # each is the other's nearest neighbour after itself, and (1 / d^2 outweighs the rest by 1e40) has its SPFH as its FPFH
    assert idx[off[ja]] == ja and idx[off[ja] + 1] == jb and idx[off[jb]] == jb and idx[off[jb] + 1] == ja
    assert out["ok"][[ja, jb]].all() and np.isfinite(out["f"][[ja, jb]]).all()
    assert np.abs(out["f"][ja].reshape(3, 11).sum(axis=1) - 100.0).max() < 1e-3


# ---- part 5: the feature k-NN -------------------------------------------------------------------------------------------
def _knn_case(src, tgt, params, k):
    p = sicp.default_bootstrap_params(k_correspondences=k, **params)
    with _engine(src, tgt) as e:
        skp, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE, p)
        tkp, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET, p)
        _, _, knn = e.bootstrap_score(np.zeros((0, p.nr_samples), np.int32), np.zeros((0, p.nr_samples), np.int32), p,
                                      n_source_keypoints=len(skp))
    want = R.feature_knn(sf, tf, k)
    assert knn.shape == want.shape == (len(skp), k)
    assert np.array_equal(knn, want)
    return skp, sf, tkp, tf, knn


# (ns, nt, k, keypoints without a feature on each side): nt around the 64-row tile, ns around the 256-thread workgroup
KNN_CASES = [(255, 63, 10, 0), (256, 64, 1, 0), (257, 65, 16, 2), (257, 129, 10, 3), (300, 1, 10, 0), (200, 5, 10, 0),
             (1, 64, 10, 0), (256, 129, 16, 0)]


@pytest.mark.parametrize("ns,nt,k,iso", KNN_CASES)
def test_feature_knn_at_chosen_keypoint_counts(ns, nt, k, iso):
    src, _, tgt, _, _ = K.lidar()
    s = K.crop_to_keypoints(src, ns, n_isolated=min(iso, max(ns - 1, 0)))
    t = K.crop_to_keypoints(tgt, nt, n_isolated=min(iso, max(nt - 1, 0)))
    skp, sf, tkp, tf, knn = _knn_case(s, t, {}, k)
    assert (len(skp), len(tkp)) == (ns, nt)
    sv, tv = ~np.isnan(sf[:, 0]), ~np.isnan(tf[:, 0])
    if iso:  # keypoints without a feature on both sides
        assert (~sv).sum() >= iso and (~tv).sum() >= iso
        assert (knn[~sv] == -1).all() and not np.isin(knn, np.flatnonzero(~tv)).any()
    if nt == 1 or ns == 1:  # a lone keypoint has no feature: nothing to match
        assert (knn == -1).all()
    else:
        k_eff = min(k, int(tv.sum()))
        assert sv.any() and (knn[sv][:, :k_eff] >= 0).all() and (knn[:, k_eff:] == -1).all()
        if nt == 5:
            assert k_eff < k  # the -1 padding


@pytest.mark.parametrize("k", [1, 2, 10, 16])
def test_feature_knn_ties_go_to_the_lower_index(k):
    """Exact ties produced through clouds: the target is two copies of one patch, a keypoint and its twin have the same
    feature row bit for bit, so every source feature is exactly as far from both."""
    tgt, m = K.tie_patches(seed=0, copies=2)
    src, _ = K.tie_patches(seed=1, copies=1)
    skp, sf, tkp, tf, knn = _knn_case(src, tgt, K.TIE_PARAMS, k)
    assert len(tkp) == 2 * m and np.array_equal(tkp[:m], tkp[m:] - np.float32([0, 0, 8]))
    twins = (tf[:m].view(np.uint32) == tf[m:].view(np.uint32)).all(axis=1) & ~np.isnan(tf[:m, 0])
    assert twins.mean() > 0.9, twins.mean()
    # the restatement's f32 distances of the GPU's features: a tie between ranks k - 1 and k decides who is listed, a tie
    # inside the first k their order
    d = np.zeros((len(sf), len(tf)), np.float32)
    for b in range(33):
        df = sf[:, b:b + 1] - tf[None, :, b]
        d = d + df * df
    ds = np.sort(d, axis=1)[:, :k + 1]
    tied = (ds[:, 1:] == ds[:, :-1]).any(axis=1)
    assert tied.mean() > 0.9, tied.mean()
    if k >= 2:  # a twin pair listed together is listed lower index first
        first = knn[:, 0]
        pair = (knn[:, 1] == first + m) & twins[np.minimum(first, m - 1)]
        assert pair.mean() > 0.5, pair.mean()
    else:
        assert (knn[:, 0] < m)[twins[knn[:, 0] % m]].all()


@pytest.mark.parametrize("nr", [3, 4, 8])
def test_hypotheses_of_more_than_three_pairs(nr):
    src, _, tgt, _, _ = K.lidar_sub(8000)
    p = sicp.default_bootstrap_params(nr_samples=nr)
    with _engine(src, tgt) as e:
        skp = e.bootstrap_keypoints(sicp.SOURCE, p)[0]
        tkp = e.bootstrap_keypoints(sicp.TARGET, p)[0]
        rng = np.random.default_rng(nr)
        a = np.stack([rng.choice(len(skp), nr, replace=False) for _ in range(48)])
        b = np.stack([rng.choice(len(tkp), nr, replace=False) for _ in range(48)])
        M, err, _ = e.bootstrap_score(a, b, p)
    tree = R.cKDTree(tkp.astype(np.float64))
    for i in range(len(a)):
        Mr = R.umeyama(skp[a[i]], tkp[b[i]])
        assert np.abs(M[i] - Mr).max() < 1e-9, (i, np.abs(M[i] - Mr).max())
        er = R.truncated_error(M[i], skp, tree, tkp, p.max_corr_distance)
        assert abs(err[i] - er) <= 1e-9 * max(1.0, abs(er))


# ---- part 6: the whole SAC-IA -------------------------------------------------------------------------------------------
def _check_sac(src, tgt, **kw):
    """Engine.bootstrap against R.sac_ia on the GPU's own keypoints and features: the three assertions of
    tests/test_gpu_bootstrap.py.  They presuppose that every hypothesis has one optimal transform: a sample whose pairs
    leave a rotation free (R.fit_rank_ratio) has many, Horn's method and the SVD return different ones, and so may any
    two correct solvers.  Every case here is chosen to have no such iteration, and says so.  Returns what the
    restatement's run went through."""
    p = sicp.default_bootstrap_params(**kw)
    with _engine(src, tgt) as e:
        skp, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE, p)
        tkp, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET, p)
        qt, info = e.bootstrap(p)
    assert info["n_source_keypoints"] == len(skp) and info["n_target_keypoints"] == len(tkp)
    stats = {}
    best, err, errs, Ms = R.sac_ia(skp, sf, tkp, tf, stats=stats, **kw)
    assert stats["ambiguous"] == [], stats["ambiguous"]
    gb = info["best_iteration"]
    assert 0 <= gb < len(errs)
    assert gb == best or abs(errs[gb] - err) <= 1e-9 * max(1.0, err)
    assert abs(info["best_error"] - errs[gb]) <= 1e-9 * max(1.0, errs[gb])
    assert np.abs(_mat(qt)[:3] - Ms[gb]).max() < 1e-9
    stats.update(n_valid_target=int((~np.isnan(tf[:, 0])).sum()), n_valid_source=int((~np.isnan(sf[:, 0])).sum()))
    return stats


SAC_SETS = [dict(seed=1), dict(seed=2), dict(seed=12345), dict(nr_samples=5), dict(k_correspondences=1),
            dict(k_correspondences=16), dict(max_iterations=1)]


@pytest.mark.parametrize("kw", SAC_SETS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_sac_ia_over_seeds_samples_and_neighbours(kw):
    src, _, tgt, _, _ = K.lidar_sub(8000)
    stats = _check_sac(src, tgt, **dict(dict(max_iterations=60), **kw))
    assert stats["halvings"] == 0 and stats["k_eff"] == kw.get("k_correspondences", 10)


def test_sac_ia_halves_the_sampling_distance_on_a_small_cloud():
    src, _, tgt, _, _ = K.lidar()
    s, t = K.crop_to_keypoints(src, 40), K.crop_to_keypoints(tgt, 60)
    kp = R.voxel_keypoints(s)
    extent = np.linalg.norm(kp.max(axis=0) - kp.min(axis=0))
    assert extent < 100.0
    # (six samples: with three or four, several iterations of this pair draw pairs that leave a rotation free)
    stats = _check_sac(s, t, min_sample_distance=100.0, max_iterations=50, nr_samples=6)
    assert stats["halvings"] >= 50  # (every iteration starts again from the full distance)


def test_sac_ia_with_fewer_target_features_than_k():
    src, _, tgt, _, _ = K.lidar()
    s, t = K.crop_to_keypoints(src, 80), K.crop_to_keypoints(tgt, 7, n_isolated=1)
    # (eight samples: three drawn from six target keypoints name one of them twice in almost every second iteration, and
    # two distinct target points fix no rotation)
    stats = _check_sac(s, t, max_iterations=50, nr_samples=8)
    assert stats["n_valid_target"] == 6 and stats["k_eff"] == 6 < 10


# ---- part 7: batches ----------------------------------------------------------------------------------------------------
INFO_KEYS = ("n_source_keypoints", "n_target_keypoints", "max_neighbours", "best_iteration")


@pytest.mark.parametrize("kw", [dict(max_iterations=60),
                                dict(max_iterations=60, leaf_size=0.25, normal_radius=1.5, feature_radius=3.0, box_max=20.0,
                                     nr_samples=4, k_correspondences=16, seed=2)], ids=["defaults", "other-parameters"])
def test_batch_over_a_mix_of_edge_cases_equals_the_lone_calls(kw):
    p = sicp.default_bootstrap_params(**kw)
    src, sl, tgt, tl, cm = K.lidar_sub(8000)
    rng = np.random.default_rng(7)
    emptied = K.emptied(src)
    es = [_engine(src, tgt),
          _engine(K.compact(src, 257), tgt),
          _engine(emptied, tgt),
          _engine(poison(src, rng)[0], poison(tgt, rng)[0]),
          _engine(src, tgt, sicp.MODE_EM, (sl, tl), cm),
          _engine(K.lidar()[0], emptied),
          _engine(src, tgt, sicp.MODE_SEMANTIC, (sl, tl), cm)]
    try:
        lone = []
        for e in es:
            try:
                lone.append((sicp.OK,) + e.bootstrap(p))
            except sicp.SicpError as ex:
                lone.append((ex.status, None, None))
        assert [l[0] for l in lone] == [sicp.OK, sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK, sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK]
        res = sicp.bootstrap_batch(es, p)
        for (st, qt, info), (lst, lq, li) in zip(res, lone):
            assert st == lst
            if st != sicp.OK:
                assert qt is None
                continue
            assert np.array_equal(qt.view(np.uint64), lq.view(np.uint64))
            for key in INFO_KEYS:
                assert info[key] == li[key], key
            assert np.float64(info["best_error"]).view(np.uint64) == np.float64(li["best_error"]).view(np.uint64)
        # labels and mode change nothing: the EM and SEMANTIC handles hold the first pair's points
        for j in (4, 6):
            assert np.array_equal(res[j][1].view(np.uint64), res[0][1].view(np.uint64))
    finally:
        for e in es:
            e.close()
