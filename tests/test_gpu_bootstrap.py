"""GPU tests of the initial alignment without a pose prior (sicp_bootstrap, exec/bootstrap.h) against the numpy
restatement tests/bootstrap_ref.py: keypoints, neighbour lists, normals, FPFH, feature k-NN, hypothesis scores, the full
SAC-IA, the end-to-end use as align()'s initial pose, and the refusals."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import bootstrap_ref as R
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])


def _mat(qt):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    return T


def _delta(A, B):
    D = np.linalg.inv(A) @ B
    return np.degrees(np.linalg.norm(Rotation.from_matrix(D[:3, :3]).as_rotvec())), np.linalg.norm(D[:3, 3])


_pairs = {}


def _pair(n, motion=(1.0, 2.0)):
    key = (n, motion)
    if key not in _pairs:
        src, _, tgt, _, T, _ = synth.lidar_pair(seed=3, n_points=n, motion=motion)
        _pairs[key] = (src, tgt, T)
    return _pairs[key]


def _engine(src, tgt, mode=sicp.MODE_GICP):
    e = sicp.Engine(0, sicp.default_params(mode))
    e.set_source(src)
    e.set_target(tgt)
    return e


@pytest.mark.parametrize("n", [20000, 100000])
def test_keypoints_neighbours_normals_fpfh_match_the_restatement(n):
    src, tgt, _ = _pair(n)
    with _engine(src, tgt) as e:
        for which, cloud in ((sicp.SOURCE, src), (sicp.TARGET, tgt)):
            xyz, nrm, f, off, idx = e.bootstrap_keypoints(which)
            kp = R.voxel_keypoints(cloud)
            assert xyz.shape == kp.shape and np.array_equal(xyz.view(np.uint32), kp.view(np.uint32))
            ref = R.features(kp)
            assert np.array_equal(off, ref["off"]) and np.array_equal(idx, ref["idx"])
            ok = ~np.isnan(ref["normals"][:, 0])
            assert np.array_equal(ok, ~np.isnan(nrm[:, 0]))
            sel = ok & (ref["gap"] > 1e-6)
            a, b = nrm[sel], ref["normals"][sel]
            ang = np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum("ij,ij->i", a, b)))
            assert ang.max() < 1e-9, ang.max()
            assert np.array_equal(np.einsum("ij,ij->i", nrm[sel], ref["normals"][sel]) > 0, np.ones(sel.sum(), bool))
            assert np.array_equal(np.isnan(f[:, 0]), ~ok)
            # FPFH on the GPU's own normals: where a neighbourhood is a line (a pole), its normal is any vector of a plane
            # and the two eigensolvers pick different ones; the features must agree given the same normals
            rf = R.fpfh(kp, nrm, off, idx, ref["d2"])
            g, r = f[ok].astype(np.float64), rf[ok].astype(np.float64)
            close = np.isclose(g, r, rtol=1e-6, atol=1e-6).all(axis=1)
            assert close.mean() >= 0.999, close.mean()
            # a bin decision that flips (an angle on a bin edge) moves one pair's increment between two bins of a third
            bad = ~np.isclose(g, r, rtol=1e-6, atol=1e-6)
            for t in range(3):
                assert (bad[:, 11 * t:11 * t + 11].sum(axis=1) <= 2).all()


def test_feature_knn_and_triple_scores_match_the_restatement():
    src, tgt, _ = _pair(20000)
    p = sicp.default_bootstrap_params()
    with _engine(src, tgt) as e:
        skp, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE)
        tkp, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET)
        rng = np.random.default_rng(0)
        a = rng.integers(0, len(skp), size=(64, 3))
        b = rng.integers(0, len(tkp), size=(64, 3))
        M, err, knn = e.bootstrap_score(a, b, p, n_source_keypoints=len(skp))
    assert np.array_equal(knn, R.feature_knn(sf, tf, p.k_correspondences))
    tree = R.cKDTree(tkp.astype(np.float64))
    for i in range(len(a)):
        Mr = R.umeyama(skp[a[i]], tkp[b[i]])
        assert np.abs(M[i] - Mr).max() < 1e-9
        er = R.truncated_error(M[i], skp, tree, tkp, p.max_corr_distance)
        assert abs(err[i] - er) <= 1e-9 * max(1.0, abs(er))


def test_full_bootstrap_picks_the_restatements_best_iteration_and_is_reproducible():
    src, tgt, _ = _pair(20000)
    p = sicp.default_bootstrap_params()
    with _engine(src, tgt) as e:
        skp, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE)
        tkp, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET)
        qt1, info1 = e.bootstrap(p)
        qt2, info2 = e.bootstrap(p)
    assert np.array_equal(qt1, qt2) and info1["best_error"] == info2["best_error"]
    assert info1["n_source_keypoints"] == len(skp) and info1["n_target_keypoints"] == len(tkp)
    best, err, errs, Ms = R.sac_ia(skp, sf, tkp, tf)
    gb = info1["best_iteration"]
    assert gb == best or abs(errs[gb] - err) <= 1e-9 * max(1.0, err)
    assert abs(info1["best_error"] - errs[gb]) <= 1e-9 * max(1.0, errs[gb])
    assert np.abs(_mat(qt1)[:3] - Ms[gb]).max() < 1e-9


@pytest.mark.parametrize("yaw", [60.0, 120.0, 180.0])
def test_bootstrap_recovers_large_motions_where_identity_misses(yaw):
    src, tgt, T = _pair(20000, motion=(4.0, yaw))
    with _engine(src, tgt) as e:
        q0, _ = e.align(IDENT)
        assert _delta(T, _mat(q0))[0] > 10.0
        qb, info = e.bootstrap()
        rot, tr = _delta(T, _mat(qb))
        assert rot < 5.0 and tr < 1.0, (rot, tr, info)
        qa, _ = e.align(qb)
        from scipy.spatial.transform import Rotation as Rot
        qg = np.r_[Rot.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]]
        qr, _ = e.align(qg)
    rot, tr = _delta(_mat(qr), _mat(qa))
    assert np.radians(rot) < 1e-4 and tr < 1e-3


def test_refusals_leave_the_handle_as_it_was():
    src, tgt, _ = _pair(20000)
    with _engine(src, tgt) as e, _engine(src, tgt) as fresh:
        tiny = np.array([[0, 0, 0], [0.1, 0, 0], [40, 40, 40]], np.float32)
        with _engine(tiny, tgt) as t:
            with pytest.raises(sicp.SicpError) as ex:
                t.bootstrap()
            assert ex.value.status == sicp.ERR_TOO_FEW_POINTS
        with pytest.raises(sicp.SicpError) as ex:
            e.bootstrap(sicp.default_bootstrap_params(leaf_size=1e-4))
        assert ex.value.status == sicp.ERR_INVALID_ARGUMENT and "leaf size" in str(ex.value)
        for bad in (dict(nr_samples=2), dict(k_correspondences=0), dict(max_iterations=0), dict(feature_radius=-1.0)):
            with pytest.raises(sicp.SicpError) as ex:
                e.bootstrap(sicp.default_bootstrap_params(**bad))
            assert ex.value.status == sicp.ERR_INVALID_ARGUMENT
        qa, sa = e.align(IDENT)
        qf, sf = fresh.align(IDENT)
    assert np.array_equal(qa, qf) and sa["outer_iters"] == sf["outer_iters"]
