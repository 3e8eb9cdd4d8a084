"""GPU tests of sicp_pose_covariance: H, g and cost are sicp_accumulate's bits; the cross sums S_src / S_tgt match the numpy
restatement (tests/pose_cov_ref.py) on the engine's own correspondences, weights and normals in all three modes, and finite
differences on a small pair; the covariance is H^-1 S H^-1; results repeat bit for bit and a batch gives every pair its lone
call's bits; zero active slots give NaN and positive_definite = 0; bad sigmas and general-form covariances are refused; and
in a Monte Carlo run of GICP registrations the covariance at each estimate matches the spread (mean NEES in [1.5, 24])."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import lm_ref
import pose_cov_ref as ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
MODES = (sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC)


def _qt(T):
    return np.concatenate([Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]])


def _near(T, seed):
    """T moved by a small pose: the search then runs off the true pose"""
    rng = np.random.default_rng(seed)
    D = np.eye(4)
    D[:3, :3] = Rotation.from_rotvec(rng.normal(scale=0.004, size=3)).as_matrix()
    D[:3, 3] = rng.normal(scale=0.02, size=3)
    return T @ D


_pairs = {}


def _pair(n, seed):
    if (n, seed) not in _pairs:
        _pairs[(n, seed)] = synth.lidar_pair(seed=seed, n_points=n)
    return _pairs[(n, seed)]


def _engine(mode, n, seed):
    src, sl, tgt, tl, T, cm = _pair(n, seed)
    p = sicp.default_params(mode)
    p.num_classes = cm.shape[0]
    if mode == sicp.MODE_SEMANTIC:
        p.min_class_pts = 40
    e = sicp.Engine(0, p)
    if mode != sicp.MODE_GICP:
        e.set_confusion(cm)
    e.set_source(src, sl)
    e.set_target(tgt, tl)
    return e, src, tgt, _qt(_near(T, seed))


def _raw(e, qt, ss=1.0, st=1.0):
    r = sicp.SicpPoseCovarianceResult()
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    assert sicp.lib().sicp_pose_covariance(e._h, sicp._ptr(qt, sicp._dp), ss, st, sicp.C.byref(r)) == sicp.OK
    return bytes(r), r.as_dict()


@pytest.mark.parametrize("n", [2000, 20000])
@pytest.mark.parametrize("mode", MODES)
def test_sums_match_accumulate_bits_and_the_numpy_restatement(mode, n):
    e, src, tgt, qt = _engine(mode, n, 11)
    with e:
        r = e.pose_covariance(qt)
        idx, _, w = e.correspondences(qt)
        out28 = e.accumulate(qt)
        assert np.array_equal(r["hessian21"], out28[:21])
        assert np.array_equal(r["gradient"], out28[21:27])
        assert r["cost"] == out28[27]
        assert r["active"] == int((idx >= 0).sum()) > 0
        _, sn, _, _ = e.covariances(sicp.SOURCE)
        _, tn, _, _ = e.covariances(sicp.TARGET)
        p = e.get_params()
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    S_src, S_tgt = ref.cross_sums(T[:3, :3], T[:3, 3], src.astype(np.float64), sn, tgt.astype(np.float64), tn, idx,
                                  w if mode == sicp.MODE_EM else None, p.epsilon, ref.MODES[mode], p.cauchy_a)
    for got, want in ((r["cross_source"], S_src), (r["cross_target"], S_tgt)):
        scale = np.abs(np.diag(want)).max()
        assert scale > 0
        assert np.abs(got - want).max() <= 1e-8 * scale, (mode, n, np.abs(got - want).max() / scale)


@pytest.mark.parametrize("mode", [sicp.MODE_GICP, sicp.MODE_EM])
def test_small_pair_matches_finite_differences(mode):
    src, sl, tgt, tl, T_gt = synth.config1_pair(seed=4, n_per_label=100)  # 300 x 300 points
    p = sicp.default_params(mode)
    p.num_classes = 4
    qt = _qt(_near(T_gt, 5))
    with sicp.Engine(0, p) as e:
        if mode == sicp.MODE_EM:
            e.set_confusion(synth.confusion_matrix(4))
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        r = e.pose_covariance(qt)
        idx, _, w = e.correspondences(qt)
        _, sn, _, _ = e.covariances(sicp.SOURCE)
        _, tn, _, _ = e.covariances(sicp.TARGET)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    ii, cc = np.nonzero(idx >= 0)
    jj = idx[ii, cc]
    ww = w[ii, cc] if mode == sicp.MODE_EM else np.ones(len(ii))
    mname = ref.MODES[mode]
    S64, T64 = src.astype(np.float64), tgt.astype(np.float64)
    pairs = np.stack([np.arange(len(ii)), np.arange(len(ii))], 1)

    def grads(S, Tg):  # per slot g_i, from lm_ref
        rr, J = lm_ref.residuals_and_jacobian(T, S[ii], sn[ii], Tg[jj], tn[jj], pairs, p.epsilon)
        _, drho = lm_ref.loss(mname, rr * rr, ww, p.cauchy_a)
        return (drho * rr)[:, None] * J

    h = 1e-6
    Gs, Gt = np.zeros((len(src), 6, 3)), np.zeros((len(tgt), 6, 3))
    for col in range(3):  # every point moved at once: slot i's gradient depends on its own two points only
        e3 = np.zeros(3)
        e3[col] = h
        d = (grads(S64 + e3, T64) - grads(S64 - e3, T64)) / (2 * h)
        np.add.at(Gs[:, :, col], ii, d)
        d = (grads(S64, T64 + e3) - grads(S64, T64 - e3)) / (2 * h)
        np.add.at(Gt[:, :, col], jj, d)
    for got, G in ((r["cross_source"], Gs), (r["cross_target"], Gt)):
        want = np.einsum("nij,nkj->ik", G, G)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(np.diag(want)).max()


def test_covariance_algebra_sigma_scaling_and_repeat_bits():
    e, _, _, qt = _engine(sicp.MODE_EM, 20000, 12)
    with e:
        b1, r1 = _raw(e, qt)
        b2, _ = _raw(e, qt)
        _, r4 = _raw(e, qt, 2.0, 2.0)
        _, rs = _raw(e, qt, 0.3, 0.0)
    assert b1 == b2
    assert r1["positive_definite"]
    cov, gn = ref.covariance(r1["hessian"], r1["cross_source"], r1["cross_target"], 1.0, 1.0)
    assert np.abs(r1["covariance"] - cov).max() <= 1e-10 * np.abs(cov).max()
    assert np.abs(r1["covariance_gn"] - gn).max() <= 1e-10 * np.abs(gn).max()
    assert np.array_equal(r1["covariance"], r1["covariance"].T)
    assert np.allclose(r4["covariance"], 4 * r1["covariance"], rtol=1e-12, atol=0)
    cov_s, _ = ref.covariance(r1["hessian"], r1["cross_source"], r1["cross_target"], 0.3, 0.0)
    assert np.abs(rs["covariance"] - cov_s).max() <= 1e-10 * np.abs(cov_s).max()
    assert np.linalg.eigvalsh(r1["covariance"]).min() > 0


@pytest.mark.parametrize("mode", MODES)
def test_batch_rows_equal_lone_calls(mode):
    es, qts = [], []
    try:
        for k in range(8):
            e, _, _, qt = _engine(mode, 2000 + 250 * k, 20 + k)
            es.append(e)
            qts.append(qt)
        lone = [_raw(e, q)[0] for e, q in zip(es, qts)]
        out = (sicp.SicpPoseCovarianceResult * 8)()
        status = np.full(8, 99, dtype=np.int32)
        q = np.ascontiguousarray(np.stack(qts))
        rc = sicp.lib().sicp_pose_covariance_batch(sicp._handles(es), 8, sicp._ptr(q, sicp._dp), 1.0, 1.0, out, sicp._ptr(status, sicp._ip))
        assert rc == sicp.OK and (status == 0).all()
        for k in range(8):
            assert bytes(out[k]) == lone[k], k
        res = sicp.pose_covariance_batch(es, q)
        assert all(s == sicp.OK for s, _ in res)
    finally:
        for e in es:
            e.close()


def test_zero_active_slots_and_general_covariances():
    e, _, _, qt = _engine(sicp.MODE_GICP, 2000, 13)
    with e:
        p = e.get_params()
        p.gate_sq = 1e-30
        e.set_params(p)
        r = e.pose_covariance(qt)
        assert r["active"] == 0 and not r["positive_definite"]
        assert np.isnan(r["covariance"]).all() and np.isnan(r["covariance_gn"]).all()
        assert not r["cross_source"].any() and not r["cross_target"].any()
        e.set_covariances(sicp.SOURCE, np.tile(0.5 * np.eye(3), (2000, 1, 1)))  # not I - (1 - eps) n n^T
        with pytest.raises(sicp.SicpError) as err:
            e.pose_covariance(qt)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT
        assert "general form" in sicp.lib().sicp_last_error(e._h).decode()
    # a failing pair does not stop the others
    a, _, _, qa = _engine(sicp.MODE_GICP, 2000, 14)
    b = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))  # no clouds
    with a, b:
        res = sicp.pose_covariance_batch([a, b, a], np.stack([qa, qa, qa]))
        assert [s for s, _ in res] == [sicp.OK, sicp.ERR_NOT_READY, sicp.OK]
        assert np.array_equal(res[0][1]["covariance"], res[2][1]["covariance"])


def test_monte_carlo_nees_in_gicp_mode():
    """Fixed covariances from the noiseless clouds (sicp_set_covariances, reuse_features = 1), 1 cm of noise on both clouds,
    64 registrations from the true pose.  Each trial's covariance is evaluated as a caller would use it: at that trial's
    estimate, on that trial's noisy clouds.  The mean NEES of the estimates' errors must lie in [1.5, 24] for 6 DoF."""
    src0, _, tgt0, _, T_gt = synth.config1_pair(seed=8, n_per_label=700, sigma=0.0)
    qt_gt = _qt(T_gt)
    p = sicp.default_params(sicp.MODE_GICP)
    p.reuse_features = 1
    sigma, trials = 0.01, 64
    with sicp.Engine(0, p) as e0:
        e0.set_source(src0)
        e0.set_target(tgt0)
        cs, _, _, _ = e0.covariances(sicp.SOURCE)
        ct, _, _, _ = e0.covariances(sicp.TARGET)
    rng = np.random.default_rng(9)
    es = []
    try:
        for _ in range(trials):
            e = sicp.Engine(0, p)
            e.set_source((src0 + rng.normal(scale=sigma, size=src0.shape)).astype(np.float32))
            e.set_target((tgt0 + rng.normal(scale=sigma, size=tgt0.shape)).astype(np.float32))
            e.set_covariances(sicp.SOURCE, cs)
            e.set_covariances(sicp.TARGET, ct)
            es.append(e)
        res = sicp.align_batch(es, np.tile(qt_gt, (trials, 1)), want_stats=False)
        qts = np.stack([qt for qt, _ in res])
        covs = sicp.pose_covariance_batch(es, qts, sigma, sigma)
    finally:
        for e in es:
            e.close()
    nees = []
    for qt, (status, c) in zip(qts, covs):
        assert status == sicp.OK and c["positive_definite"]
        T_hat = np.eye(4)
        T_hat[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
        T_hat[:3, 3] = qt[4:]
        xi = _se3_log(np.linalg.inv(T_hat) @ T_gt)  # the error in the tangent space at the estimate (right perturbation)
        nees.append(float(xi @ np.linalg.solve(c["covariance"], xi)))
    mean = float(np.mean(nees))
    print(f"Monte Carlo NEES (GICP, {trials} trials, sigma {sigma} m): mean {mean:.3f} for 6 DoF")
    assert 1.5 <= mean <= 24.0, mean


def test_bad_sigmas_are_refused_on_a_live_handle():
    e, _, _, qt = _engine(sicp.MODE_GICP, 2000, 15)
    with e:
        qt = np.ascontiguousarray(qt)
        qp = sicp._ptr(qt, sicp._dp)
        r = sicp.SicpPoseCovarianceResult()
        sicp.C.memset(sicp.C.byref(r), 0x5A, sicp.C.sizeof(r))
        before = bytes(r)
        for ss, st in ((-1.0, 1.0), (1.0, -1e-300), (float("nan"), 1.0), (1.0, float("inf"))):
            assert sicp.lib().sicp_pose_covariance(e._h, qp, ss, st, sicp.C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
            assert bytes(r) == before
            outs = (sicp.SicpPoseCovarianceResult * 2)()
            sicp.C.memset(outs, 0x5A, sicp.C.sizeof(outs))
            status = np.full(2, 77, dtype=np.int32)
            q2 = np.ascontiguousarray(np.stack([qt, qt]))
            rc = sicp.lib().sicp_pose_covariance_batch(sicp._handles([e, e]), 2, sicp._ptr(q2, sicp._dp), ss, st, outs,
                                                       sicp._ptr(status, sicp._ip))
            assert rc == sicp.ERR_INVALID_ARGUMENT
            assert (status == 77).all() and bytes(outs) == bytes([0x5A]) * sicp.C.sizeof(outs)
        assert "sigma" in sicp.lib().sicp_last_error(e._h).decode()
        assert e.pose_covariance(qt, 0.0, 0.0)["positive_definite"]  # zero noise is allowed


def _se3_log(T):
    """[upsilon; omega] of T (Sophus' SE3::log)"""
    w = Rotation.from_matrix(T[:3, :3]).as_rotvec()
    th = np.linalg.norm(w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-10:
        Vi = np.eye(3) - 0.5 * W
    else:
        Vi = np.eye(3) - 0.5 * W + (1 - th * np.sin(th) / (2 * (1 - np.cos(th)))) / th ** 2 * (W @ W)
    return np.concatenate([Vi @ T[:3, 3], w])
