"""CPU tests of the deskew rules (include/sicp.h, "deskewing a scan"): the numpy restatement (tests/deskew_ref.py) against an
independent float64 computation within the bound the header states, the constant of that bound, and the definition of the
constant-velocity knots against scipy's matrix exponential and logarithm.

The bound, per point in interval a of the relative knots K:
  Theta = the angle of K_a^-1 K_(a+1), L = |t_(a+1) - t_a|.
  rotation: the component-wise blend of two unit quaternions lies on their great circle, at the half-angle
    phi(u) = atan2(u sin h, (1 - u) + u cos h), h = Theta / 2, instead of u h; 2 (phi - u h) = (Theta^3 / 24) u (1 - u)(1 - 2 u) + ...,
    and u (1 - u)(1 - 2 u) <= sqrt(3) / 18, so the rotation is off by at most (sqrt(3) / 432) Theta^3 (1 + Theta^2): |p| times that.
  translation: a screw motion's translation runs along an arc of angle Theta over the chord of length L (the part along the axis
    is linear in u); the blend runs along the chord.  The two are farthest apart at u = 1/2, by the sagitta
    (L / 2) tan(Theta / 4) = (L Theta / 8)(1 + Theta^2 / 48 + ...).
  rounding: the restatement rounds to float32 once -- half an ulp of the coordinate; one ulp is allowed."""
import numpy as np
import pytest
from scipy.linalg import expm, logm
from scipy.spatial.transform import Rotation, Slerp

import deskew_cases
import deskew_ref as R

C_ROT = np.sqrt(3.0) / 432.0


def _mat(qt):
    M = np.eye(4)
    M[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    M[:3, 3] = qt[4:]
    return M


def _independent(xyz, times, kt, K):
    """p' = K_a exp(u log(K_a^-1 K_(a+1))) p with 4x4 matrix exponentials per point, the rotation checked against Slerp; returns the
    points in float64 and each point's (Theta, L)"""
    m = len(kt)
    out = np.full((len(xyz), 3), np.nan)
    theta, chord = np.zeros(len(xyz)), np.zeros(len(xyz))
    logs = {}
    for i, (p, t) in enumerate(zip(xyz.astype(np.float64), times)):
        if not (np.isfinite(p).all() and np.isfinite(t)):
            continue
        a = int(np.clip(np.searchsorted(kt, t, side="right") - 1, 0, m - 2))
        u = float(np.clip((t - kt[a]) / (kt[a + 1] - kt[a]), 0.0, 1.0))
        if a not in logs:
            A, B = _mat(K[a]), _mat(K[a + 1])
            logs[a] = (A, np.real(logm(np.linalg.inv(A) @ B)), Slerp([0.0, 1.0], Rotation.from_quat(K[a:a + 2, :4])))
        A, lg, slerp = logs[a]
        T = A @ expm(u * lg)
        assert np.abs(T[:3, :3] - slerp([u]).as_matrix()[0]).max() < 1e-12
        out[i] = T[:3, :3] @ p + T[:3, 3]
        theta[i] = np.linalg.norm((Rotation.from_quat(K[a, :4]).inv() * Rotation.from_quat(K[a + 1, :4])).as_rotvec())
        chord[i] = np.linalg.norm(K[a + 1, 4:] - K[a, 4:])
    return out, theta, chord


@pytest.mark.parametrize("name", deskew_cases.SMALL)
def test_restatement_is_within_the_derived_bound_of_an_independent_computation(name):
    c = deskew_cases.case(name)
    K = R.compose_knots(c["knot_qt"], c["ref_qt"])
    got = R.deskew(c["xyz"], c["times"], c["knot_time"], K)
    want, theta, chord = _independent(c["xyz"], c["times"], c["knot_time"], K)
    moved = np.isfinite(want).all(axis=1)
    assert moved.sum() == got["n_moved"] and got["n_points"] == len(c["xyz"])
    norm = np.linalg.norm(c["xyz"][moved].astype(np.float64), axis=1)
    th, L = theta[moved], chord[moved]
    bound = C_ROT * th**3 * (1 + th**2) * norm + 0.5 * L * np.tan(th / 4)
    p = got["points"][moved]
    err = np.abs(p.astype(np.float64) - want[moved])
    ulp = np.spacing(np.abs(p)).astype(np.float64)
    worst = (err - ulp).max(axis=1) / np.maximum(bound, 1e-300)
    print(name, "Theta max", th.max(), "L max", L.max(), "bound max", bound.max(), "err max", err.max(), "worst (err - ulp) / bound", worst.max())
    assert (err <= bound[:, None] + ulp).all()
    # the other classes: bit for bit
    finite = np.isfinite(c["xyz"]).all(axis=1)
    assert got["points"][~finite].tobytes() == c["xyz"][~finite].tobytes()
    bad = finite & ~np.isfinite(c["times"])
    assert (got["points"][bad].view(np.uint32) == 0x7FC00000).all() and got["n_bad_time"] == bad.sum()
    assert got["n_finite"] == finite.sum()
    assert got["n_clamped_lo"] == (moved & (c["times"] < c["knot_time"][0])).sum()
    assert got["n_clamped_hi"] == (moved & (c["times"] > c["knot_time"][-1])).sum()


def test_cases_cover_what_they_claim():
    for name in deskew_cases.SMALL:
        c = deskew_cases.case(name)
        K = R.compose_knots(c["knot_qt"], c["ref_qt"])
        dots = (K[1:, :4] * K[:-1, :4]).sum(axis=1)
        assert (dots > 0).all() and np.abs(np.linalg.norm(K[:, :4], axis=1) - 1).max() < 1e-12, name
    raw = deskew_cases.case("sign_flip")["knot_qt"]
    assert ((raw[1:, :4] * raw[:-1, :4]).sum(axis=1) < 0).sum() > 20
    half = deskew_cases.case("half_turn")["knot_qt"]
    assert abs(np.linalg.norm((Rotation.from_quat(half[0, :4]).inv() * Rotation.from_quat(half[-1, :4])).as_rotvec()) - np.pi) < 0.02
    r = R.deskew(*(deskew_cases.case("clamped")[k] for k in ("xyz", "times", "knot_time")), R.compose_knots(deskew_cases.case("clamped")["knot_qt"]))
    assert r["n_clamped_lo"] == 21 and r["n_clamped_hi"] == 31
    r = R.deskew(*(deskew_cases.case("bad_times")[k] for k in ("xyz", "times", "knot_time")), R.compose_knots(deskew_cases.case("bad_times")["knot_qt"]))
    assert r["n_bad_time"] == 8 and r["n_moved"] == 192
    c = deskew_cases.case("bad_points")
    r = R.deskew(c["xyz"], c["times"], c["knot_time"], R.compose_knots(c["knot_qt"]))
    assert r["n_finite"] == 194 and r["n_bad_time"] == 2 and r["n_moved"] == 192
    # ref = NULL is the last knot: the last relative knot is the identity; a knot as ref makes that knot the identity
    assert np.abs(R.compose_knots(c["knot_qt"])[-1] - [0, 0, 0, 1, 0, 0, 0]).max() < 1e-13
    k5 = deskew_cases.case("ref_knot")
    K5 = R.compose_knots(k5["knot_qt"], k5["ref_qt"])[5]
    assert np.abs(np.abs(K5[3]) - 1).max() < 1e-13 and np.abs(K5[4:]).max() < 1e-12


def test_the_rotation_constant():
    """the blend's angle against the geodesic's over a dense scan of u: the largest difference is sqrt(3) / 432 Theta^3 to within
    Theta^2, from below 1 + Theta^2"""
    u = np.linspace(0.0, 1.0, 200001)
    for theta in (0.02, 0.05, 0.1, 0.2, 0.3, 0.5):
        h = 0.5 * theta
        phi = np.arctan2(u * np.sin(h), (1 - u) + u * np.cos(h))
        worst = np.abs(2 * (phi - u * h)).max()
        ratio = worst / theta**3
        print(theta, worst, ratio / C_ROT)
        assert C_ROT * (1 - theta**2) <= ratio <= C_ROT * (1 + theta**2)
    # and through the restatement's own rotation: a point on the x axis turned about z
    theta = 0.3
    K = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, np.sin(theta / 2), np.cos(theta / 2), 0, 0, 0]], float)
    t = np.linspace(0, 1, 20001)
    out = R.deskew(np.tile(np.float32([1, 0, 0]), (len(t), 1)), t, np.array([0.0, 1.0]), K)["points"].astype(np.float64)
    ang = np.arctan2(out[:, 1], out[:, 0])
    assert abs(np.abs(ang - t * theta).max() / theta**3 - C_ROT) < C_ROT * theta**2 + 1e-6 / theta**3


def test_twist_knots_definition_against_matrix_exponentials():
    rng = np.random.default_rng(7)
    for trial in range(6):
        xi = rng.normal(size=6) * [3, 3, 3, 0.4, 0.4, 0.4] if trial else np.array([1.0, 2.0, 3.0, 0, 0, 0])
        delta = R.se3_exp(xi)
        D = _mat(delta)
        nk = (2, 3, 33, 7, 1024, 5)[trial]
        kt, kq = R.twist_knots(delta, 5.0, 5.1, nk)
        assert kt[0] == 5.0 and abs(kt[-1] - 5.1) < 1e-15 and (np.diff(kt) > 0).all()
        lg = np.real(logm(D))
        for k in sorted({0, 1, nk // 2, nk - 1}):
            want = expm(k / (nk - 1) * lg)
            assert np.abs(_mat(kq[k]) - want).max() < 1e-12, (trial, k)
        assert np.abs(_mat(kq[-1]) - D).max() < 1e-12
    # exp and log are each other's inverse; below Sophus' epsilon of 1e-10 rad both take V = I, off by theta |upsilon| / 2
    for xi, tol in ((np.array([0.3, -0.2, 0.1, 1e-12, 0, 0]), 1e-12 * 0.4), (np.array([0.3, -0.2, 0.1, 0.5, -0.4, 0.3]), 1e-14)):
        assert np.abs(R.se3_log(R.se3_exp(xi)) - xi).max() < tol
