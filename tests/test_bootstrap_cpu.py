"""CPU tests of the initial alignment without a pose prior: the numpy restatement tests/bootstrap_ref.py checked against
facts that do not depend on it, and the C ABI of sicp_bootstrap (exports, defaults = exec/bootstrap.h)."""
import ctypes
import importlib
import os

import numpy as np
from scipy.spatial.transform import Rotation

import bootstrap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


def _pf(p1, n1, p2, n2):
    f1, f2, f3, ok = R.pair_features(*(np.asarray([v], np.float64) for v in (p1, n1, p2, n2)))
    return f1[0], f2[0], f3[0], ok[0]


def test_pair_features_closed_form_and_swap_rule():
    # n2 tilted by theta towards the connecting line: |angle2| > |angle1| swaps the roles -> (theta, 0, -sin theta)
    for th in (0.3, -1.1, 1.4):
        s, c = np.sin(th), np.cos(th)
        f1, f2, f3, ok = _pf((0, 0, 0), (0, 0, 1), (1, 0, 0), (s, 0, c))
        assert ok and abs(f1 - th) < 1e-15 and abs(f2) < 1e-15 and abs(f3 + s) < 1e-15
        # the same pair seen from the other end: no swap, the same features
        assert np.allclose(_pf((1, 0, 0), (s, 0, c), (0, 0, 0), (0, 0, 1))[:3], (th, 0.0, -s), atol=1e-15)
    # parallel normals perpendicular to the line: all zero; coincident points / parallel frame: invalid
    assert np.allclose(_pf((0, 0, 0), (0, 0, 1), (2, 0, 0), (0, 0, 1))[:3], 0.0)
    assert not _pf((1, 2, 3), (0, 0, 1), (1, 2, 3), (0, 1, 0))[3]
    assert not _pf((0, 0, 0), (1, 0, 0), (1, 0, 0), (0, 0, 1))[3]
    # in general the swap rule makes the features symmetric in (p, q)
    rng = np.random.default_rng(1)
    p, q = rng.normal(size=(500, 3)), rng.normal(size=(500, 3))
    n = rng.normal(size=(500, 3)); n /= np.linalg.norm(n, axis=1)[:, None]
    m = rng.normal(size=(500, 3)); m /= np.linalg.norm(m, axis=1)[:, None]
    a, b = R.pair_features(p, n, q, m), R.pair_features(q, m, p, n)
    for x, y in zip(a[:3], b[:3]):
        assert np.allclose(x, y, atol=1e-12)


def test_fpfh_is_invariant_under_a_rigid_motion():
    rng = np.random.default_rng(4)
    # a wavy surface: normals from the neighbourhoods, oriented consistently (+z side) rather than towards the origin
    uv = rng.uniform(-6, 6, size=(1500, 2))
    kp = np.c_[uv, 0.6 * np.sin(uv[:, 0]) * np.cos(0.7 * uv[:, 1])].astype(np.float32)
    off, idx, d2 = R.radius_lists(kp, 3.0)
    nrm, _ = R.normals(kp, off, idx)
    nrm[nrm[:, 2] < 0] *= -1
    f = R.fpfh(kp, nrm, off, idx, d2)
    Rm = Rotation.from_rotvec([0.4, -1.2, 2.0]).as_matrix()
    kp2 = (kp.astype(np.float64) @ Rm.T + [5.0, -3.0, 1.0]).astype(np.float32)
    off2, idx2, d22 = R.radius_lists(kp2, 3.0)
    f2 = R.fpfh(kp2, nrm @ Rm.T, off, idx, d2)
    assert np.isfinite(f).all()
    # the same histograms up to f32 rounding, except where an angle sits on a bin edge
    close = np.isclose(f, f2, rtol=1e-4, atol=1e-4).all(axis=1)
    assert close.mean() > 0.98
    assert np.abs(f - f2).mean() < 1e-2
    # the neighbourhoods themselves survive the motion but for pairs on the radius
    assert abs(len(idx2) - len(idx)) <= 0.001 * len(idx)


def test_umeyama_recovers_a_planted_transform_from_three_pairs():
    rng = np.random.default_rng(7)
    for _ in range(20):
        Rm = Rotation.random(random_state=rng).as_matrix()
        t = rng.uniform(-20, 20, 3)
        src = rng.uniform(-10, 10, size=(3, 3))
        M = R.umeyama(src, src @ Rm.T + t)
        assert np.abs(M[:, :3] - Rm).max() < 1e-12 and np.abs(M[:, 3] - t).max() < 1e-12


def test_prng_sequence_is_pinned():
    # splitmix64's published test vector (seed 1234567) and the engine's index mapping for the default seed
    r = R.SplitMix64(1234567)
    assert [r.next() for _ in range(5)] == [6457827717110365317, 3203168211198807973, 9817491932198370423,
                                            4593380528125082431, 16408922859458223821]
    assert R.SplitMix64(0).next() == 0xE220A8397B1DCDAF
    r = R.SplitMix64(1)
    assert [r.index(1000) for _ in range(8)] == [566, 745, 971, 444, 444, 762, 877, 523]


def test_voxel_grid_restatement_on_a_hand_built_cloud():
    p = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.5, 0.1, 0.1], [-0.1, 0, 0], [36, 0, 0], [-40, 0, 0], [np.nan, 0, 0]], np.float32)
    kp = R.voxel_keypoints(p)
    # box filter is signed (x = -40 stays, x = 36 goes); voxels in ascending index: x = -40, [-0.4, 0), [0, 0.4), [0.4, 0.8)
    assert np.array_equal(kp, np.array([[-40, 0, 0], [-0.1, 0, 0], [0.2, 0.1, 0.1], [0.5, 0.1, 0.1]], np.float32))
    try:
        R.voxel_keypoints(np.array([[0, 0, 0], [30, 30, 30]], np.float32), leaf=1e-4)
        assert False, "overflow not detected"
    except OverflowError:
        pass


def test_library_exports_bootstrap_and_defaults_are_the_reference_constants():
    lib = ctypes.CDLL(sicp.build())
    for name in ("sicp_bootstrap", "sicp_default_bootstrap_params", "sicp_bootstrap_keypoints", "sicp_bootstrap_score"):
        assert hasattr(lib, name)
    p = sicp.default_bootstrap_params()
    # exec/bootstrap.h:24-65 and PCL's SampleConsensusInitialAlignment defaults (nr_samples 3, k_correspondences 10)
    assert (p.box_max, p.leaf_size, p.normal_radius, p.feature_radius) == (35.0, 0.4, 3.0, 3.0)
    assert (p.min_sample_distance, p.max_corr_distance, p.max_iterations) == (0.4, 0.8, 500)
    assert (p.nr_samples, p.k_correspondences, p.seed) == (3, 10, 1)
    for k, v in R.DEFAULTS.items():
        assert getattr(p, k) == v
