"""CPU tests of sicp_pose_covariance: the ABI (symbols, struct layout, refusals before any device call) and the numpy
restatement of its sums (tests/pose_cov_ref.py) against finite differences of an independent gradient."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import lm_ref
import pose_cov_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")
EPS = 1e-3
MODE_A = {"gicp": 3.0, "em": 3.0, "semantic": 1.5}  # sicp_default_params' cauchy_a per mode


def test_entry_points_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "sicp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sicp_pose_covariance", "sicp_pose_covariance_batch"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(C.CDLL(sicp.build()), name), name


def test_result_struct_matches_the_c_compiler():
    code = textwrap.dedent(
        """
        #include <stddef.h>
        #include <stdio.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %zu %zu\\n", sizeof(sicp_pose_covariance_result), offsetof(sicp_pose_covariance_result, covariance),
                 offsetof(sicp_pose_covariance_result, active), offsetof(sicp_pose_covariance_result, positive_definite));
          return 0;
        }
        """
    )
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size, cov, act, pd = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    R = sicp.SicpPoseCovarianceResult
    assert C.sizeof(R) == size
    assert (R.covariance.offset, R.active.offset, R.positive_definite.offset) == (cov, act, pd)


def test_refusals_happen_before_any_device_call():
    lib = sicp.lib()
    qt = np.array([0, 0, 0, 1, 0, 0, 0.0])
    qp = qt.ctypes.data_as(C.POINTER(C.c_double))
    r = sicp.SicpPoseCovarianceResult()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    before = bytes(r)
    assert lib.sicp_pose_covariance(None, qp, 1.0, 1.0, C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_pose_covariance(None, qp, -1.0, 1.0, C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_pose_covariance(None, qp, 1.0, float("nan"), C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_pose_covariance(None, qp, 1.0, 1.0, None) == sicp.ERR_INVALID_ARGUMENT
    assert bytes(r) == before
    status = np.full(2, 77, dtype=np.int32)
    sp = status.ctypes.data_as(C.POINTER(C.c_int32))
    hs = (C.c_void_p * 2)(None, None)
    qts = np.tile(qt, 2)
    qsp = qts.ctypes.data_as(C.POINTER(C.c_double))
    outs = (sicp.SicpPoseCovarianceResult * 2)()
    assert lib.sicp_pose_covariance_batch(None, 2, qsp, 1.0, 1.0, outs, sp) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_pose_covariance_batch(hs, 0, qsp, 1.0, 1.0, outs, sp) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_pose_covariance_batch(hs, 2, qsp, 1.0, 1.0, outs, sp) == sicp.ERR_INVALID_ARGUMENT  # NULL handles
    assert lib.sicp_pose_covariance_batch(hs, 2, qsp, float("inf"), 1.0, outs, sp) == sicp.ERR_INVALID_ARGUMENT
    assert (status == 77).all()


def _random_slots(rng, n):
    def unit(m):
        v = rng.normal(size=(m, 3))
        return v / np.linalg.norm(v, axis=1, keepdims=True)
    p = rng.uniform(-5, 5, size=(n, 3))
    q = p + rng.normal(scale=0.3, size=(n, 3))
    return p, unit(n), q, unit(n)


def _slot_gradients(T, mode, a, p, ns, q, nt, w):
    """g_i = rho'(r^2) r J per slot from lm_ref (the corrected residual times the corrected Jacobian)"""
    pairs = np.stack([np.arange(len(p)), np.arange(len(p))], 1)
    r, J = lm_ref.residuals_and_jacobian(T, p, ns, q, nt, pairs, EPS)
    _, drho = lm_ref.loss(mode, r * r, w, a)
    return (drho * r)[:, None] * J


@pytest.mark.parametrize("mode", ["gicp", "em", "semantic"])
def test_slot_derivatives_match_central_differences(mode):
    rng = np.random.default_rng({"gicp": 1, "em": 2, "semantic": 3}[mode])
    a = MODE_A[mode]
    for trial in range(4):
        T = np.eye(4)
        T[:3, :3] = Rotation.from_rotvec(rng.normal(scale=0.4, size=3)).as_matrix()
        T[:3, 3] = rng.normal(scale=0.5, size=3)
        p, ns, q, nt = _random_slots(rng, 16)
        w = rng.uniform(0.2, 1.0, size=16) if mode == "em" else np.ones(16)
        _, _, Bp, Bq = ref.slot_terms(T[:3, :3], T[:3, 3], p, ns, q, nt, EPS, mode, a, w)
        h = 1e-6
        for z, B in (("p", Bp), ("q", Bq)):
            fd = np.zeros_like(B)
            for col in range(3):
                e = np.zeros(3)
                e[col] = h
                pp, qp_ = (p + e, q) if z == "p" else (p, q + e)
                pm, qm = (p - e, q) if z == "p" else (p, q - e)
                fd[:, :, col] = (_slot_gradients(T, mode, a, pp, ns, qp_, nt, w) - _slot_gradients(T, mode, a, pm, ns, qm, nt, w)) / (2 * h)
            scale = np.abs(fd).max(axis=(1, 2), keepdims=True) + 1e-12
            assert np.abs(B - fd).max() / scale.max() < 1e-6, (mode, trial, z)
            assert (np.abs(B - fd) / scale).max() < 1e-5, (mode, trial, z)


def test_kappa_matches_mpmath_including_r_to_zero():
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    eps = mp.mpf(np.finfo(np.float64).eps)
    for mode in ("em", "semantic"):
        a, w = 3.0 if mode == "em" else 1.5, 0.7 if mode == "em" else 1.0
        b = mp.mpf(a) ** 2

        def rho(s):
            if mode == "em":
                return w * b * mp.log(1 + mp.sqrt(s + eps) / b)
            return b * mp.log(1 + s / b)

        for r in (0.0, 1e-30, 1e-12, 1e-8, 1e-4, 0.1, 1.0, 7.0, 300.0):
            s = mp.mpf(r) ** 2
            want = mp.diff(rho, s, 1) + 2 * s * mp.diff(rho, s, 2)
            _, got = ref.rho1_kappa(mode, np.float64(r) ** 2, w, a)
            assert abs(mp.mpf(float(got)) - want) <= mp.mpf("1e-13") * abs(want), (mode, r, float(got), float(want))


def test_point_sums_match_differences_of_the_whole_gradient():
    """Target points shared by several slots: G_k must be the derivative of the WHOLE gradient by target point k."""
    rng = np.random.default_rng(7)
    n_s, n_t, K = 7, 4, 3
    for mode in ("gicp", "em", "semantic"):
        a = MODE_A[mode]
        src = rng.uniform(-3, 3, size=(n_s, 3))
        tgt = rng.uniform(-3, 3, size=(n_t, 3))
        sn = rng.normal(size=(n_s, 3))
        sn /= np.linalg.norm(sn, axis=1, keepdims=True)
        tn = rng.normal(size=(n_t, 3))
        tn /= np.linalg.norm(tn, axis=1, keepdims=True)
        idx = rng.integers(0, n_t, size=(n_s, K)).astype(np.int32)
        idx[0, 1] = -1  # a gated-out slot
        w = rng.uniform(0.3, 1.0, size=(n_s, K)) if mode == "em" else None
        T = np.eye(4)
        T[:3, :3] = Rotation.from_rotvec([0.1, -0.2, 0.05]).as_matrix()
        T[:3, 3] = [0.2, 0.1, -0.3]
        ii, cc = np.nonzero(idx >= 0)
        ww = np.ones(len(ii)) if w is None else w[ii, cc]

        def total_gradient(S, Tg):
            return _slot_gradients(T, mode, a, S[ii], sn[ii], Tg[idx[ii, cc]], tn[idx[ii, cc]], ww).sum(0)

        h = 1e-6
        Gs = np.zeros((n_s, 6, 3))
        Gt = np.zeros((n_t, 6, 3))
        for pts, G, is_src in ((src, Gs, True), (tgt, Gt, False)):
            for j in range(len(pts)):
                for col in range(3):
                    P1, P2 = pts.copy(), pts.copy()
                    P1[j, col] += h
                    P2[j, col] -= h
                    g1 = total_gradient(P1, tgt) if is_src else total_gradient(src, P1)
                    g2 = total_gradient(P2, tgt) if is_src else total_gradient(src, P2)
                    G[j, :, col] = (g1 - g2) / (2 * h)
        S_src, S_tgt = ref.cross_sums(T[:3, :3], T[:3, 3], src, sn, tgt, tn, idx, w, EPS, mode, a)
        want_src = np.einsum("nij,nkj->ik", Gs, Gs)
        want_tgt = np.einsum("nij,nkj->ik", Gt, Gt)
        assert np.abs(S_src - want_src).max() <= 1e-6 * np.abs(want_src).max(), mode
        assert np.abs(S_tgt - want_tgt).max() <= 1e-6 * np.abs(want_tgt).max(), mode
        # summing per slot instead of per point would be a different matrix here
        _, _, _, Bq = ref.slot_terms(T[:3, :3], T[:3, 3], src[ii], sn[ii], tgt[idx[ii, cc]], tn[idx[ii, cc]], EPS, mode, a, ww)
        per_slot = np.einsum("nij,nkj->ik", Bq, Bq)
        assert np.abs(per_slot - want_tgt).max() > 1e-3 * np.abs(want_tgt).max(), mode


def test_covariance_algebra():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    H = A @ A.T + 6 * np.eye(6)
    B = rng.normal(size=(6, 6))
    S = B @ B.T
    c1, gn = ref.covariance(H, S, 0 * S, 1.0, 1.0)
    c2, _ = ref.covariance(H, S, 0 * S, 2.0, 1.0)
    assert np.allclose(c2, 4 * c1, rtol=1e-12)
    assert np.allclose(gn @ H, np.eye(6), atol=1e-12)
    assert np.array_equal(ref.full6(ref.upper21(H)), ref.full6(ref.upper21(H)).T)
