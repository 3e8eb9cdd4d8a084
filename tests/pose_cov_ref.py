"""Numpy restatement of sicp_pose_covariance (include/sicp.h) for the tests.

Per correspondence slot i (source point p, target point q, unit normals n_s, n_t, pose T = (R, t) perturbed on the right as
T exp(delta), delta = [upsilon; omega]):

    d = q - (R p + t)     M = (C_t + R C_s R^T)^-1     a2 = 2 M d     b2 = R^T a2     c = p + 1/2 C_s b2
    r = d^T M d           J = [-b2; b2 x c]             g_i = rho'(r^2) r J
    B_i^z = d g_i / d z = kappa J (dr/dz) + rho'(s) r dJ/dz,   s = r^2,   kappa = rho' + 2 s rho''

with C = I - (1 - eps) n n^T held fixed.  M is formed by a plain 3x3 inverse here (the engine uses the Woodbury form), and
the derivatives are written out from the chain rule, not taken from the engine's code.  The tests check them against
central differences of an independent gradient (lm_ref.residuals_and_jacobian + lm_ref.loss)."""
from __future__ import annotations

import numpy as np

from np_ref import DBL_EPS

MODES = {0: "gicp", 1: "em", 2: "semantic"}  # sicp.MODE_* -> the loss stacks of lm_ref.loss


def _skew(v):
    """[v]x for a stack of vectors: (n, 3) -> (n, 3, 3)"""
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], 1)


def rho1_kappa(mode, s, w, a):
    """rho'(s) and kappa = rho'(s) + 2 s rho''(s) of the engine's loss stacks, closed forms (no cancellation)."""
    b = a * a
    s = np.asarray(s, dtype=np.float64)
    if mode in ("gicp", "em"):
        u = np.sqrt(s + DBL_EPS)
        q = 1.0 + u / b
        rho1 = w / (2.0 * u * q)
        kappa = w * DBL_EPS / (2.0 * u ** 3 * q) - w * s / (2.0 * b * u ** 2 * q ** 2)
        return rho1, kappa
    q = 1.0 + s / b
    return w / q, w * (1.0 - s / b) / (q * q)


def slot_terms(R, t, p, ns, q, nt, eps, mode, a, w):
    """r, J (n, 6), B^p, B^q (n, 6, 3) of every slot (rows of p / ns / q / nt / w)."""
    k = 1.0 - eps
    n = len(p)
    I = np.eye(3)[None]
    Cs = I - k * ns[:, :, None] * ns[:, None, :]
    Ct = I - k * nt[:, :, None] * nt[:, None, :]
    M = np.linalg.inv(Ct + R[None] @ Cs @ R.T[None])
    d = q - (p @ R.T + t)
    a2 = 2.0 * np.einsum("nij,nj->ni", M, d)
    r = 0.5 * np.einsum("ni,ni->n", d, a2)
    b2 = a2 @ R
    c = p + 0.5 * np.einsum("nij,nj->ni", Cs, b2)
    J = np.concatenate([-b2, np.cross(b2, c)], axis=1)
    rho1, kappa = rho1_kappa(mode, r * r, w, a)
    D = 2.0 * R.T[None] @ M                     # d b2 / d q
    Dp = -D @ R[None]                           # d b2 / d p
    Eq = 0.5 * Cs @ D                           # d c / d q
    Ep = I + 0.5 * Cs @ Dp                      # d c / d p
    Sb, Sc = _skew(b2), _skew(c)
    dJq = np.concatenate([-D, Sb @ Eq - Sc @ D], axis=1)
    dJp = np.concatenate([-Dp, Sb @ Ep - Sc @ Dp], axis=1)
    f = (rho1 * r)[:, None, None]
    Bq = kappa[:, None, None] * J[:, :, None] * a2[:, None, :] + f * dJq
    Bp = kappa[:, None, None] * J[:, :, None] * (-b2)[:, None, :] + f * dJp
    assert Bq.shape == (n, 6, 3)
    return r, J, Bp, Bq


def cross_sums(R, t, src, sn, tgt, tn, idx, w, eps, mode, a):
    """S_src, S_tgt (6x6) of correspondences idx [n_s, K] (-1 = none) with weights w [n_s, K] (None: 1)."""
    n_s, K = idx.shape
    ii, cc = np.nonzero(idx >= 0)
    jj = idx[ii, cc]
    ww = np.ones(len(ii)) if w is None else w[ii, cc]
    S_src, S_tgt = np.zeros((6, 6)), np.zeros((6, 6))
    if len(ii) == 0:
        return S_src, S_tgt
    _, _, Bp, Bq = slot_terms(R, t, src[ii], sn[ii], tgt[jj], tn[jj], eps, mode, a, ww)
    Gs = np.zeros((n_s, 6, 3))
    np.add.at(Gs, ii, Bp)
    Gt = np.zeros((len(tgt), 6, 3))
    np.add.at(Gt, jj, Bq)
    S_src = np.einsum("nij,nkj->ik", Gs, Gs)
    S_tgt = np.einsum("nij,nkj->ik", Gt, Gt)
    return S_src, S_tgt


def upper21(M):
    return np.asarray(M)[np.triu_indices(6)]


def full6(u21):
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = u21
    return M + np.triu(M, 1).T


def covariance(H, S_src, S_tgt, sigma_source, sigma_target):
    """(Censi) H^-1 (sigma_s^2 S_src + sigma_t^2 S_tgt) H^-1 and H^-1"""
    Hi = np.linalg.inv(H)
    return Hi @ (sigma_source ** 2 * S_src + sigma_target ** 2 * S_tgt) @ Hi, Hi
