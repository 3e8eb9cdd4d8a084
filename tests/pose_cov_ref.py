"""Numpy restatement of sicp_pose_covariance (include/sicp.h) for the tests.

Per correspondence slot i (source point p, target point q, unit normals n_s, n_t, pose T = (R, t) perturbed on the right as
T exp(delta), delta = [upsilon; omega]):

    d = q - (R p + t)     M = (C_t + R C_s R^T)^-1     a2 = 2 M d     b2 = R^T a2     c = p + 1/2 C_s b2
    r = d^T M d           J = [-b2; b2 x c]             g_i = rho'(r^2) r J
    B_i^z = d g_i / d z = kappa J (dr/dz) + rho'(s) r dJ/dz,   s = r^2,   kappa = rho' + 2 s rho''

with C = I - (1 - eps) n n^T held fixed.  M is formed by a plain 3x3 inverse here (the engine uses the Woodbury form), and
the derivatives are written out from the chain rule, not taken from the engine's code.  The tests check them against
central differences of an independent gradient (lm_ref.residuals_and_jacobian + lm_ref.loss).

The loss stack is two settings, whatever the mode (sicp_params): use_sqloss (1: Scaled(Composed(Cauchy(a), SQLoss), w),
0: the plain Cauchy(a)) and cauchy_a.  A mode only names its defaults (STACKS); every function here takes both explicitly
(`use_sqloss=None` means the default of the mode's name).  `dtype=np.longdouble` runs the whole restatement in extended
precision: the distance between the two runs is what float64 itself loses in these formulas."""
from __future__ import annotations

import numpy as np

from np_ref import DBL_EPS

MODES = {0: "gicp", 1: "em", 2: "semantic"}  # sicp.MODE_* -> the loss stacks of lm_ref.loss
STACKS = {"gicp": (1, 3.0), "em": (1, 3.0), "semantic": (0, 1.5)}  # a mode's defaults: (use_sqloss, cauchy_a) of sicp_default_params


def stack_of(mode, use_sqloss=None):
    """use_sqloss as given, or the default of the mode's name"""
    return STACKS[mode][0] if use_sqloss is None else int(bool(use_sqloss))


def effective_weights(w, use_sqloss, n, dtype=np.float64, always=False):
    """THE weight rule (fill_acc in csrc/stages.cpp): the weights of the correspondences (the EM
    probabilities; absent in the other modes) scale the loss only inside the SQLoss stack -- ScaledLoss wraps that stack and
    nothing else.  With use_sqloss = 0 the loss is the plain Cauchy and every live slot counts once.  `w`: one weight per live
    slot or None; `always` applies them regardless (what the engine must NOT compute)."""
    if w is None or not (use_sqloss or always):
        return np.ones(n, dtype=dtype)
    return np.asarray(w, dtype=np.float64).astype(dtype)


def _skew(v):
    """[v]x for a stack of vectors: (n, 3) -> (n, 3, 3)"""
    z = np.zeros(len(v), dtype=v.dtype)
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], -1), np.stack([v[:, 2], z, -v[:, 0]], -1),
                     np.stack([-v[:, 1], v[:, 0], z], -1)], 1)


def rho1_kappa(mode, s, w, a, use_sqloss=None, dtype=np.float64):
    """rho'(s) and kappa = rho'(s) + 2 s rho''(s) of a loss stack, closed forms (no cancellation).  `w` multiplies the loss
    as given (effective_weights decides whether a slot's weight gets here); `a` is cauchy_a."""
    one, two = dtype(1), dtype(2)
    b = dtype(a) * dtype(a)
    s = np.asarray(s, dtype=dtype)
    w = np.asarray(w, dtype=dtype)
    if stack_of(mode, use_sqloss):
        e = dtype(DBL_EPS)
        u = np.sqrt(s + e)
        q = one + u / b
        rho1 = w / (two * u * q)
        kappa = w * e / (two * u ** 3 * q) - w * s / (two * b * u ** 2 * q ** 2)
        return rho1, kappa
    q = one + s / b
    return w / q, w * (one - s / b) / (q * q)


def inv3(A):
    """(n, 3, 3) inverses in closed form, adjugate over determinant (np.linalg.inv does not take longdouble)"""
    a, b, c = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2]
    d, e, f = A[:, 1, 0], A[:, 1, 1], A[:, 1, 2]
    g, h, i = A[:, 2, 0], A[:, 2, 1], A[:, 2, 2]
    adj = np.empty_like(A)
    adj[:, 0, 0], adj[:, 0, 1], adj[:, 0, 2] = e * i - f * h, c * h - b * i, b * f - c * e
    adj[:, 1, 0], adj[:, 1, 1], adj[:, 1, 2] = f * g - d * i, a * i - c * g, c * d - a * f
    adj[:, 2, 0], adj[:, 2, 1], adj[:, 2, 2] = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * adj[:, 0, 0] + b * adj[:, 1, 0] + c * adj[:, 2, 0]
    return adj / det[:, None, None]


def slot_terms(R, t, p, ns, q, nt, eps, mode, a, w, use_sqloss=None, dtype=np.float64):
    """r, J (n, 6), B^p, B^q (n, 6, 3) of every slot (rows of p / ns / q / nt / w)."""
    ld = dtype is not np.float64
    R, t, p, ns, q, nt = (np.asarray(v, dtype=np.float64).astype(dtype) for v in (R, t, p, ns, q, nt))
    k = dtype(1) - dtype(eps)
    half, two = dtype(0.5), dtype(2)
    n = len(p)
    I = np.eye(3, dtype=dtype)[None]
    Cs = I - k * ns[:, :, None] * ns[:, None, :]
    Ct = I - k * nt[:, :, None] * nt[:, None, :]
    A = Ct + R[None] @ Cs @ R.T[None]
    M = inv3(A) if ld else np.linalg.inv(A)
    d = q - (p @ R.T + t)
    a2 = two * np.einsum("nij,nj->ni", M, d)
    r = half * np.einsum("ni,ni->n", d, a2)
    b2 = a2 @ R
    c = p + half * np.einsum("nij,nj->ni", Cs, b2)
    J = np.concatenate([-b2, np.cross(b2, c)], axis=1)
    rho1, kappa = rho1_kappa(mode, r * r, w, a, use_sqloss, dtype)
    D = two * R.T[None] @ M                     # d b2 / d q
    Dp = -D @ R[None]                           # d b2 / d p
    Eq = half * Cs @ D                          # d c / d q
    Ep = I + half * Cs @ Dp                     # d c / d p
    Sb, Sc = _skew(b2), _skew(c)
    dJq = np.concatenate([-D, Sb @ Eq - Sc @ D], axis=1)
    dJp = np.concatenate([-Dp, Sb @ Ep - Sc @ Dp], axis=1)
    f = (rho1 * r)[:, None, None]
    Bq = kappa[:, None, None] * J[:, :, None] * a2[:, None, :] + f * dJq
    Bp = kappa[:, None, None] * J[:, :, None] * (-b2)[:, None, :] + f * dJp
    assert Bq.shape == (n, 6, 3)
    return r, J, Bp, Bq


def cross_sums(R, t, src, sn, tgt, tn, idx, w, eps, mode, a, use_sqloss=None, dtype=np.float64, weights_always=False):
    """S_src, S_tgt (6x6) of correspondences idx [n_s, K] (-1 = none) with weights w [n_s, K] (None: absent); the weights
    enter by effective_weights' rule (`weights_always`: regardless of the stack)."""
    n_s, K = idx.shape
    ii, cc = np.nonzero(idx >= 0)
    jj = idx[ii, cc]
    sq = stack_of(mode, use_sqloss)
    ww = effective_weights(None if w is None else w[ii, cc], sq, len(ii), dtype, weights_always)
    S_src, S_tgt = np.zeros((6, 6), dtype=dtype), np.zeros((6, 6), dtype=dtype)
    if len(ii) == 0:
        return S_src, S_tgt
    _, _, Bp, Bq = slot_terms(R, t, src[ii], sn[ii], tgt[jj], tn[jj], eps, mode, a, ww, sq, dtype)
    Gs = np.zeros((n_s, 6, 3), dtype=dtype)
    np.add.at(Gs, ii, Bp)
    Gt = np.zeros((len(tgt), 6, 3), dtype=dtype)
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
