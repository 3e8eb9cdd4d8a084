"""numpy float64 restatement of EM-ICP's label path -- neighbour lists -> label counts -> projections through the confusion
matrix -> per-slot label factor x geometric gate -> weights and fused labels -- in the reference's order of operations
(em_icp.hpp:77-89,108,224-266,298-301 and gicp_cost_function.h:75-87, as oracle/sicp_oracle.c spells them out).  Whole
arrays at a time: the only Python loops run over the classes and the (four) slots, which is the order the sums are taken in.
tests/test_label_path_cpu.py holds it against the oracle and against its own longdouble form; tests/test_gpu_label_path.py
holds the kernels against it."""
from __future__ import annotations

import numpy as np

LOG_SMALLEST = -1075.0 * np.log(2.0)  # a product below 2^-1075 rounds to exactly 0: where Probability() turns false


# ---- counts ---------------------------------------------------------------------------------------------------------------
def hist_counts(labels, nn, C):
    """uint8 [n, C]: how many of each point's listed neighbours carry class c + 1 (em_icp.hpp:301 as a count).  -1 entries and
    labels outside 1..C are ignored."""
    nn = np.asarray(nn)
    n = nn.shape[0]
    lab = np.asarray(labels).astype(np.int64)[np.maximum(nn, 0)]
    ok = (nn >= 0) & (lab >= 1) & (lab <= C)
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], nn.shape)
    flat = rows[ok] * C + (lab[ok] - 1)
    counts = np.bincount(flat, minlength=n * C).reshape(n, C)
    assert counts.max(initial=0) <= 255
    return counts.astype(np.uint8)


def hval(k):
    """hval[c] = 0 + 1/k + ... + 1/k (c times), every addition rounded: the value a bin holds after c increments
    (em_icp.hpp:279,301).  np.cumsum of a 1-D array adds one element after the other."""
    return np.concatenate([[0.0], np.cumsum(np.full(k, 1.0 / k))])


# ---- projections and the label factor ---------------------------------------------------------------------------------------
def projections(counts, cm, k, dtype=np.float64):
    """proj[i, s] = sum_r hval[counts[i, r]] * cm[r, s], r ascending, every product rounded on its own (the two inner sums
    of em_icp.hpp:86-87).  dtype = np.longdouble gives the same sums with more digits (the table stays the float64 one: it is
    the data)."""
    cm = np.asarray(cm, dtype=np.float64)
    C = cm.shape[0]
    hv = hval(k)[np.asarray(counts)].astype(dtype)
    cmx = cm.astype(dtype)
    proj = np.zeros((hv.shape[0], C), dtype=dtype)
    for r in range(C):
        proj += hv[:, r, None] * cmx[r][None, :]
    return proj


def label_factor(ps, pt, idx):
    """[n, K]: sum_s pt[j, s] * ps[i, s], s ascending, each product rounded on its own (em_icp.hpp:84-89); slots with
    idx < 0 are computed on target 0 and are for the caller to mask"""
    j = np.maximum(np.asarray(idx), 0)
    f = np.zeros(j.shape, dtype=ps.dtype)
    for s in range(ps.shape[1]):
        f += pt[j, s] * ps[:, None, s]
    return f


# ---- the geometric gate -----------------------------------------------------------------------------------------------------
def rotation(qt):
    """Eigen's Quaternion::toRotationMatrix, qt = (x, y, z, w, tx, ty, tz)"""
    x, y, z, w = (float(v) for v in qt[:4])
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def _mul(A, B):
    """3x3 products over leading axes, every entry (a0 b0 + a1 b1) + a2 b2"""
    return (A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]


def _vec(A, v):
    return (A[..., :, 0] * v[..., None, 0] + A[..., :, 1] * v[..., None, 1]) + A[..., :, 2] * v[..., None, 2]


def _det(A):
    return (A[..., 0, 0] * (A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1])
            - A[..., 0, 1] * (A[..., 1, 0] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 0])) \
        + A[..., 0, 2] * (A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0])


def _inverse(A):
    """Eigen's Matrix3d::inverse(): cofactors over the determinant"""
    a = [[A[..., i, j] for j in range(3)] for i in range(3)]
    c00 = a[1][1] * a[2][2] - a[1][2] * a[2][1]
    c10 = a[1][2] * a[2][0] - a[1][0] * a[2][2]
    c20 = a[1][0] * a[2][1] - a[1][1] * a[2][0]
    det = (a[0][0] * c00 + a[0][1] * c10) + a[0][2] * c20
    inv = 1.0 / det
    M = np.empty(A.shape)
    M[..., 0, 0] = c00 * inv
    M[..., 0, 1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) * inv
    M[..., 0, 2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) * inv
    M[..., 1, 0] = c10 * inv
    M[..., 1, 1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) * inv
    M[..., 1, 2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) * inv
    M[..., 2, 0] = c20 * inv
    M[..., 2, 1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) * inv
    M[..., 2, 2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) * inv
    return M


def gate(qt, src, scov, tgt, tcov, idx, as_bool=True):
    """GICPCostFunction::Probability of every slot (gicp_cost_function.h:75-87): A = C_t + R C_s R^T, r = res^T A^-1 res,
    pow(det(2 pi A), -1/2) * exp(-r / 2) -- returned as the double, or (quirk Q1, what the reference does) as `!= 0`.
    Returns (gate [n, K] float64, r, log-probability = -1/2 log det(2 pi A) - r / 2).  Slots with idx < 0 are computed on
    target 0 and are for the caller to mask."""
    qt = np.asarray(qt, dtype=np.float64)
    j = np.maximum(np.asarray(idx), 0)
    R = rotation(qt)
    scov = np.asarray(scov, dtype=np.float64).reshape(-1, 3, 3)
    tcov = np.asarray(tcov, dtype=np.float64).reshape(-1, 3, 3)
    ps = np.asarray(src, dtype=np.float32).astype(np.float64)
    pt = np.asarray(tgt, dtype=np.float32).astype(np.float64)
    Rb = np.broadcast_to(R, scov.shape)
    RCRt = _mul(_mul(Rb, scov), np.broadcast_to(R.T, scov.shape))
    A = tcov[j] + RCRt[:, None]
    M = _inverse(A)
    tp = _vec(np.broadcast_to(R, (len(ps), 3, 3)), ps) + qt[4:7]
    res = pt[j] - tp[:, None, :]
    dT = _vec(M, res)
    r = (res[..., 0] * dT[..., 0] + res[..., 1] * dT[..., 1]) + res[..., 2] * dT[..., 2]
    mahal = -1.0 / 2.0 * r
    det = _det(2 * np.pi * A)
    with np.errstate(under="ignore"):
        probability = np.power(det, -1.0 / 2.0) * np.exp(mahal)
    logp = -0.5 * np.log(det) + mahal
    g = (probability != 0.0).astype(np.float64) if as_bool else probability
    return g, r, logp


def near_edge(logp, rel=1e-9):
    """slots whose probability lies so close to the smallest double that pow / exp of two libraries may disagree on `!= 0`"""
    return np.abs(logp - LOG_SMALLEST) <= rel * abs(LOG_SMALLEST)


# ---- weights and fused labels -------------------------------------------------------------------------------------------------
def weights(counts_s, counts_t, cm, k, qt, src, scov, tgt, tcov, idx, as_bool=True):
    """the EM weight of every slot (em_icp.hpp:108): label factor x gate, 0 where idx < 0"""
    ps, pt = projections(counts_s, cm, k), projections(counts_t, cm, k)
    g, _, _ = gate(qt, src, scov, tgt, tcov, idx, as_bool)
    return np.where(np.asarray(idx) >= 0, label_factor(ps, pt, idx) * g, 0.0)


def fused_scores(ps, pt, idx, g):
    """[n, C]: per class s, sum over the live slots in slot order of (pt[j, s] * ps[i, s]) * gate (em_icp.hpp:243-253)"""
    idx = np.asarray(idx)
    j = np.maximum(idx, 0)
    sc = np.zeros(ps.shape)
    for c in range(idx.shape[1]):
        sc += np.where(idx[:, c, None] >= 0, (pt[j[:, c]] * ps) * g[:, c, None], 0.0)
    return sc


def fused_labels(scores):
    """arg max over the classes, the first maximum wins, and a point whose scores are all 0 (no live slot) gets label 1
    (em_icp.hpp:256-265: `>` against a running maximum that starts at 0)"""
    scores = np.asarray(scores)
    return (np.where(scores.max(axis=1) > 0, np.argmax(scores, axis=1), 0) + 1).astype(np.uint32)


def top_two(scores):
    """(label of the best class, label of the runner-up, relative gap between their scores; gap = inf for rows of zeros)"""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.shape[1] == 1:
        one = np.ones(len(scores), np.uint32)
        return one, one, np.full(len(scores), np.inf)
    order = np.argsort(-scores, axis=1, kind="stable")
    rows = np.arange(len(scores))
    a, b = scores[rows, order[:, 0]], scores[rows, order[:, 1]]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(a > 0, (a - b) / a, np.inf)
    return (order[:, 0] + 1).astype(np.uint32), (order[:, 1] + 1).astype(np.uint32), gap
