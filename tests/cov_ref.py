"""A restatement of the covariance kernel's contract (cov_body, csrc/feature_kernels.hip; em_icp.hpp:298-340) that shares no
line with the cyclic-Jacobi code of the kernel or of the oracle (orc_sym3_svd_u runs the same sweeps line for line, so a
defect common to both is invisible to a comparison of the two).

For a cloud p (float32), neighbour lists nn in caller indices (-1 = none), k and the flag quirk_float_products:

  A   the moment matrix sum prod_ab / k - mean_a mean_b in np.longdouble, mean = sum p_j / k, the products float32 * float32
      rounded to float32 under the flag and exact (the widened values' products: 48 bits) without it, the divisor k whatever
      the live count (quirk Q3); rounded to float64 at the end;
  S   max_ab sum_j |prod_ab| / k + max_a mean_a^2: the magnitude before the cancellation in c / k - mean mean, the scale to
      which any float64 evaluation of A is uncertain.

A returned unit vector n is then held by its eigen-residual in units of u S, u = 2^-53:

  ratio(n) = max(|A n - (n^T A n) n|_2, |n^T A n| - min |lambda(A)|) / (u S),   lambda from np.linalg.eigvalsh.

A small ratio says that n is an eigenvector of A to working precision AND that it belongs to the eigenvalue of smallest
magnitude (singular values are |eigenvalues|).  Where the gap is wide this pins the direction (Davis-Kahan:
angle <= residual / gap); where the spectrum is degenerate it asks for exactly what is determined.  No point is excluded."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -53
UNIT_BOUND = 540 * U   # | |n| - 1 |: at most 30 sweeps x 3 rotations, each within 6 u of orthogonal
PAIRS = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))
L = np.longdouble


def moments(p32, nn, k, float_products):
    """(A [m, 3, 3] float64, S [m] float64) of the rows of nn (an [m, <= k] int array of indices into p32, -1 = none)"""
    p32 = np.asarray(p32)
    assert p32.dtype == np.float32
    nn = np.asarray(nn)
    live = nn >= 0
    P = p32[np.where(live, nn, 0)]                      # [m, j, 3] float32
    W = P.astype(L) * live[..., None]
    kk = L(k)
    mean = W.sum(axis=1) / kk
    m = nn.shape[0]
    A = np.zeros((m, 3, 3), dtype=L)
    mag = np.zeros(m, dtype=L)
    for a, b in PAIRS:
        if float_products:
            prod = P[..., a] * P[..., b]
            assert prod.dtype == np.float32
            prod = prod.astype(L) * live
        else:
            prod = W[..., a] * W[..., b]                # exact: 24 + 24 bits in a 64-bit significand
        A[:, a, b] = A[:, b, a] = prod.sum(axis=1) / kk - mean[:, a] * mean[:, b]
        mag = np.maximum(mag, np.abs(prod).sum(axis=1) / kk)
    S = mag + (mean * mean).max(axis=1)
    return A.astype(np.float64), S.astype(np.float64)


def min_abs_eigenvalue(A):
    return np.abs(np.linalg.eigvalsh(A)).min(axis=-1)


def ratio(A, S, n):
    """the eigen-residual of each row's n in units of u S (0 / 0 = 0: a cloud at the origin has nothing to get wrong)"""
    Al, nl = A.astype(L), np.asarray(n).astype(L)
    An = np.einsum("nab,nb->na", Al, nl)
    lam = np.einsum("na,na->n", nl, An)
    res = An - lam[:, None] * nl
    res = np.sqrt((res * res).sum(axis=1))
    num = np.maximum(res, np.abs(lam) - min_abs_eigenvalue(A).astype(L)).astype(np.float64)
    den = U * np.asarray(S, dtype=np.float64)
    out = np.full(num.shape, np.inf)
    np.divide(num, den, out=out, where=den > 0)
    out[(den == 0) & (num == 0)] = 0.0
    out[~np.isfinite(num)] = np.inf
    return out


def unit_error(n):
    nl = np.asarray(n).astype(L)
    return np.abs(np.sqrt((nl * nl).sum(axis=1)) - L(1)).astype(np.float64)


def matrix_of_normal(n, eps):
    """C = I - (1 - eps) n n^T exactly as sicp_covariances states it, on the host and in cov9_caller_order_kernel (both
    compiled without contraction): for a <= b, C[a, b] = C[b, a] = (a == b) - ((1 - eps) n[a]) n[b] in float64"""
    n = np.asarray(n, dtype=np.float64)
    ome = np.float64(1.0) - np.float64(eps)
    C = np.empty((len(n), 3, 3))
    for a in range(3):
        for b in range(a, 3):
            e = (1.0 if a == b else 0.0) - (ome * n[:, a]) * n[:, b]
            C[:, a, b] = e
            C[:, b, a] = e
    return C


def signed_smallest_normal(A):
    """the eigenvector of the smallest SIGNED eigenvalue: what an eigen-solve that forgets the magnitudes returns"""
    return np.linalg.eigh(A)[1][..., 0]


def abs_smallest_normal(A):
    w, V = np.linalg.eigh(A)
    c = np.abs(w).argmin(axis=-1)
    return np.take_along_axis(V, c[:, None, None], axis=2)[..., 0]
