"""Inputs, sizes and bars of the full-matrix covariance tests (tests/test_general_cov_cases_cpu.py on the cases and the oracle
alone, tests/test_gpu_general_covariances.py through the library): caller covariances that are NOT I - (1 - eps) n n^T
(sicp_set_covariances -> Cloud::cov_general) and the code they switch a registration onto -- accumulate_general_kernel
(csrc/solve_kernels.hip), its own chunk split, the trust-region loop on the host, the matrices packed to six doubles per
point in device order.

The reference everywhere is the oracle's literal Evaluate / solve / outer loop on the indices the engine reports and on
the matrices the engine hands back (oracle_lib.accumulate, solver_option_cases.expectation / outer_replay); above it stands
accumulate_cases.accumulate_longdouble.  Weights are None: SICP_MODE_GICP and SICP_MODE_SEMANTIC carry none.

Points, parameter builders, bars and the longdouble restatement are those of tests/accumulate_cases.py, imported, not copied.

No figure in this file is an expected value of a GPU run."""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from accumulate_cases import (LOSS_A, accumulate_longdouble, assert_sums, bars, far_pose, mid_pair, oracle_distance, oracle_params,  # noqa: F401
                              pair20k, project_bars, semantic_first_class_small, semantic_one_point_class)
import accumulate_cases as A
from solver_option_cases import expectation, outer_replay  # noqa: F401

GATE_OPEN = A.GATE_OPEN
HALF_GATE_SHIFT = (0.0, 22.0, 0.0)       # the reference drops about half of the mid-size pair's slots there
SYMMETRY_TOL = 1e-8                      # sicp_set_covariances: |C_ab - C_ba| <= tol (1 + |C_ab|)   (csrc/sicp_api.cpp)
FORM_TOL = 1e-8                          # ... and the distance from I - (1 - eps) n n^T up to which a matrix is of that form
POSE_BOUND = 1e-7                        # rad and m against the oracle (tests/test_gpu_validation.py, tests/test_gpu_stream.py)


# ---- the general kernel's split (accumulate_general_kernel; eval28 in csrc/stages.cpp) ------------------------------------------------
def general_chunks(n_s, K):
    """n_chunks = accumulate_blocks(n_s K, K): the product kernel's chunk count, also the general kernel's grid"""
    return A.n_chunks(n_s, K)


def general_split(n_s, K):
    """[(s0, s1)] per workgroup: per = ceil(total / n_chunks), s0 = chunk per, s1 = min(total, s0 + per); a lane walks its
    range 256 slots apart"""
    total = n_s * K
    n = general_chunks(n_s, K)
    per = (total + n - 1) // n
    return [(c * per, min(total, c * per + per)) for c in range(n)]


# K -> source sizes: one slot, either side of one lane stride (256 slots), of one chunk (2048 slots), and sizes of several chunks
# whose `per` is no multiple of 256 (tests/test_general_cov_cases_cpu.py asserts each)
SPLIT_SIZES = {1: (1, 2, 255, 256, 257, 2047, 2048, 2049, 16385), 4: (1, 511, 512, 513, 4097), 20: (1, 102, 103, 820)}
SPLIT_CASES = [(K, n) for K, sizes in SPLIT_SIZES.items() for n in sizes]


def split_removals(idx):
    """{what: the index array with one slot dead}: the first slot of every chunk's range under the general split, the last
    source point's last slot, slot 0"""
    n_s, K = idx.shape
    flat = idx.reshape(-1)
    out = {}
    for c, (s0, s1) in enumerate(general_split(n_s, K)):
        if s0 < s1 and c > 0:
            b = flat.copy(); b[s0] = -1
            out[f"first slot of chunk {c}"] = b.reshape(n_s, K)
    a = flat.copy(); a[-1] = -1
    out["last source point"] = a.reshape(n_s, K)
    z = flat.copy(); z[0] = -1
    out["slot 0"] = z.reshape(n_s, K)
    return out


# ---- matrix families --------------------------------------------------------------------------------------------------------------------
FAMILIES = {"spd": (0.05, 1.5), "wide": (1e-6, 10.0), "indef": (0.2, 1.5)}     # eigenvalue (magnitude) ranges
WHICH = ("source", "target", "both")
SEEDS = {"source": 101, "target": 202}
# indef: A = C_t + R C_s R^T comes close to singular at single slots, and then float64 itself is far from the formulas.  Of the
# seed offsets 0 .. 11 this one leaves the float64 oracle closest to its longdouble restatement over every K, loss and pose of
# group 1 (4 x distance = 1.3e-2 of the project bar; tests/test_general_cov_cases_cpu.py holds every case to 0.1).
FAMILY_SEED = {"spd": 0, "wide": 0, "indef": 9}


def symmetrise(C):
    return 0.5 * (C + np.swapaxes(C, -1, -2))


def _eigen_family(rng, n, lo, hi, signs):
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    lam = rng.uniform(lo, hi, size=(n, 3))
    if signs:
        lam = lam * rng.choice([-1.0, 1.0], size=(n, 3))
    return symmetrise(np.einsum("nij,nj,nkj->nik", q, lam, q))


@functools.lru_cache(maxsize=None)
def family(name, side, n, seed_offset=0):
    """n seeded, exactly symmetric, per point distinct matrices Q diag(lam) Q^T of a family for one side of a pair; `indef`
    puts random signs on the SOURCE's eigenvalues only (its target is `spd`)"""
    seed = SEEDS[side] + seed_offset + FAMILY_SEED[name]
    if name == "indef" and side == "target":
        name = "spd"
    lo, hi = FAMILIES[name]
    C = _eigen_family(np.random.default_rng(seed + 1000 * sorted(FAMILIES).index(name)), n, lo, hi, name == "indef")
    C.setflags(write=False)
    return C


def matrices(name, which, n_s, n_t, seed_offset=0):
    """(source matrices or None, target matrices or None): None = that cloud keeps the engine's own I - (1 - eps) n n^T"""
    cs = family(name, "source", n_s, seed_offset) if which in ("source", "both") else None
    ct = family(name, "target", n_t, seed_offset) if which in ("target", "both") else None
    return cs, ct


# 1. every instantiation: K x loss stack x which cloud is general (spd), and the harder families on both
INSTANTIATIONS = [(knn, sq, which, fam) for knn in (1, 4, 20) for sq in (0, 1)
                  for which, fam in (("source", "spd"), ("target", "spd"), ("both", "spd"), ("both", "wide"), ("both", "indef"))]
# one instantiation each away from the default loss scale / epsilon (epsilon moves the `engine` side only)
LOSS_CASES = [(4, 1, "both", "spd", dict(cauchy_a=LOSS_A[0])), (1, 0, "source", "spd", dict(cauchy_a=LOSS_A[-1])),
              (4, 1, "source", "spd", dict(epsilon=1e-1))]
# 4. solve and align on the host loop: spd only
SOLVE_CASES = [(knn, sq, which) for knn in (1, 4) for sq in (0, 1) for which in ("source", "both")]
# a start from which the oracle's default solve rejects steps (asserted where it is used)
FAR_START_SHIFT = (0.5, 0.3, -0.2)
FAR_START_ROT = (0.02, 0.03, -0.05)


def inst_id(knn, sq, which, fam, *rest):
    return "-".join([f"k{knn}", "sqloss" if sq else "cauchy", which, fam] + [str(r) for r in rest])


def far_start(qt):
    """exp([FAR_START_SHIFT; FAR_START_ROT]) * qt"""
    d = np.concatenate([FAR_START_SHIFT, FAR_START_ROT])
    return O.se3_mul(O.se3_exp(d), np.asarray(qt, dtype=np.float64))


# ---- Semantic: the caller's order shuffled ------------------------------------------------------------------------------------------------
SEMANTIC_FIXTURES = {"first_class_small": semantic_first_class_small, "one_point_class": semantic_one_point_class}


@functools.lru_cache(maxsize=None)
def semantic_case(name, shuffled):
    """(src, labels, tgt, labels, qt, source permutation, target permutation): row i of the returned clouds is row perm[i] of
    the fixture (the identity when not shuffled)"""
    src, sl, tgt, tl, qt, _ = SEMANTIC_FIXTURES[name]()
    if shuffled:
        rng = np.random.default_rng(53)
        ps, pt = rng.permutation(len(src)), rng.permutation(len(tgt))
    else:
        ps, pt = np.arange(len(src)), np.arange(len(tgt))
    out = (np.ascontiguousarray(src[ps]), np.ascontiguousarray(sl[ps]), np.ascontiguousarray(tgt[pt]), np.ascontiguousarray(tl[pt]), qt, ps, pt)
    for a in out:
        a.setflags(write=False)
    return out


def semantic_matrices(name, which, shuffled):
    """the spd matrices of a Semantic case, shuffled like its points: a point keeps its matrix"""
    src, _, tgt, _, _, ps, pt = semantic_case(name, shuffled)
    cs, ct = matrices("spd", which, len(src), len(tgt), seed_offset=7)
    return (None if cs is None else np.ascontiguousarray(cs[ps])), (None if ct is None else np.ascontiguousarray(ct[pt]))


# ---- non-finite rows ------------------------------------------------------------------------------------------------------------------------
def with_non_finite_rows(points, cov, seed, fraction=0.03):
    """(points, matrices, mask): `fraction` of the rows, seeded, hold NaN / inf coordinates and an all-NaN matrix"""
    rng = np.random.default_rng(seed)
    n = len(points)
    bad = np.zeros(n, dtype=bool)
    bad[rng.choice(n, size=max(1, int(round(fraction * n))), replace=False)] = True
    p, c = np.array(points), np.array(cov)
    rows = np.nonzero(bad)[0]
    p[rows, rng.integers(0, 3, size=len(rows))] = np.where(rng.random(len(rows)) < 0.5, np.nan, np.inf).astype(np.float32)
    c[rows] = np.nan
    return p, c, bad


def finite_for_oracle(points, cov, bad):
    """the same arrays with the non-finite rows replaced by zeros / identities: no live slot refers to them (asserted by the
    caller), the oracle must not meet a NaN it multiplies by zero"""
    p, c = np.array(points), np.array(cov)
    p[bad] = 0.0
    c[bad] = np.eye(3)
    return p, c


# ---- the kernel's arithmetic in float64 -----------------------------------------------------------------------------------------------------
def closed_form_float64(p, qt, src, scov, tgt, tcov, idx):
    """accumulate_general_kernel restated in numpy float64 for SYMMETRIC matrices: A = C_t + R C_s R^T, a = A^-1 res by
    cofactors, b = R^T a, c = p_s + C_s b, J = [-2 b; 2 b x c], r = res . a, the Ceres losses at s = r^2, the 28 sums.  Its
    distance to accumulate_longdouble is what float64 loses in the closed form itself."""
    q = np.asarray(qt, dtype=np.float64)
    R, t = O.se3_matrix(q)[:3, :3], q[4:]
    idx = np.asarray(idx)
    ii, cc = np.nonzero(idx >= 0)
    out = np.zeros(28)
    if len(ii) == 0:
        return out
    jj = idx[ii, cc]
    ps, pt = np.asarray(src, dtype=np.float32)[ii].astype(np.float64), np.asarray(tgt, dtype=np.float32)[jj].astype(np.float64)
    Cs = np.asarray(scov, dtype=np.float64).reshape(-1, 3, 3)[ii]
    Ct = np.asarray(tcov, dtype=np.float64).reshape(-1, 3, 3)[jj]
    Am = Ct + R @ Cs @ R.T
    a = np.einsum("nij,nj->ni", A._inv3(Am), pt - (ps @ R.T + t))
    res = pt - (ps @ R.T + t)
    r = (res * a).sum(axis=1)
    b = a @ R
    c = ps + np.einsum("nij,nj->ni", Cs, b)
    J = np.concatenate([-2.0 * b, 2.0 * np.cross(b, c)], axis=1)
    ca = float(p.cauchy_a)
    bb = ca * ca
    s = r * r
    if p.use_sqloss:
        v = s + np.finfo(np.float64).eps
        g0, g1 = np.sqrt(v), 1.0 / (2.0 * np.sqrt(v))
        total = 1.0 + g0 / bb
        rho0, rho1 = bb * np.log(total), np.maximum(1.0 / total, np.finfo(np.float64).tiny) * g1
    else:
        total = 1.0 + s / bb
        rho0, rho1 = bb * np.log(total), np.maximum(1.0 / total, np.finfo(np.float64).tiny)
    o = 0
    for x in range(6):
        for y in range(x, 6):
            out[o] = (rho1 * J[:, x] * J[:, y]).sum()
            o += 1
        out[21 + x] = (rho1 * J[:, x] * r).sum()
    out[27] = (0.5 * rho0).sum()
    return out


# ---- the condition that keeps a widened bar from hiding anything ----------------------------------------------------------------------------
WIDENING_CAP = 0.1


def widening(ref, dist):
    """4 x the oracle's distance to the longdouble restatement over the project bar, per group (H, g, cost)"""
    bar = project_bars(ref)
    d = np.asarray(dist, dtype=np.float64)
    return 4.0 * d[:21].max() / bar[0], 4.0 * d[21:27].max() / bar[21], 4.0 * d[27] / bar[27]


# ---- the oracle's own slots and covariances, for the CPU module -----------------------------------------------------------------------------
def oracle_engine_form(points, labels=None, eps=1e-3):
    """I - (1 - eps) n n^T as the oracle's align() computes it: over the whole cloud, or per label segment"""
    if labels is None:
        return O.covariances(points, None, 20, eps, kdtree=True)[0]
    out = np.empty((len(points), 3, 3))
    for L in np.unique(labels):
        m = np.nonzero(labels == L)[0]
        if len(m) == 1:
            out[m] = np.eye(3)
        else:
            out[m] = O.covariances(np.ascontiguousarray(points[m]), None, 20, eps, kdtree=True)[0]
    return out


def oracle_slots(src, tgt, qt, K, gate=250.0, sl=None, tl=None, min_class_pts=400):
    """idx [n_s, K] at qt from the oracle's exact k-NN, -1 beyond the gate; with labels: searched label by label, classes
    with at most min_class_pts source points or without a target skipped"""
    moved = O.transform_points(O.se3_matrix(qt), src)
    if sl is None:
        idx, d2 = O.knn(moved, tgt, K, kdtree=True)
        return np.where(d2 < np.float32(gate), idx, -1).astype(np.int32)
    idx = np.full((len(src), K), -1, dtype=np.int32)
    for L in np.unique(sl):
        ms, mt = np.nonzero(sl == L)[0], np.nonzero(tl == L)[0]
        if len(ms) <= min_class_pts or len(mt) == 0:
            continue
        i, d = O.knn(np.ascontiguousarray(moved[ms]), np.ascontiguousarray(tgt[mt]), min(K, len(mt)), kdtree=True)
        idx[ms, : i.shape[1]] = np.where(d < np.float32(gate), mt[i], -1)
    return idx
