"""Inputs and the bar of the covariance-kernel tests (tests/test_cov_cases_cpu.py on the oracle and the restatement alone,
tests/test_gpu_covariances.py through the library; the restatement: tests/cov_ref.py).

What the cases are about.  cov_body (csrc/feature_kernels.hip) loads a point's k neighbours in batches of 8 with a guarded
tail, from lists that lie [n][k] or rank-major [k][n]; sums float32 or float64 products; divides by k whatever the live
count; runs at most 30 Jacobi sweeps with an absolute (1e-300) and a relative (1e-34) exit; and returns the column of
smallest |eigenvalue|, ties to the later column.  The clouds are the smallest at which each of these can go wrong:

  every_k    the lidar cloud + 35 m (the float32 products then carry rounding), k = 1..32, flag 1; flag 0 at the batch edges
  rule       clouds where the smallest signed eigenvalue is often not the smallest absolute one, or the spectrum is
             degenerate: lidar + 300 m, a 40 x 40 planar grid (axis-aligned; rotated and offset), 500 collinear points, every
             point 7 times, all points coincident; k in {3, 5, 20, 31}
  scale      the lidar cloud x 1e-3 and x 1e3: the check is scale-free, the kernel's exit thresholds are not
  full       clouds of exactly n = k = 20 points about the origin, z flattened by 1, 1e-3, 1e-6: S ~ |A|, so an early exit
             from the sweeps is not forgiven (the lidar cases have S / |A| of 1e2 .. 1e7)
  short      n < k: the -1 tail, the divisor k
  edge       n around the 256-thread workgroup
  semantic   one labelled cloud whose classes have 1, 2, k - 1, k, k + 1 (k in {5, 20, 32}) and a few hundred points
  dropped    50 non-finite rows among 2000

The bar: ratio <= GAMMA = 4 x the oracle's largest ratio over all of these (the oracle runs the kernel's Jacobi code on
the CPU; the factor 4 leaves room for another legitimate summation or rotation order).  A dropped neighbour, a wrong
divisor, a product of the wrong width or an unconverged sweep lands at 1e6 .. 1e12 (profiles/covariances/)."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np
from scipy.spatial.transform import Rotation

import cov_ref as ref
import oracle_lib as O
import synth

EPS = 1e-3                    # sicp_default_params
ORACLE_MAX_RATIO = 3.036      # measured by tests/test_cov_cases_cpu.py::test_gamma_is_four_times_the_oracles_largest_ratio
GAMMA = 4.0 * ORACLE_MAX_RATIO
BITE_THRESHOLD = 8.0          # a signed-smallest eigenvector "fails" a point above this ratio

Case = namedtuple("Case", "family cloud k flag")

ALL_K = tuple(range(1, 33))
FLAG0_K = (1, 7, 8, 9, 20, 32)
RULE_K = (3, 5, 20, 31)
RULE_CLOUDS = ("lidar+300", "grid", "grid_tilted", "line", "dup7", "coincident")
SCALE_CLOUDS = ("lidar_x1e-3", "lidar_x1e3")
FULL_SEEDS = tuple(range(8))
FULL_FLATTEN = (1.0, 1e-3, 1e-6)
SHORT = tuple((n, 20) for n in (1, 2, 3, 7, 8, 9, 19)) + ((31, 32),)
EDGE_N = (255, 256, 257, 513)
SEMANTIC_K = (5, 20, 32)
SEMANTIC_SIZES = (1, 2, 4, 5, 6, 19, 20, 21, 31, 32, 33, 300, 400)   # class c + 1 has SEMANTIC_SIZES[c] points
N_DROPPED = 50

# the least share of points at which a reference that picks the signed-smallest eigenvector exceeds BITE_THRESHOLD
# (measured shares are printed by tests/test_cov_cases_cpu.py::test_the_rule_cases_bite; the floors lie just below them)
BITES = {
    ("lidar+35", 1): 0.90, ("lidar+35", 2): 0.45,
    ("lidar+300", 3): 0.35, ("lidar+300", 5): 0.07,
    ("grid_tilted", 3): 0.20,
    ("line", 3): 0.40, ("line", 5): 0.40, ("line", 20): 0.40, ("line", 31): 0.40,
    ("dup7", 3): 0.90, ("dup7", 5): 0.90,
}


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _lidar(n):
    return _frozen(synth.lidar_pair(seed=4, n_points=n)[0])


def _rotation(seed):
    return Rotation.from_rotvec(np.random.default_rng(seed).normal(size=3)).as_matrix()


@functools.lru_cache(maxsize=None)
def cloud(name):
    """the float32 [n, 3] cloud of that name, built once and read-only"""
    f32 = np.float32
    if name == "lidar":
        return _lidar(3000)
    if name.startswith("lidar+"):
        return _frozen((_lidar(3000).astype(np.float64) + float(name[6:])).astype(f32))
    if name.startswith("lidar_x"):
        return _frozen((_lidar(3000).astype(np.float64) * float(name[7:])).astype(f32))
    if name in ("grid", "grid_tilted"):
        i, j = np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij")
        g = np.stack([0.25 * i.ravel(), 0.25 * j.ravel(), np.full(1600, 2.0)], axis=1)
        if name == "grid_tilted":
            g = g @ _rotation(71).T + np.array([12.5, -7.25, 3.125])
        return _frozen(g.astype(f32))
    if name == "line":
        t = np.sort(np.random.default_rng(72).uniform(-20.0, 20.0, 500))
        d = _rotation(73)[:, 0]
        return _frozen((t[:, None] * d[None, :] + np.array([4.0, 9.0, -1.5])).astype(f32))
    if name == "dup7":
        return _frozen(np.repeat(cloud("lidar+35")[:400], 7, axis=0))
    if name == "coincident":
        return _frozen(np.tile(np.array([[1.5, -2.25, 0.75]], f32), (300, 1)))
    if name.startswith("full/"):                       # full/<seed>/<flatten>: exactly 20 points about the origin
        _, seed, flat = name.split("/")
        rng = np.random.default_rng(900 + int(seed))
        p = rng.normal(size=(20, 3)) * np.array([1.0, 0.6, 0.3 * float(flat)])
        p = (p - p.mean(axis=0)) @ _rotation(950 + int(seed)).T
        return _frozen(p.astype(f32))
    if name.startswith("first/"):                      # first/<n>: the first n points of lidar + 35
        return _frozen(cloud("lidar+35")[:int(name[6:])])
    if name == "semantic":
        return _frozen(cloud("lidar+35")[:sum(SEMANTIC_SIZES)])
    if name == "dropped":
        p = cloud("lidar+35")[:2000].copy()
        rows = dropped_rows()
        bad = np.array([np.nan, np.inf, -np.inf], f32)
        for t, r in enumerate(rows):
            p[r, t % 3] = bad[(t // 3) % 3]
        return _frozen(p)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def dropped_rows():
    return _frozen(np.sort(np.random.default_rng(74).choice(2000, N_DROPPED, replace=False)))


@functools.lru_cache(maxsize=None)
def semantic_labels():
    """labels 1 .. len(SEMANTIC_SIZES) scattered over the cloud (so that every class's segment has to be gathered)"""
    lab = np.repeat(np.arange(1, len(SEMANTIC_SIZES) + 1), SEMANTIC_SIZES).astype(np.uint32)
    return _frozen(np.random.default_rng(75).permutation(lab))


def cases():
    out = [Case("every_k", "lidar+35", k, 1) for k in ALL_K]
    out += [Case("every_k", "lidar+35", k, 0) for k in FLAG0_K]
    out += [Case("rule", c, k, 1) for c in RULE_CLOUDS for k in RULE_K]
    out += [Case("scale", c, k, f) for c in SCALE_CLOUDS for k in (5, 20) for f in (1, 0)]
    out += [Case("full", f"full/{s}/{z:g}", 20, f) for s in FULL_SEEDS for z in FULL_FLATTEN for f in (1, 0)]
    out += [Case("short", f"first/{n}", k, 1) for n, k in SHORT]
    out += [Case("edge", f"first/{n}", 20, 1) for n in EDGE_N]
    return out


def case_id(c):
    return f"{c.family}-{c.cloud}-k{c.k}-flag{c.flag}"


# ---- the oracle's side ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_lists(name, k):
    """O.knn(p, p, k, kdtree=True): the lists every test asserts of the engine (caller indices, -1 tail when n < k)"""
    p = cloud(name)
    return _frozen(O.knn(p, p, k, kdtree=True)[0])


def jacobi_normals(A):
    """the oracle's Jacobi code (orc_sym3_svd_u) on given matrices: the last column of U"""
    return np.stack([O.sym3_svd_u(a)[0][:, 2] for a in A]) if len(A) else np.empty((0, 3))


@functools.lru_cache(maxsize=None)
def oracle_normals(name, k, flag=1):
    """the oracle's normals: orc_covariances under the flag (the only form the reference has); without it the oracle's
    Jacobi code on the restatement's matrices"""
    if flag:
        return _frozen(O.covariances(cloud(name), None, k, EPS, 0, kdtree=True)[1])
    return _frozen(jacobi_normals(reference(name, k, 0)[0]))


def semantic_classes():
    """(label, caller indices of its points, ascending) per class"""
    lab = semantic_labels()
    return [(int(l), np.nonzero(lab == l)[0]) for l in range(1, len(SEMANTIC_SIZES) + 1)]


def kept_rows():
    """the finite rows of the `dropped` cloud, ascending"""
    return np.nonzero(np.isfinite(cloud("dropped")).all(axis=1))[0]


def local_lists(rows, nn_rows, n_total):
    """caller-index lists of the points `rows` as indices into p[rows] (-1 stays; an index outside `rows` raises)"""
    inv = np.full(n_total + 1, -2, dtype=np.int64)
    inv[rows] = np.arange(len(rows))
    inv[-1] = -1                                     # nn == -1 reads the last slot
    out = inv[nn_rows]
    assert (out != -2).all(), "a neighbour outside the segment"
    return out.astype(np.int32)


@functools.lru_cache(maxsize=None)
def reference(name, k, flag):
    """(A, S) of the cloud on the oracle's lists"""
    A, S = ref.moments(cloud(name), oracle_lists(name, k), k, flag)
    return _frozen(A), _frozen(S)


# ---- the checks -------------------------------------------------------------------------------------------------------------------------
def figures(p, nn, k, flag, nrm, onrm=None):
    """dict(ratio, unit, same): the largest eigen-residual ratio and | |n| - 1 | of the normals nrm on the lists nn, and the
    number of rows whose normal has the oracle's bits up to sign (None without onrm)"""
    A, S = ref.moments(p, nn, k, flag)
    r = ref.ratio(A, S, nrm)
    out = dict(ratio=float(r.max()) if len(r) else 0.0, unit=float(ref.unit_error(nrm).max()) if len(r) else 0.0, same=None, rows=len(r),
               ratios=r)
    if onrm is not None:
        out["same"] = int((np.all(nrm == onrm, axis=1) | np.all(nrm == -onrm, axis=1)).sum())
    return out


def assert_normals(p, nn, k, flag, nrm, what, onrm=None, gamma=None):
    """every row: finite, unit length within 540 u, eigen-residual ratio within GAMMA.  Returns figures()."""
    gamma = GAMMA if gamma is None else gamma
    assert np.isfinite(nrm).all(), what
    f = figures(p, nn, k, flag, nrm, onrm)
    print(f"covariances: {what}: rows {f['rows']}  ratio {f['ratio']:.3f}  unit {f['unit']:.2e}  oracle-bits {f['same']}")
    assert f["unit"] <= ref.UNIT_BOUND, (what, f["unit"])
    bad = np.nonzero(~(f["ratios"] <= gamma))[0]
    assert bad.size == 0, (what, f"{bad.size} rows above {gamma}", bad[:5], f["ratios"][bad[:5]])
    return f


def assert_matrices(cov, nrm, eps, what):
    """the returned matrix, bit for bit from the returned normal"""
    want = ref.matrix_of_normal(nrm, eps)
    assert cov.shape == want.shape and np.array_equal(cov, want), (what, int((cov != want).any(axis=(1, 2)).sum()))
