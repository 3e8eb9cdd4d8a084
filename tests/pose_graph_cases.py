"""Seeded generators of pose-graph cases for tests/test_pose_graph_cpu.py and tests/test_gpu_pose_graph.py.  A graph is a dict:
poses [N, 7] (the initial ones), fixed [N] bool, ei / ej [M] int32, z [M, 7], omega [M, 6, 6], truth [N, 7] (where there is
one)."""
import numpy as np

import pose_graph_ref as R

SIGMA_T, SIGMA_R = 0.02, np.deg2rad(1.0)  # 2 cm and 1 degree per edge


def random_pose(rng, n=None, scale=3.0, angle=np.pi):
    shape = (6,) if n is None else (n, 6)
    xi = rng.normal(size=shape)
    xi[..., :3] *= scale
    w = xi[..., 3:]
    xi[..., 3:] = w / np.linalg.norm(w, axis=-1, keepdims=True) * rng.uniform(0, angle, size=shape[:-1] + (1,))
    return R.exp(xi)


def random_spd(rng, m, lo=1.0, hi=1e4):
    """anisotropic information matrices: random axes, eigenvalues log-uniform in [lo, hi]"""
    out = np.empty((m, 6, 6))
    for k in range(m):
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
        out[k] = (Q * np.exp(rng.uniform(np.log(lo), np.log(hi), size=6))) @ Q.T
    return 0.5 * (out + np.swapaxes(out, 1, 2))


def default_omega(m):
    return np.tile(np.diag([1 / SIGMA_T ** 2] * 3 + [1 / SIGMA_R ** 2] * 3), (m, 1, 1))


# the rotation angles of a residual: zero, tiny, both sides of the series threshold, mid-range and up to 3 rad
RESIDUAL_ANGLES = (0.0, 1e-12, 1e-6, 0.1, R.SERIES_THETA * (1 - 1e-9), R.SERIES_THETA, R.SERIES_THETA * (1 + 1e-9), 1.0, 2.0, 3.0)


def edge_cases(seed=0, per_angle=3):
    """single edges whose residual has a prescribed rotation angle: (Ti, Tj, z, omega, r_wanted), one row per case"""
    rng = np.random.default_rng(seed)
    rows = []
    for angle in RESIDUAL_ANGLES:
        for k in range(per_angle):
            r = rng.normal(size=6)
            r[3:] *= angle / np.linalg.norm(r[3:])
            if angle == 0.0 and k == 0:
                r[:] = 0.0  # |r| = 0
            Ti, z = random_pose(rng), random_pose(rng, scale=1.0)
            Tj = R.mul(R.mul(Ti, z), R.exp(r))
            rows.append((Ti, Tj, z, random_spd(rng, 1)[0], r))
    return tuple(np.array([row[k] for row in rows]) for k in range(5))


def edge_case_graph(seed=0):
    """the cases above as one graph: nodes 2k and 2k + 1 carry case k; node 0 is fixed"""
    Ti, Tj, z, omega, _ = edge_cases(seed)
    m = len(z)
    poses = np.empty((2 * m, 7))
    poses[0::2], poses[1::2] = Ti, Tj
    fixed = np.zeros(2 * m, dtype=bool)
    fixed[0] = True
    return dict(poses=poses, fixed=fixed, ei=np.arange(0, 2 * m, 2, dtype=np.int32), ej=np.arange(1, 2 * m, 2, dtype=np.int32), z=z, omega=omega)


def _measure(rng, truth, ei, ej, noise=True):
    z = R.mul(R.inverse(truth[ei]), truth[ej])
    if noise:
        d = rng.normal(size=(len(ei), 6)) * np.array([SIGMA_T] * 3 + [SIGMA_R] * 3)
        z = R.mul(z, R.exp(d))
    return z


def _integrate(truth, z_odo):
    poses = np.empty_like(truth)
    poses[0] = truth[0]
    for k in range(1, len(truth)):
        poses[k] = R.mul(poses[k - 1], z_odo[k - 1])
    return poses


def _circle(n, radius=10.0):
    a = 2 * np.pi * np.arange(n) / n
    xi = np.zeros((n, 6))
    xi[:, 5] = a + np.pi / 2
    T = R.exp(xi)
    T[:, 4], T[:, 5], T[:, 6] = radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(3 * a)
    return T


def ring(n=65, closures=1, seed=1, noise=True, outliers=0, omega=None):
    """n poses round a circle: odometry edges k -> k + 1, `closures` loop edges (the first joins the last node to node 0, the
    others random pairs), the last `outliers` of them grossly wrong.  Node 0 is fixed; the initial poses are integrated odometry."""
    rng = np.random.default_rng(seed)
    truth = _circle(n)
    ei = list(range(n - 1)) + [n - 1]
    ej = list(range(1, n)) + [0]
    for _ in range(closures - 1):
        a, b = rng.choice(n, size=2, replace=False)
        ei.append(int(a)); ej.append(int(b))
    ei, ej = np.array(ei, dtype=np.int32), np.array(ej, dtype=np.int32)
    z = _measure(rng, truth, ei, ej, noise)
    for k in range(len(ei) - outliers, len(ei)):
        z[k] = R.mul(z[k], R.exp(np.array([3.0, -2.0, 1.0, 0.3, -0.5, 0.8])))
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    om = default_omega(len(ei)) if omega is None else omega(rng, len(ei))
    return dict(poses=_integrate(truth, z[: n - 1]), fixed=fixed, ei=ei, ej=ej, z=z, omega=om, truth=truth)


def hub(spokes=120, seed=2, noise=True):
    """node 0 (fixed) with 300 incident edges: every spoke twice (a duplicate edge), half of them given as (j, i), plus a rim"""
    rng = np.random.default_rng(seed)
    n = spokes + 1
    truth = np.concatenate([R.exp(np.zeros((1, 6))), random_pose(rng, spokes, scale=5.0)])
    ei, ej = [], []
    for k in range(1, n):
        for rep in range(2):
            a, b = (0, k) if (k + rep) % 2 == 0 else (k, 0)
            ei.append(a); ej.append(b)
    for k in range(1, spokes // 2 + 1):  # 60 more edges at node 0, and a rim among the spokes
        ei.append(k); ej.append(0)
    for k in range(1, n - 1):
        ei.append(k); ej.append(k + 1)
    ei, ej = np.array(ei, dtype=np.int32), np.array(ej, dtype=np.int32)
    z = _measure(rng, truth, ei, ej, noise)
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    poses = R.mul(truth, R.exp(rng.normal(size=(n, 6)) * 0.05))
    poses[0] = truth[0]
    return dict(poses=poses, fixed=fixed, ei=ei, ej=ej, z=z, omega=default_omega(len(ei)), truth=truth)


def counted(m, n=130, seed=3):
    """m random edges on n nodes with anisotropic information; node 7 fixed, the poses off the truth"""
    rng = np.random.default_rng(seed + m)
    truth = random_pose(rng, n)
    ei = rng.integers(0, n, size=m).astype(np.int32)
    ej = ((ei + rng.integers(1, n, size=m)) % n).astype(np.int32)
    z = _measure(rng, truth, ei, ej)
    fixed = np.zeros(n, dtype=bool)
    fixed[7] = True
    return dict(poses=R.mul(truth, R.exp(rng.normal(size=(n, 6)) * 0.1)), fixed=fixed, ei=ei, ej=ej, z=z, omega=random_spd(rng, m), truth=truth)


def chain(n=9, seed=4, fixed_at=4, isolated=1):
    """a chain with a fixed node in the middle and `isolated` nodes without edges at the end"""
    rng = np.random.default_rng(seed)
    truth = random_pose(rng, n + isolated)
    ei, ej = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    z = _measure(rng, truth, ei, ej)
    fixed = np.zeros(n + isolated, dtype=bool)
    fixed[fixed_at] = True
    return dict(poses=R.mul(truth, R.exp(rng.normal(size=(n + isolated, 6)) * 0.05)), fixed=fixed, ei=ei, ej=ej, z=z,
                omega=random_spd(rng, n - 1), truth=truth)


def two_nodes(seed=5):
    g = chain(2, seed, fixed_at=0, isolated=0)
    return g


def triangle(seed=6):
    rng = np.random.default_rng(seed)
    truth = random_pose(rng, 3)
    ei, ej = np.array([0, 1, 2], dtype=np.int32), np.array([1, 2, 0], dtype=np.int32)
    fixed = np.array([False, True, False])
    return dict(poses=R.mul(truth, R.exp(rng.normal(size=(3, 6)) * 0.1)), fixed=fixed, ei=ei, ej=ej, z=_measure(rng, truth, ei, ej),
                omega=random_spd(rng, 3), truth=truth)


def grid_world(side=10, n_closures=1000, seed=7):
    """a boustrophedon walk through a side^3 grid (about 1000 nodes): odometry along the walk plus closures between grid
    neighbours that the walk does not join; 2 cm / 1 degree per edge, the initial poses from integrated odometry"""
    rng = np.random.default_rng(seed)
    cells = []
    for zc in range(side):
        plane = []
        for yc in range(side):
            row = [(xc, yc, zc) for xc in range(side)]
            plane += row if yc % 2 == 0 else row[::-1]
        cells += plane if zc % 2 == 0 else plane[::-1]
    cells = np.array(cells, dtype=float)
    n = len(cells)
    xi = np.zeros((n, 6))
    xi[:, 3:] = rng.normal(size=(n, 3)) * 0.3
    truth = R.exp(xi)
    truth[:, 4:] = cells * 2.0
    index = {tuple(c): k for k, c in enumerate(cells.astype(int))}
    pairs = []
    for k, c in enumerate(cells.astype(int)):
        for d in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            o = index.get((c[0] + d[0], c[1] + d[1], c[2] + d[2]))
            if o is not None and abs(o - k) > 1:
                pairs.append((min(k, o), max(k, o)))
    pairs = np.array(pairs)[rng.choice(len(pairs), size=n_closures, replace=False)]
    ei = np.concatenate([np.arange(n - 1), pairs[:, 1]]).astype(np.int32)
    ej = np.concatenate([np.arange(1, n), pairs[:, 0]]).astype(np.int32)
    z = _measure(rng, truth, ei, ej)
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    return dict(poses=_integrate(truth, z[: n - 1]), fixed=fixed, ei=ei, ej=ej, z=z, omega=default_omega(len(ei)), truth=truth)


def step_control(seed=8):
    """a 12-node ring whose closure measurement is off by a rotation of 2.95 rad: at the initial poses (integrated odometry)
    the closure's residual rotates by about 3 rad, and with initial_radius = 1e16 the first full step overshoots"""
    g = ring(n=12, closures=1, seed=seed)
    xi = np.zeros(6)
    xi[3:] = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0]) * 2.95
    g["z"][-1] = R.mul(g["z"][-1], R.exp(xi))
    return g


# ---- the comparison of per-edge outputs with the restatement, shared by the CPU and the GPU tests ---------------------------------
BLOCKS = ("r", "s", "w", "rho", "Hi", "Hj", "B", "gi", "gj")


def restated(Ti, Tj, z, omega, kind, a, dtype=np.float64):
    m = len(z)
    poses = np.concatenate([Ti, Tj]).astype(dtype)
    ei, ej = np.arange(m), np.arange(m, 2 * m)
    return R.edges(poses, ei, ej, z.astype(dtype), omega.astype(dtype), kind, a)


def floors(Ti, Tj, z, omega):
    """Per edge, the size of the quantities a block is formed from.  A residual near zero comes out of a product of poses with
    entries of size one (and translations of their own size): its rounding error is relative to those, not to itself, and so are
    the errors of what is built on it.  The blocks of the normal equations need no floor (the Jacobians are of size one)."""
    size = np.maximum(1.0, np.max(np.abs(np.concatenate([Ti[:, 4:], Tj[:, 4:], z[:, 4:]], axis=1)).astype(np.float64), axis=1))
    om = np.abs(omega).reshape(len(z), -1).max(axis=1).astype(np.float64)
    return {"r": size, "s": om * size ** 2, "rho": om * size ** 2, "w": 1.0 + 0 * size, "gi": om * size, "gj": om * size,
            "Hi": 0 * size, "Hj": 0 * size, "B": 0 * size}


def relative_gap(A, B, floor=0.0):
    """per edge: the largest difference of a block relative to the block's largest magnitude (or its floor, see floors())"""
    A, B = np.asarray(A), np.asarray(B)
    m = len(A)
    d = np.abs(A - B).reshape(m, -1).max(axis=1).astype(np.float64)
    scale = np.maximum(np.abs(B).reshape(m, -1).max(axis=1).astype(np.float64), floor)
    return d / np.maximum(scale, np.finfo(np.float64).tiny)


def rounding_noise(Ti, Tj, z, omega, kind, a):
    """the restatement's own float64 noise: against np.longdouble on the same cases"""
    E64, E80 = restated(Ti, Tj, z, omega, kind, a), restated(Ti, Tj, z, omega, kind, a, np.longdouble)
    F = floors(Ti, Tj, z, omega)
    return max(float(relative_gap(E64[k], E80[k], F[k]).max()) for k in BLOCKS)


def header_tolerance():
    """32 x the restatement's rounding noise on the edge cases (the margin: libm's few-ulp sin / cos / atan against an
    extended-precision evaluation)"""
    Ti, Tj, z, omega, _ = edge_cases()
    noise = max(rounding_noise(Ti, Tj, z, omega, kind, 1.5) for kind in (R.LOSS_NONE, R.LOSS_CAUCHY))
    tol = 32 * noise
    return noise, tol
