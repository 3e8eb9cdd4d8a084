"""Inputs of tests/test_wrap_cases_cpu.py and tests/test_gpu_launch_wraps.py: clouds at the size where four modules' launches
change what they do.  The per-point kernels of the camera and of the range image run at most MAX_GROUPS workgroups of GROUP
lanes, so with more than N0 = GROUP MAX_GROUPS *finite* points some workgroups take a second pass of their stride loop; the
tree sums of the planes and of the filter reduce TREE_RUN caller indices per workgroup, level over level, so with more than
N0 = TREE_RUN TREE_RUN *caller* indices the tree has a third level.  Every family comes at three sizes: N0 (the last one
without), N0 + 1 (one lane of one wave in the second pass; a second-level run of one entry) and N0 + 3 workgroups + 77 (several
workgroups wrap, the last one a partial wave or a partial run).

Camera and range: every point is live (the per-point work is cheap), the images are small, and the last TAIL points are placed
by hand -- TAIL_PIXELS chosen pixels, each visited TAIL / TAIL_PIXELS times at falling depth, all nearer than anything before
them -- so the winners of those pixels are the cloud's last points: the second pass' at the two larger sizes.  NAN_ROWS rows
that are not finite sit between the others; the sizes count the finite points, which is what the launches see.

Planes and filter: the trees run over the caller's indices whether a point is alive or not, so the clouds are stretches of NaN
rows and of points masked out, with the live points of plane_cases._scene -- about 3 000 -- at chosen indices.

Two small things of the same kind: lattices through the origin in the planes y = 0, x = 0 and x = y (plane_orient's ny and nx
branches), and one grid cell of more than PAIR_CHUNK PAIR_CHUNK_GROUPS points whose second label sits on the late points only."""
import functools

import numpy as np

import camera_cases
import camera_ref
import cluster_cases
import cluster_ref
import filter_cases
import filter_ref
import plane_cases
import plane_ref
import range_cases
import range_ref

F = np.float32
N0 = camera_ref.GROUP * camera_ref.MAX_GROUPS
SIZES = ("last_without", "plus_one", "several")
POINT_SIZES = {"last_without": N0, "plus_one": N0 + 1, "several": N0 + 3 * camera_ref.GROUP + 77}
TREE_SIZES = {"last_without": N0, "plus_one": N0 + 1, "several": N0 + 3 * plane_ref.TREE_RUN + 77}
TREE_LEVELS = {"last_without": 2, "plus_one": 3, "several": 3}
TAIL, TAIL_PIXELS, NAN_ROWS = 1000, 200, 1200
MIN_TAIL_WINNERS = 150


def _with_rows_that_are_not_finite(xyz, lab, seed):
    """NAN_ROWS rows (every fifth of them with one infinite coordinate only) put between the rows before the tail"""
    rng = np.random.default_rng(seed)
    at = np.sort(rng.choice(len(xyz) - TAIL, NAN_ROWS, replace=False))
    bad = np.full((NAN_ROWS, 3), np.nan, F)
    bad[::5] = [1.0, np.inf, 2.0]
    return np.insert(xyz, at, bad, axis=0), np.insert(lab, at, rng.integers(1, 10, NAN_ROWS).astype(np.uint32))


# ---- camera ---------------------------------------------------------------------------------------------------------------------
CAMERA_P = dict(camera_cases.intrinsics(64, 48), max_depth=25.0, **camera_cases.LENS)
CAMERA_WINDOWS = (1, 5)


def _camera_tail(p, qt, seed):
    """TAIL points through the centres of TAIL_PIXELS pixels, depths falling from 0.9 to 0.4 (the cloud before them begins at 1)"""
    q = camera_ref.params(**p)
    rng = np.random.default_rng(seed)
    pix = np.sort(rng.choice(q.width * q.height, TAIL_PIXELS, replace=False))[np.arange(TAIL) % TAIL_PIXELS]
    xd, yd = (pix % q.width - q.cx) / q.fx, (pix // q.width - q.cy) / q.fy
    x, y = xd, yd
    for _ in range(30):  # the distortion undone: the fixed point of rule 12
        _, rad, tx, ty = camera_ref._distortion(q, x, y)
        x, y = (xd - tx) / rad, (yd - ty) / rad
    Z = 0.9 - 0.5 * np.arange(TAIL) / TAIL
    m = camera_ref.matrices(qt)["cam_to_cloud"]
    return (np.stack([x * Z, y * Z, Z], axis=1) @ m[:, :3].T + m[:, 3]).astype(F), rng.integers(1, 10, TAIL).astype(np.uint32), pix


@functools.lru_cache(maxsize=None)
def camera_case(size):
    """a camera_cases case of POINT_SIZES[size] finite points and NAN_ROWS others; "tail_pixels": the pixels of the tail"""
    n = POINT_SIZES[size]
    body, lab = camera_cases.cloud(n - TAIL, 7 + n, CAMERA_P, camera_cases.QT, z_lo=1.0)
    tail, tail_lab, pix = _camera_tail(CAMERA_P, camera_cases.QT, 8 + n)
    xyz, lab = _with_rows_that_are_not_finite(np.concatenate([body, tail]), np.concatenate([lab, tail_lab]), 9 + n)
    c = camera_cases.case(xyz, lab, camera_cases.QT, seed=n, **CAMERA_P)
    c["tail_pixels"] = np.unique(pix)
    return c


@functools.lru_cache(maxsize=None)
def camera_reference(size, window):
    """camera_ref.labels (its "image" is camera_ref.image) with the restatement's own matrices"""
    c = camera_case(size)
    return camera_ref.labels(c["xyz"], c["labels"], c["pixel_label"], camera_ref.params(**dict(c["p"], window=window)), camera_ref.matrices(c["qt"]))


# ---- range ----------------------------------------------------------------------------------------------------------------------
RANGE_ORIGIN = (1.5, -2.0, 0.5)
RANGE_P = dict(width=64, height=8, clockwise=1, min_range=0.5, max_range=40.0, window=3, k=5, max_dist_sq=9.0)


def _range_tail(p, seed):
    """TAIL points through the middles of TAIL_PIXELS (row, sector) pairs, ranges falling from 1.5 to 0.6 (the cloud before them
    begins at 2)"""
    q = range_ref.params(**p)
    W, H = q.width, q.height
    rng = np.random.default_rng(seed)
    cell = np.sort(rng.choice(W * H, TAIL_PIXELS, replace=False))[np.arange(TAIL) % TAIL_PIXELS]
    a = range_ref.edge_angles(q)
    el = (0.5 * (a[:-1] + a[1:]))[cell // W]
    az = 2.0 * np.pi * (cell % W + 0.5) / W
    r = 1.5 - 0.9 * np.arange(TAIL) / TAIL
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1) + np.asarray(RANGE_ORIGIN)
    return xyz.astype(F), rng.integers(1, 10, TAIL).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def range_case(size):
    """a range_cases case of POINT_SIZES[size] finite points and NAN_ROWS others, with "pixel_label" """
    n = POINT_SIZES[size]
    body, lab = range_cases.sphere(n - TAIL, 17 + n, r_lo=2.0, origin=RANGE_ORIGIN)
    tail, tail_lab = _range_tail(RANGE_P, 18 + n)
    xyz, lab = _with_rows_that_are_not_finite(np.concatenate([body, tail]), np.concatenate([lab, tail_lab]), 19 + n)
    c = range_cases.case(xyz, lab, origin=RANGE_ORIGIN, **RANGE_P)
    c["pixel_label"] = np.random.default_rng(20 + n).integers(0, 4, (RANGE_P["height"], RANGE_P["width"])).astype(np.uint32)
    return c


@functools.lru_cache(maxsize=None)
def range_reference(size):
    """range_ref.vote (its "image" is range_ref.image) with the restatement's own tables"""
    c = range_case(size)
    p = range_ref.params(**c["p"])
    return range_ref.vote(c["xyz"], c["labels"], c["pixel_label"], p, range_ref.tables(p), c["origin"])


def finite_position(xyz):
    """per caller index the position f among the finite points (what the launches index by), -1 for a row that is not finite"""
    ok = np.isfinite(np.asarray(xyz, F).reshape(-1, 3)).all(axis=1)
    return np.where(ok, np.cumsum(ok) - 1, -1)


# ---- planes and filter ----------------------------------------------------------------------------------------------------------
STRETCH = 4096  # dead caller indices alternate between NaN rows and masked-out points in stretches of this length
PLANE_T = 0.05


def live_indices(n):
    """0 .. 599, a stretch over 511 | 512, one over N0 - 1 | N0, the last 300, every 997th and every 151st index between: three or
    four live points in every run of the first level"""
    run = plane_ref.TREE_RUN
    parts = [np.arange(0, 600), np.arange(run - 40, run + 40), np.arange(N0 - 150, N0 + 150), np.arange(n - 300, n), np.arange(600, n, 997), np.arange(600, n, 151)]
    live = np.unique(np.concatenate(parts))
    return live[live < n]


def must_be_members(n):
    """caller indices that hold a point of the plane, unmasked: either side of the first run's end, either side of N0, the last"""
    run = plane_ref.TREE_RUN
    return [i for i in (run - 1, run, N0 - 1, N0, n - 1) if i < n]


@functools.lru_cache(maxsize=None)
def tree_cloud(size):
    """(xyz, labels, mask) over TREE_SIZES[size] caller indices"""
    n = TREE_SIZES[size]
    rng = np.random.default_rng(50 + n)
    live = live_indices(n)
    sx, sl = plane_cases._scene(51 + n % 89, len(live))
    resid = np.abs(sx[:, 2].astype(np.float64) - (0.3 * sx[:, 0].astype(np.float64) - 0.1 * sx[:, 1].astype(np.float64) + 1.0))
    want = [int(np.searchsorted(live, i)) for i in must_be_members(n)]
    spare = [int(k) for k in np.flatnonzero((sl == 1) & (resid < 0.01)) if int(k) not in want]
    for k in want:  # a point near the middle of the plane's noise at each of these
        g = spare.pop()
        sx[[k, g]], sl[[k, g]] = sx[[g, k]], sl[[g, k]]
    xyz = rng.uniform(-5, 5, (n, 3)).astype(F)
    lab = (1 + rng.integers(0, 3, n)).astype(np.uint32)
    mask = np.ones(n, np.uint8)
    nan_stretch = (np.arange(n) // STRETCH) % 2 == 0
    xyz[nan_stretch] = np.nan
    mask[~nan_stretch] = 0
    xyz[live], lab[live], mask[live] = sx, sl, 1
    holes = np.setdiff1d(live[5::11], must_be_members(n))  # (filter_cases._tree's holes among the live points, and its NaN)
    mask[holes] = 0
    xyz[7] = np.nan
    return xyz, lab, mask


@functools.lru_cache(maxsize=None)
def plane_case(size):
    """refine = 1: the x y z e e tree and the products' tree both run; H = HYP_GROUP + 1; the second round's trees run with most
    members gone"""
    xyz, lab, mask = tree_cloud(size)
    p = plane_cases._params(distance_threshold=PLANE_T, num_hypotheses=plane_ref.HYP_GROUP + 1, max_planes=2, min_inliers=5, refine=1)
    return plane_cases._case(xyz, lab, p, mask)


@functools.lru_cache(maxsize=None)
def plane_reference(size):
    c = plane_case(size)
    return plane_ref.segment_planes(c["xyz"], c["labels"], c["mask"], **c["params"])


@functools.lru_cache(maxsize=None)
def filter_case(size):
    """filter_cases._tree's parameters on the tree cloud"""
    xyz, lab, mask = tree_cloud(size)
    return filter_cases._case(xyz, lab, filter_cases._params(mean_k=6, std_mul=1.5, drop=(3,), protect=(2,)), mask)


@functools.lru_cache(maxsize=None)
def filter_reference(size):
    c = filter_case(size)
    return filter_ref.filter(c["xyz"], c["labels"], c["mask"], **c["params"])


# ---- plane_orient ---------------------------------------------------------------------------------------------------------------
ORIENT = {"lattice_y0": (0.0, 1.0, 0.0, 0.0), "lattice_x0": (1.0, 0.0, 0.0, 0.0),  # the coefficients by hand
          "lattice_xy": (-np.sqrt(0.5), np.sqrt(0.5), 0.0, 0.0)}                  # (these two to a rounding of the unit normal)


@functools.lru_cache(maxsize=None)
def orient_case(name):
    """plane_cases._lattice_ties moved into the plane y = 0 or x = 0, the origin one of its points: d = 0 and nz = 0, so the sign
    is decided by ny, or -- ny = 0 too -- by nx.  In the plane x = y, which holds the z axis, nx and ny are both there with
    opposite signs: ny decides, and a rule that asked nx first would give the other sign.  (d = -(n . a) is a zero whose sign the
    negation and the flip leave as they find it; the order of the columns is the one that ends at +0.0, the mirrored lattice
    ends at -0.0.)"""
    g = np.arange(6, dtype=F) - F(2)
    u, v = np.meshgrid(g, g, indexing="ij")
    zero = np.zeros(36, F)
    cols = {"lattice_y0": [u.ravel(), zero, v.ravel()], "lattice_x0": [zero, v.ravel(), u.ravel()], "lattice_xy": [u.ravel(), u.ravel(), v.ravel()]}[name]
    return plane_cases._case(np.stack(cols, axis=1), None, plane_cases._params(num_hypotheses=200, min_inliers=3, refine=0))


def orient_by_hand(name, coeff):
    """the coefficients written by hand: exactly where they are 0 and 1; within 2^-52 -- n / |n| and sqrt(1 / 2) are each rounded
    once -- and with the hand's signs otherwise; d = +0.0"""
    want, got = np.array(ORIENT[name]), np.asarray(coeff, np.float64).reshape(4)
    exact = want == np.round(want)
    return bool((got[exact] == want[exact]).all() and (np.abs(got - want) <= 2.0 ** -52).all() and
                (np.sign(got[~exact]) == np.sign(want[~exact])).all() and not np.signbit(got[3]))


@functools.lru_cache(maxsize=None)
def orient_reference(name):
    c = orient_case(name)
    return plane_ref.segment_planes(c["xyz"], c["labels"], c["mask"], **c["params"])


def orient_branch(coeff, axis):
    """the branch of rules 4 / 5 that fixed a plane's sign, from its coefficients (a flip changes no magnitude)"""
    c = [float(v) for v in coeff]
    if axis is not None and any(float(v) != 0.0 for v in axis):
        if (c[0] * float(axis[0]) + c[1] * float(axis[1])) + c[2] * float(axis[2]) != 0.0:
            return "axis"
    return next((name for name, v in zip(("d", "nz", "ny", "nx"), (c[3], c[2], c[1], c[0])) if v != 0.0), "nx")


# ---- one cell of more than PAIR_CHUNK PAIR_CHUNK_GROUPS points ------------------------------------------------------------------
CELL_STEP = cluster_ref.PAIR_CHUNK * cluster_ref.PAIR_CHUNK_GROUPS
ONE_CELL_N = 4100
ONE_CELL_FIRST_LABEL = CELL_STEP + 100  # points before this index have label 1, the others label 2


def fullest_cell(xyz, tolerance):
    """the number of points in the fullest cell of the search grid"""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    cells = cluster_ref.cell_coords(xyz[np.isfinite(xyz).all(axis=1)], tolerance)
    return int(np.unique(cells, axis=0, return_counts=True)[1].max())


@functools.lru_cache(maxsize=None)
def one_cell_case():
    """ONE_CELL_N points in a ball of radius 0.2 T about the middle of a cell.  A cell's points keep the caller's order, so
    label 2 lies on points that only a workgroup's second step takes: no first step joins two of them"""
    T = cluster_cases.T
    rng = np.random.default_rng(27)
    d = rng.normal(size=(ONE_CELL_N, 3))
    d *= (0.2 * T * rng.uniform(0, 1, ONE_CELL_N) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
    edge = 1.0 / float(cluster_ref.grid_inv(T))
    centre = (np.array([20.0, -9.0, 1.0]) + 0.5) * edge
    lab = np.where(np.arange(ONE_CELL_N) < ONE_CELL_FIRST_LABEL, 1, 2).astype(np.uint32)
    return {"xyz": (centre + d).astype(F), "labels": lab, "params": cluster_cases._params(min_points=1, same_label=1)}


@functools.lru_cache(maxsize=None)
def one_cell_cluster_reference():
    c = one_cell_case()
    return cluster_ref.cluster(c["xyz"], c["labels"], **c["params"])


@functools.lru_cache(maxsize=None)
def one_cell_filter_case():
    c = one_cell_case()
    return filter_cases._case(c["xyz"], c["labels"], filter_cases._params(mean_k=0, radius=cluster_cases.T, min_neighbors=2))


@functools.lru_cache(maxsize=None)
def one_cell_filter_reference():
    c = one_cell_filter_case()
    return filter_ref.filter(c["xyz"], c["labels"], c["mask"], **c["params"])
