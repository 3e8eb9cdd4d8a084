"""Inputs of the distance-field tests (tests/test_distance_cpu.py on the restatement, tests/test_gpu_distance.py through the
library): hand-built map states -- get_state() dicts -- with a window and params each, the smallest shapes at which the kernels
of sicp_map_distance can go wrong, and naive(): the header's rules once more, every obstacle against every cell of its ball in
plain loops over the obstacles, written from include/sicp.h and not from tests/distance_ref.py.

CASES            name -> a function giving {"state", "center", "shape" (nx, ny, nz), "params" (distance_ref.defaults), "points"
                 ([n, 3] float32 or None), "point_labels", "qt", "expect" (a function of the result that asserts what the case is
                 named for)}
case(name)       that dict, built once and read-only
reference(name)  the restatement's answer, computed once and read-only
The states use leaf 0.5 (inv_leaf = 2 exactly).  A result's arrays are indexed [k, j, i]; the window's cell (i, j, k) is the voxel
(x0 + i, y0 + j, z0 + k)."""
from __future__ import annotations

import functools
import math

import numpy as np

import distance_ref as ref
import np_ref
from elevation_cases import CLASSES, LEAF, make_state, patch_state, pose

BIAS = 1 << 20
EDGE = BIAS - 1  # the largest |voxel coordinate| the key holds


def centre_of(vx, vy, vz, leaf=LEAF):
    """a centre inside the voxel (vx, vy, vz)"""
    return ((vx + 0.5) * leaf, (vy + 0.5) * leaf, (vz + 0.5) * leaf)


def centred(shape, corner=(0, 0, 0)):
    """the centre that puts the window's cell (0, 0, 0) on the voxel `corner`"""
    return centre_of(*(c + n // 2 for c, n in zip(corner, shape)))


def row_of(state, v):
    """the map row of voxel v"""
    key = ((v[2] + BIAS) << 42) | ((v[1] + BIAS) << 21) | (v[0] + BIAS)
    r = int(np.searchsorted(state["key"], np.uint64(key)))
    assert int(state["key"][r]) == key
    return r


def _case(state, center, shape, points=None, point_labels=None, qt=None, expect=None, **params):
    nx, ny, nz = shape
    return dict(state=state, center=tuple(float(c) for c in center), shape=(nx, ny, nz), params=ref.defaults(nx=nx, ny=ny, nz=nz, **params),
                points=points, point_labels=point_labels, qt=qt, expect=expect if expect is not None else (lambda out: None))


def _random_voxels(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return np.unique(np.stack([rng.integers(lo[a], hi[a], n) for a in range(3)], axis=1), axis=0)


# ---- shapes -------------------------------------------------------------------------------------------------------------------
def _one_cell(occupied):
    st = make_state([(4, -2, 7), (5, -2, 7)], seed=30)
    at = (4, -2, 7) if occupied else (3, -2, 7)  # one voxel beside the obstacle: outside the window, so it does not exist
    def expect(out):
        assert out["dist_sq"].shape == (1, 1, 1)
        if occupied:
            assert out["dist_sq"].item() == 0 and out["nearest"].item() == 0 and out["info"]["n_obstacles"] == 1
        else:
            assert out["dist_sq"].item() == -1 and out["nearest"].item() == -1 and out["info"]["max_dist_sq"] == -1
    return _case(st, centre_of(*at), (1, 1, 1), max_dist_voxels=3, expect=expect)


def _shape(seed, shape, n, R):
    """random voxels over the window and a margin of R around it"""
    v = _random_voxels(seed, n, (-R, -R, -R), tuple(s + R for s in shape))
    def expect(out):
        d = out["dist_sq"]
        assert d.shape == shape[::-1] and (d == 0).sum() == out["info"]["n_obstacles"] > 0
        assert (d < 0).any() and out["info"]["max_dist_sq"] > (R - 1) * (R - 1)
    return _case(make_state(v, seed=seed + 1), centred(shape), shape, max_dist_voxels=R, expect=expect)


def _long_line():
    """1024 x 4 x 2 at R = 64: lines longer than any tile plus its halo; one obstacle stands alone, 200 cells from the next"""
    v = [(100, 1, 0), (300, 2, 1), (363, 0, 0), (364, 3, 1), (700, 1, 1), (1023, 0, 0), (0, 3, 1), (511, 2, 0), (512, 1, 1), (255, 0, 1),
         (256, 3, 0), (830, 2, 0)]
    st = make_state(v, seed=32)
    def expect(out):
        d, near = out["dist_sq"], out["nearest"]
        assert d[0, 1, 100 + 64] == 64 * 64 and near[0, 1, 164] == row_of(st, (100, 1, 0)) and d[0, 1, 165] == -1  # R itself, and one past
        assert out["info"]["max_dist_sq"] == 64 * 64 and (d < 0).any() and (d > 60 * 60).any()
    return _case(st, centred((1024, 4, 2)), (1024, 4, 2), max_dist_voxels=64, expect=expect)


def _r_larger_than_window():
    st = make_state([(0, 0, 0), (4, 3, 2), (9, 9, 9)], seed=33)
    def expect(out):
        assert (out["dist_sq"] >= 0).all() and out["info"]["n_obstacles"] == 2 and 0 < out["info"]["max_dist_sq"] < 64
        assert set(out["nearest"].reshape(-1).tolist()) == {0, 1}
    return _case(st, centred((5, 4, 3)), (5, 4, 3), max_dist_voxels=64, expect=expect)


def _r1():
    v = _random_voxels(34, 40, (0, 0, 0), (9, 9, 5))
    def expect(out):
        d = out["dist_sq"]
        assert set(d.reshape(-1).tolist()) == {-1, 0, 1}
    return _case(make_state(v, seed=35), centred((9, 9, 5)), (9, 9, 5), max_dist_voxels=1, expect=expect)


# ---- the ball ------------------------------------------------------------------------------------------------------------------
BALL_A, BALL_B = (5, 5, 1), (20, 5, 1)


def _ball_not_cube():
    st = make_state([BALL_A, BALL_B], label=[2, 3], count=2, frac=0.5)
    def expect(out):
        d, near = out["dist_sq"], out["nearest"]
        assert d[1, 9, 8] == 25 and near[1, 9, 8] == 0 and out["label"][1, 9, 8] == 2  # A + (3, 4, 0)
        assert d[1, 6, 25] == -1 and near[1, 6, 25] == -1 and out["label"][1, 6, 25] == 0  # B + (5, 1, 0): in the cube, not in the ball
        assert d[1, 5, 25] == 25 and d[1, 6, 24] == 17 and out["info"]["max_dist_sq"] == 25
    return _case(st, centred((30, 12, 3)), (30, 12, 3), max_dist_voxels=5, expect=expect)


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def _tie_midway():
    """three pairs with a cell midway: along x, along y, and a diagonal pair whose smaller row lies towards +x"""
    v = [(2, 3, 1), (8, 3, 1), (15, 1, 1), (15, 7, 1), (28, 2, 1), (22, 6, 1)]
    st = make_state(v, seed=36)
    def expect(out):
        d, near = out["dist_sq"], out["nearest"]
        assert d[1, 3, 5] == 9 and near[1, 3, 5] == row_of(st, (2, 3, 1)) < row_of(st, (8, 3, 1))
        assert d[1, 4, 15] == 9 and near[1, 4, 15] == row_of(st, (15, 1, 1)) < row_of(st, (15, 7, 1))
        assert d[1, 4, 25] == 13 and near[1, 4, 25] == row_of(st, (28, 2, 1)) < row_of(st, (22, 6, 1))
    return _case(st, centred((32, 9, 3)), (32, 9, 3), max_dist_voxels=6, expect=expect)


TIE_AXES_CELL = (4, 5, 2)


def _tie_axes():
    """equal d^2 = 9 along the three axes from one cell: the smallest row is the one along -y"""
    c = TIE_AXES_CELL
    v = [(c[0] + 3, c[1], c[2]), (c[0], c[1] - 3, c[2]), (c[0], c[1], c[2] + 3)]
    st = make_state(v, label=[1, 2, 3], count=1, frac=0.5)
    def expect(out):
        assert out["dist_sq"][c[2], c[1], c[0]] == 9 and out["nearest"][c[2], c[1], c[0]] == 0 == row_of(st, v[1])
        assert out["label"][c[2], c[1], c[0]] == 2
    return _case(st, centred((9, 9, 7)), (9, 9, 7), max_dist_voxels=4, expect=expect)


def _tie_decompositions():
    """25 = 5^2 + 0 = 3^2 + 4^2: at the first cell the (5, 0, 0) obstacle is the smaller row, at the second the (3, -4, 0) one"""
    a, b = (3, 6, 1), (18, 6, 1)
    v = [(a[0] + 5, a[1], 1), (a[0] + 3, a[1] + 4, 1), (b[0] + 5, b[1], 1), (b[0] + 3, b[1] - 4, 1)]
    st = make_state(v, seed=37)
    def expect(out):
        d, near = out["dist_sq"], out["nearest"]
        assert d[1, a[1], a[0]] == 25 and near[1, a[1], a[0]] == row_of(st, v[0]) < row_of(st, v[1])
        assert d[1, b[1], b[0]] == 25 and near[1, b[1], b[0]] == row_of(st, v[3]) < row_of(st, v[2])
    return _case(st, centred((28, 12, 3)), (28, 12, 3), max_dist_voxels=5, expect=expect)


# ---- the window's faces -------------------------------------------------------------------------------------------------------
def _faces():
    nx, ny, nz = 9, 7, 5
    v = [(x, y, z) for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)]            # corners
    v += [(4, 0, 0), (0, 3, nz - 1), (nx - 1, ny - 1, 2)]                                       # edges
    v += [(4, 3, 0), (4, 3, nz - 1), (0, 3, 2), (nx - 1, 3, 2), (4, 0, 2), (4, ny - 1, 2)]      # faces
    def expect(out):
        assert out["info"]["n_obstacles"] == 17 and (out["dist_sq"] >= 0).all() and out["dist_sq"][2, 3, 4] == 4
    return _case(make_state(v, seed=38), centred((nx, ny, nz)), (nx, ny, nz), max_dist_voxels=3, expect=expect)


def _outside_within_r():
    """an obstacle one voxel outside every face, within R of inside cells, and one inside: only the inside one exists"""
    n = 8
    v = [(-1, 3, 2), (n, 3, 2), (3, -1, 2), (3, n, 2), (3, 3, -1), (3, 3, 4), (7, 7, 3)]
    st = make_state(v, seed=39)
    def expect(out):
        d = out["dist_sq"]
        assert out["info"]["n_obstacles"] == 1 and out["info"]["n_voxels"] == 7
        assert d[2, 3, 0] == -1 and d[0, 3, 3] == -1 and d[3, 3, 3] == -1 and d[2, 0, 3] == -1  # the cells beside the outside ones
        assert d[3, 7, 7] == 0 and set(out["nearest"].reshape(-1).tolist()) == {-1, row_of(st, (7, 7, 3))}
    return _case(st, centred((n, n, 4)), (n, n, 4), max_dist_voxels=4, expect=expect)


def _key_range(sign):
    """a window that reaches past the key's range: x cells at +-2^20 and beyond hold no voxel, the voxel at +-(2^20 - 1) counts"""
    v = [(sign * EDGE, 0, 0), (sign * (EDGE - 3), 1, 0)]
    st = make_state(v, seed=40)
    centre = centre_of(sign * (EDGE - 2), 0, 0)
    def expect(out):
        x0 = out["info"]["x0"]
        assert x0 == sign * (EDGE - 2) - 4 and (x0 + 7 > EDGE or x0 < -EDGE)
        d = out["dist_sq"]
        assert d[1, 1, sign * EDGE - x0] == 0 and out["info"]["n_obstacles"] == 2 and (d >= 0).all()
        beyond = (sign * (EDGE + 1)) - x0
        assert 0 <= beyond < 8 and d[1, 1, beyond] == 1  # no voxel there, but a cell of the field all the same
    return _case(st, centre, (8, 3, 3), max_dist_voxels=8, expect=expect)


# ---- selection -----------------------------------------------------------------------------------------------------------------
def _min_count(min_count):
    st = make_state([(1, 1, 1), (4, 1, 1), (7, 1, 1)], count=[1, 3, 5], label=1, frac=0.5)
    def expect(out):
        assert out["info"]["n_obstacles"] == (2 if min_count == 3 else 1)
        assert out["dist_sq"][1, 1, 1] == (9 if min_count == 3 else 36)
    return _case(st, centred((9, 3, 3)), (9, 3, 3), min_count=min_count, max_dist_voxels=8, expect=expect)


def _labels(**lists):
    """rows 0..4 with labels 1, 2 (a tie 2 = 3 that goes to 2), 3, 0 (bin 0 wins), 4"""
    v = [(1, 1, 0), (4, 1, 0), (7, 1, 0), (10, 1, 0), (13, 1, 0)]
    hist = [[0, 3, 0, 0, 0], [0, 1, 2, 2, 0], [0, 0, 1, 4, 0], [5, 1, 0, 0, 0], [0, 0, 0, 0, 2]]
    st = make_state(v, hist=hist, seed=41)
    labels = [1, 2, 3, 0, 4]
    def expect(out):
        kept = [l for l in labels if l not in lists.get("ignore", ()) and (not lists.get("only") or l in lists["only"])]
        assert 0 < len(kept) < 5 and out["info"]["n_obstacles"] == len(kept)
        assert sorted(set(out["label"][out["dist_sq"] >= 0].tolist())) == sorted(kept)
        assert out["dist_sq"][0, 1, 4] == (0 if 2 in kept else 9 if (1 in kept or 3 in kept) else 36)
    return _case(st, centred((15, 3, 1)), (15, 3, 1), max_dist_voxels=6, expect=expect, **lists)


def _no_classes():
    def expect(out):
        assert not out["label"].any() and (out["dist_sq"] >= 0).sum() > 100
    return _case(patch_state(0), (0.1, 0.1, 1.1), (11, 9, 6), max_dist_voxels=2, expect=expect)


def _all_ignored():
    st = make_state(_random_voxels(42, 30, (0, 0, 0), (6, 6, 3)), label=3, seed=43)
    def expect(out):
        assert (out["dist_sq"] == -1).all() and (out["nearest"] == -1).all() and not out["label"].any()
        assert out["info"]["n_obstacles"] == 0 and out["info"]["n_reached"] == 0 and out["info"]["n_voxels"] > 20
    return _case(st, centred((6, 6, 3)), (6, 6, 3), ignore=(3,), max_dist_voxels=4, expect=expect)


def _empty_map():
    st = dict(key=np.zeros(0, np.uint64), sums=np.zeros((0, 3)), count=np.zeros(0, np.uint32), hist=np.zeros((0, CLASSES + 1), np.uint32),
              leaf_size=LEAF, num_classes=CLASSES)
    def expect(out):
        assert (out["dist_sq"] == -1).all() and (out["nearest"] == -1).all() and not out["label"].any()
        assert out["info"]["n_voxels"] == 0 and out["info"]["n_reached"] == 0 and out["info"]["max_dist_sq"] == -1
    return _case(st, (1.0, -1.0, 0.3), (7, 5, 3), expect=expect)


# ---- planar --------------------------------------------------------------------------------------------------------------------
PLANAR_BAND = dict(z_min=1.0, z_max=2.9)  # levels 2 .. 5 at leaf 0.5


def _planar_band():
    """column (2, 2): rows at levels 0, 3, 7 -- the band cuts it, level 3 counts; column (6, 2): levels 3 and 4, the smaller row
    is level 3; column (10, 2): levels 0 and 9 only, no obstacle; column (2, 6): levels 2 and 5, the band's ends, inclusive"""
    v = [(2, 2, 0), (2, 2, 3), (2, 2, 7), (6, 2, 3), (6, 2, 4), (10, 2, 0), (10, 2, 9), (2, 6, 5), (2, 6, 2)]
    st = make_state(v, label=[1, 2, 3, 4, 1, 2, 3, 4, 1], count=1, frac=0.5)
    def expect(out):
        d, near, lab = out["dist_sq"][0], out["nearest"][0], out["label"][0]
        assert out["info"]["n_obstacles"] == 3 and out["info"]["z0"] == 0
        assert d[2, 2] == 0 and near[2, 2] == row_of(st, (2, 2, 3)) and lab[2, 2] == 2
        assert d[2, 6] == 0 and near[2, 6] == row_of(st, (6, 2, 3)) and lab[2, 6] == 4
        assert d[6, 2] == 0 and near[6, 2] == row_of(st, (2, 6, 2)) and lab[6, 2] == 1
        assert d[2, 10] == 16 and near[2, 10] == row_of(st, (6, 2, 3))  # its own rows lie outside the band
        assert d[2, 4] == 4 and near[2, 4] == row_of(st, (2, 2, 3))     # midway between columns (2, 2) and (6, 2): the smaller row
        assert d[4, 2] == 4 and near[4, 2] == row_of(st, (2, 6, 2))     # midway between (2, 2) and (2, 6): level 2 is the smaller row
    centre = centred((12, 9, 1))[:2] + (123.0,)  # (z is not looked at)
    return _case(st, centre, (12, 9, 1), planar=1, max_dist_voxels=4, expect=expect, **PLANAR_BAND)


def _planar_patch():
    def expect(out):
        assert out["dist_sq"].shape == (1, 21, 23) and (out["dist_sq"] == 0).sum() == out["info"]["n_obstacles"] > 50
        assert (out["dist_sq"] > 0).any() and (out["dist_sq"] < 0).any()
    return _case(patch_state(), (0.3, -0.4, -7.0), (23, 21, 1), planar=1, max_dist_voxels=3, z_min=0.6, z_max=1.4, ignore=(2,), expect=expect)


# ---- dense ---------------------------------------------------------------------------------------------------------------------
def _dense():
    shape = (96, 80, 40)
    rng = np.random.default_rng(44)
    cells = shape[0] * shape[1] * shape[2]
    at = rng.choice(cells, cells // 100, replace=False)
    v = np.stack([at % shape[0], (at // shape[0]) % shape[1], at // (shape[0] * shape[1])], axis=1)
    def expect(out):
        assert out["info"]["n_obstacles"] == cells // 100 and out["info"]["n_reached"] > 0.99 * cells
    return _case(make_state(v, seed=45), centred(shape), shape, max_dist_voxels=8, expect=expect)


# ---- points --------------------------------------------------------------------------------------------------------------------
def _points(planar):
    rng = np.random.default_rng(46)
    xyz = rng.uniform(-8, 8, (500, 3)).astype(np.float32)
    xyz[:, 2] = rng.uniform(-1, 3, 500)
    xyz[7, 0] = np.nan
    xyz[8, 2] = np.inf
    xyz[9] = (3.0e6, 0.0, 0.0)     # beyond the key's range at leaf 0.5, under the pose too
    xyz[10] = (0.0, -3.0e6, 1.0)
    xyz[11] = (300.0, 2.0, 1.0)    # far outside the window
    M = np_ref.qt_to_mat(pose())   # a point that the pose moves over the window's centre at a z beyond the key's range: outside in
    xyz[12] = M[:3, :3].T @ (np.array([0.3, -0.4, 2.0e6]) - M[:3, 3])  # 3-D, its column's cell in planar mode
    lab = rng.integers(1, CLASSES + 1, 500).astype(np.uint32)
    xyz.setflags(write=False)
    lab.setflags(write=False)
    def expect(out):
        pc, pd, pn = out["point_cell"], out["point_dist_sq"], out["point_nearest"]
        assert (pc[7:12] == -1).all() and (pd[7:12] == -1).all() and (pn[7:12] == -1).all()
        assert (pc[12] >= 0) == bool(planar)
        inside = pc >= 0
        unreached = inside & (pd < 0)
        assert inside.sum() == out["info"]["n_points_inside"] > 60 and (~inside).sum() > 20 and unreached.sum() > 10
        assert (pn[unreached] == -1).all() and (pn[inside & ~unreached] >= 0).all() and (inside & ~unreached).sum() > 30
        flat = out["dist_sq"].reshape(-1)
        assert np.array_equal(pd[inside], flat[pc[inside]])
        if planar:
            assert "point_range_sq" not in out
        else:
            pr = out["point_range_sq"]
            assert np.isnan(pr[~inside | unreached]).all() and np.isfinite(pr[inside & ~unreached]).all()
            assert pr[~inside].tobytes() == np.full((~inside).sum(), 0x7FC00000, np.uint32).tobytes()
    if planar:
        return _case(patch_state(), (0.3, -0.4, 0.0), (17, 14, 1), points=xyz, point_labels=lab, qt=pose(), planar=1, max_dist_voxels=1,
                     z_min=1.0, z_max=1.4, expect=expect)
    return _case(patch_state(), (0.3, -0.4, 1.0), (17, 14, 9), points=xyz, point_labels=lab, qt=pose(), max_dist_voxels=1, expect=expect)


CASES = {
    "one_cell_occupied": functools.partial(_one_cell, True),
    "one_cell_beside": functools.partial(_one_cell, False),
    "shape_67x5x3": functools.partial(_shape, 50, (67, 5, 3), 60, 4),
    "shape_130x66x35": functools.partial(_shape, 52, (130, 66, 35), 900, 6),
    "long_line_r64": _long_line,
    "r_larger_than_window": _r_larger_than_window,
    "r1": _r1,
    "ball_not_cube": _ball_not_cube,
    "tie_midway": _tie_midway,
    "tie_axes": _tie_axes,
    "tie_decompositions": _tie_decompositions,
    "faces": _faces,
    "outside_within_r": _outside_within_r,
    "key_range_high": functools.partial(_key_range, 1),
    "key_range_low": functools.partial(_key_range, -1),
    "min_count_at": functools.partial(_min_count, 3),
    "min_count_above": functools.partial(_min_count, 4),
    "ignore": functools.partial(_labels, ignore=(2, 0)),
    "ignore_tie_loser": functools.partial(_labels, ignore=(3,)),
    "only": functools.partial(_labels, only=(2, 4)),
    "ignore_and_only": functools.partial(_labels, ignore=(4,), only=(4, 0, 1)),
    "no_classes": _no_classes,
    "all_ignored": _all_ignored,
    "empty_map": _empty_map,
    "planar_band": _planar_band,
    "planar_patch": _planar_patch,
    "dense": _dense,
    "points_posed": functools.partial(_points, 0),
    "points_planar": functools.partial(_points, 1),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def freeze(out):
    for k, a in out.items():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return freeze(ref.distance(c["state"], c["params"], c["center"], c["points"], c["qt"]))


# ---- what is refused: the keywords of params that the call refuses on a map with CLASSES classes, and their accepted neighbours
REFUSED = {
    "nx 0": dict(nx=0), "nx 1025": dict(nx=1025), "ny 0": dict(ny=0), "ny 1025": dict(ny=1025), "nz 0": dict(nz=0), "nz 257": dict(nz=257),
    "2^24 + 1024 cells": dict(nx=1024, ny=1024, nz=17), "max_dist_voxels 0": dict(max_dist_voxels=0), "max_dist_voxels 65": dict(max_dist_voxels=65),
    "min_count 0": dict(min_count=0), "planar 2": dict(planar=2, nz=1), "planar -1": dict(planar=-1, nz=1), "planar with nz 2": dict(planar=1, nz=2),
    "z_min NaN": dict(z_min=math.nan), "z_max NaN": dict(z_max=math.nan), "z_min above z_max": dict(z_min=1.0, z_max=0.5),
    "an ignored label above num_classes": dict(ignore=(CLASSES + 1,)), "an only label above": dict(only=(1, CLASSES + 1)),
}
ACCEPTED = {
    "z_min = z_max": dict(z_min=0.5, z_max=0.5), "infinite z": dict(z_min=-math.inf, z_max=math.inf), "z both +inf": dict(z_min=math.inf),
    "label num_classes": dict(ignore=(CLASSES,), only=(0, CLASSES)), "2^24 cells": dict(nx=1024, ny=1024, nz=16), "nz 256": dict(nx=256, ny=256, nz=256),
    "max_dist_voxels 64": dict(max_dist_voxels=64), "planar with nz 1": dict(planar=1, nz=1),
}


# ---- the naive twin -------------------------------------------------------------------------------------------------------------
def _f32(x):
    return np.float32(x)


def _level(z, inv, lo, hi):
    if z == -math.inf:
        return lo
    if z == math.inf:
        return hi
    with np.errstate(over="ignore"):
        f = float(np.floor(_f32(_f32(z) * inv)))
    return int(min(max(f, float(lo)), float(hi)))


def naive(state, p, center, points=None, qt=None):
    """sicp_map_distance by the header's rules: every obstacle in ascending map row against every cell of the cube of half-side R
    about it; a cell keeps the first obstacle at its smallest d^2 (a later row has to be strictly nearer), and the ball's test
    comes last.  No packed keys, no separable passes."""
    leaf, C = state["leaf_size"], state["num_classes"]
    nx, ny, nz, R, planar = p["nx"], p["ny"], p["nz"], p["max_dist_voxels"], p["planar"]
    inv = _f32(1.0) / _f32(leaf)
    vc = [int(math.floor(float(_f32(_f32(center[d]) * inv)))) for d in range(3)]
    x0, y0, z0 = vc[0] - nx // 2, vc[1] - ny // 2, (0 if planar else vc[2] - nz // 2)
    lo, hi = _level(p["z_min"], inv, -EDGE, EDGE), _level(p["z_max"], inv, -EDGE, EDGE)
    n = len(state["key"])

    def fullest(bins):
        best = 0
        for l in range(1, len(bins)):
            if bins[l] > bins[best]:
                best = l
        return best

    labels = [fullest([int(b) for b in state["hist"][r]]) if C > 0 else 0 for r in range(n)]
    best = np.full((nz, ny, nx), 1 << 40, np.int64)
    near = np.full((nz, ny, nx), -1, np.int64)
    taken = set()
    n_obstacles = 0
    for r in range(n):  # ascending map row
        key = int(state["key"][r])
        vx, vy, vz = (key & 0x1FFFFF) - BIAS, ((key >> 21) & 0x1FFFFF) - BIAS, (key >> 42) - BIAS
        if int(state["count"][r]) < p["min_count"]:
            continue
        if len(p["ignore"]) and labels[r] in [int(l) for l in p["ignore"]]:
            continue
        if len(p["only"]) and labels[r] not in [int(l) for l in p["only"]]:
            continue
        if planar and not lo <= vz <= hi:
            continue
        i, j, k = vx - x0, vy - y0, (0 if planar else vz - z0)
        if not (0 <= i < nx and 0 <= j < ny and 0 <= k < nz):
            continue
        if (i, j, k) in taken:  # (planar: the column has its row, the smallest)
            continue
        taken.add((i, j, k))
        n_obstacles += 1
        i0, i1, j0, j1, k0, k1 = max(i - R, 0), min(i + R, nx - 1), max(j - R, 0), min(j + R, ny - 1), max(k - R, 0), min(k + R, nz - 1)
        dk, dj, di = np.meshgrid(np.arange(k0, k1 + 1) - k, np.arange(j0, j1 + 1) - j, np.arange(i0, i1 + 1) - i, indexing="ij")
        d2 = di * di + dj * dj + dk * dk
        box = (slice(k0, k1 + 1), slice(j0, j1 + 1), slice(i0, i1 + 1))
        nearer = (d2 <= R * R) & (d2 < best[box])
        best[box] = np.where(nearer, d2, best[box])
        near[box] = np.where(nearer, r, near[box])
    reached = near >= 0
    out = dict(dist_sq=np.where(reached, best, -1).astype(np.int32), nearest=near.astype(np.int32),
               label=np.array([labels[r] if r >= 0 else 0 for r in near.reshape(-1)], np.uint32).reshape(nz, ny, nx))

    n_points = n_inside = 0
    if points is not None:
        M = np_ref.qt_to_mat(np.array([0, 0, 0, 1, 0, 0, 0.0]) if qt is None else qt)
        n_points = len(points)
        pc, pd, pn = (np.full(n_points, -1, np.int32) for _ in range(3))
        pr = np.full(n_points, ref.NAN, np.float32)
        for g in range(n_points):
            x, y, z = (float(a) for a in points[g])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                continue
            with np.errstate(over="ignore", invalid="ignore"):
                q = [_f32(((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]) for a in range(3)]
                v = [float(np.floor(_f32(q[a] * inv))) for a in range(3)]
            if not all(abs(v[a]) < BIAS for a in range(2 if planar else 3)):
                continue
            i, j, k = int(v[0]) - x0, int(v[1]) - y0, (0 if planar else int(v[2]) - z0)
            if not (0 <= i < nx and 0 <= j < ny and 0 <= k < nz):
                continue
            n_inside += 1
            pc[g], pd[g], pn[g] = (k * ny + j) * nx + i, out["dist_sq"][k, j, i], out["nearest"][k, j, i]
            if not planar and pn[g] >= 0:
                c = [_f32(float(state["sums"][pn[g]][a]) / float(state["count"][pn[g]])) for a in range(3)]
                d = [_f32(q[a] - c[a]) for a in range(3)]
                pr[g] = _f32(_f32(_f32(d[0] * d[0]) + _f32(d[1] * d[1])) + _f32(d[2] * d[2]))
        out["point_cell"], out["point_dist_sq"], out["point_nearest"] = pc, pd, pn
        if not planar:
            out["point_range_sq"] = pr
    out["info"] = dict(n_voxels=n, n_points=n_points, n_points_inside=n_inside, x0=x0, y0=y0, z0=z0, nx=nx, ny=ny, nz=nz,
                       n_obstacles=n_obstacles, n_reached=int(reached.sum()), max_dist_sq=int(best[reached].max()) if reached.any() else -1,
                       voxel_size=leaf)
    return out
