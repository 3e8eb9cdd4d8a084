"""Inputs of the elevation tests (tests/test_elevation_cpu.py on the restatement, tests/test_gpu_elevation.py through the
library): hand-built map states -- get_state() dicts -- with a window and params each, the smallest shapes at which the kernels
of sicp_map_elevation can go wrong, and naive(): the header's rules once more, cell by cell in plain Python loops, written from
include/sicp.h and not from tests/elevation_ref.py.

CASES            name -> a function giving {"state", "center", "width", "height", "params" (elevation_ref.defaults), "points"
                 ([n, 3] float32 or None), "point_labels", "qt", "expect" (a function of the result that asserts what the case is
                 named for)}
case(name)       that dict, built once and read-only
reference(name)  the restatement's answer, computed once and read-only
Hand cases use leaf 0.5 (inv_leaf = 2 exactly) and, where values are written out, a mean z of (level + 0.5) * leaf per voxel."""
from __future__ import annotations

import functools
import math

import numpy as np

import elevation_ref as ref
import np_ref

LEAF = 0.5
CLASSES = 4
BIAS = 1 << 20


# ---- map states ---------------------------------------------------------------------------------------------------------------
def make_state(v, count=None, label=None, hist=None, leaf=LEAF, num_classes=CLASSES, frac=None, seed=0):
    """a get_state() dict of the voxels v [n, 3] (vx, vy, vz; distinct): `count` points each (default 1..5 at random), all with
    `label` (default random 1..C) unless `hist` [n, C + 1] is given, at a mean z of (vz + frac) * leaf (frac: a number, or None for
    random in 0.1..0.9 per voxel)"""
    rng = np.random.default_rng(seed)
    v = np.asarray(v, dtype=np.int64).reshape(-1, 3)
    n = len(v)
    key = ((v[:, 2] + BIAS) << 42) | ((v[:, 1] + BIAS) << 21) | (v[:, 0] + BIAS)
    assert len(np.unique(key)) == n, "the voxels are not distinct"
    count = rng.integers(1, 6, n) if count is None else np.broadcast_to(np.asarray(count, dtype=np.int64), (n,))
    f = rng.uniform(0.1, 0.9, (n, 3)) if frac is None else np.full((n, 3), float(frac))
    sums = (v + f) * leaf * count[:, None]
    h = None
    if num_classes > 0:
        if hist is not None:
            h = np.asarray(hist, dtype=np.uint32).reshape(n, num_classes + 1)
            count = h.sum(axis=1).astype(np.int64)
            sums = (v + f) * leaf * count[:, None]
        else:
            lab = rng.integers(1, num_classes + 1, n) if label is None else np.broadcast_to(np.asarray(label, dtype=np.int64), (n,))
            h = np.zeros((n, num_classes + 1), np.uint32)
            h[np.arange(n), lab] = count
    order = np.argsort(key)
    st = dict(key=key[order].astype(np.uint64), sums=np.ascontiguousarray(sums[order], dtype=np.float64), count=count[order].astype(np.uint32),
              hist=None if h is None else np.ascontiguousarray(h[order]), leaf_size=float(leaf), num_classes=int(num_classes))
    for a in ("key", "sums", "count", "hist"):
        if st[a] is not None:
            st[a].setflags(write=False)
    return st


def centre_of(vx, vy, leaf=LEAF):
    """a centre inside the voxel column (vx, vy)"""
    return ((vx + 0.5) * leaf, (vy + 0.5) * leaf)


def _case(state, center, width, height, points=None, point_labels=None, qt=None, expect=None, **params):
    return dict(state=state, center=tuple(float(c) for c in center), width=width, height=height,
                params=ref.defaults(width=width, height=height, **params), points=points, point_labels=point_labels, qt=qt,
                expect=expect if expect is not None else (lambda out: None))


def _column(vx, vy, levels):
    return [(vx, vy, int(l)) for l in levels]


SEGMENT_ROWS = (0, 1, 2, 63, 64, 65, 128, 129)


def _segments_b1():
    rng = np.random.default_rng(5)
    v = []
    for k, n in enumerate(SEGMENT_ROWS):
        levels = np.cumsum(rng.choice([1, 1, 1, 2, 12], n)) - 40
        v += _column(k, 0, levels)
    # x0 = 4 - 5 = -1, y0 = 0 - 1 = -1: cell (k + 1, 1) is column k
    def expect(out):
        assert out["state"][1, 1:9].tolist() == [0, 1, 1, 1, 1, 1, 1, 1] and int(out["state"].sum()) == 7
        assert out["n_levels"].max() > 1 and np.isfinite(out["ceiling"][1]).any() and np.isinf(out["ceiling"][1]).any()
    return _case(make_state(v, seed=6), centre_of(4, 0), 10, 3, expect=expect)


def _segments_b2():
    rng = np.random.default_rng(7)
    v = []
    for k, n in enumerate(SEGMENT_ROWS):
        pick = rng.choice(4 * 41, n, replace=False)  # (column of the cell's four, level 0..40)
        v += [(2 * k + (q % 4) % 2, (q % 4) // 2, int(q // 4)) for q in pick]
    # B = 2: vc = (8, 0), fdiv = (4, 0), x0 = 4 - 5 = -1, y0 = -1: cell (k + 1, 1) is the columns 2k, 2k + 1 x 0, 1
    def expect(out):
        assert out["state"][1, 1:9].tolist() == [0, 1, 1, 1, 1, 1, 1, 1] and int(out["state"].sum()) == 7
        assert out["info"]["cell_size"] == 1.0
    return _case(make_state(v, seed=8), centre_of(8, 0), 10, 3, cell_voxels=2, clearance_voxels=3, expect=expect)


def _clearance_exact():
    v = _column(0, 0, [0, 10]) + _column(1, 0, [0, 11])
    # x0 = 0 - 2 = -2, y0 = 0 - 1 = -1: the columns are the cells (2, 1) and (3, 1)
    def expect(out):
        assert out["n_levels"][1, 2] == 2 and out["level_top"][1, 2] == 10 and np.isinf(out["ceiling"][1, 2])
        assert out["n_levels"][1, 3] == 1 and out["level_top"][1, 3] == 0 and out["ceiling"][1, 3] == np.float32(5.75)
    return _case(make_state(v, count=2, label=1, frac=0.5), centre_of(0, 0), 4, 2, max_extent_voxels=20, expect=expect)


THREE_RUNS = ((0, 1), (20, 21, 22), (40,))
# ref_z -> (vref, the run chosen in the column of three runs)
THREE_RUNS_REF = {"below": (-3.0, 0), "in0": (0.6, 0), "in1": (10.7, 1), "on1": (10.0, 1), "in2": (20.2, 2), "above": (100.0, 2)}


def _three_runs(which):
    v = _column(0, 0, sum(THREE_RUNS, ())) + _column(1, 0, [20])
    ref_z, run = THREE_RUNS_REF[which]
    def expect(out):
        levels = THREE_RUNS[run]
        assert (out["level_bottom"][0, 1], out["level_top"][0, 1], out["n_levels"][0, 1]) == (levels[0], levels[-1], len(levels))
        if run < 2:
            assert out["ceiling"][0, 1] == np.float32((THREE_RUNS[run + 1][0] + 0.5) * LEAF)
        else:
            assert np.isinf(out["ceiling"][0, 1])
        assert out["level_top"][0, 2] == 20  # one run, whatever ref_z
    # x0 = 0 - 1 = -1, y0 = 0: the columns are the cells (1, 0) and (2, 0)
    return _case(make_state(v, count=3, label=2, frac=0.5), centre_of(0, 0), 3, 1, use_ref_z=1, ref_z=ref_z, expect=expect)


def _b8_full():
    cols = [(x, y) for y in range(8) for x in range(8)]
    v = []
    for l in (3, 4, 5, 16):
        v += [(x, y, l) for x, y in cols]
    for l in (5, 6):
        v += [(x + 8, y, l) for x, y in cols]
    v += [(x - 8, y, 5) for x, y in cols]
    # vc = (4, 4), fdiv = (0, 0), x0 = -2, y0 = -1: the cells (1, 1), (2, 1), (3, 1)
    def expect(out):
        assert out["level_top"][1, 1:4].tolist() == [5, 5, 6] and out["n_levels"][1, 1:4].tolist() == [1, 3, 2]
        assert np.isfinite(out["ceiling"][1, 2]) and int(out["state"].sum()) == 3
        assert (out["count"][1, 1:4] >= 64).all()
    return _case(make_state(v, seed=9), centre_of(4, 4), 4, 3, cell_voxels=8, expect=expect)


def _b3_negative():
    at = (-4, -3, -1, 0, 2)
    v = [(x, y, 0) for x in at for y in at] + [(x, -1, 1) for x in at]
    # vc = (-1, -1), fdiv(-1, 3) = -1, x0 = y0 = -1 - 2 = -3: cells -3 .. 0; columns -4 | -3, -1 | 0, 2 are the cells -2 | -1 | 0
    def expect(out):
        assert out["state"].tolist() == [[0, 0, 0, 0], [0, 1, 1, 1], [0, 1, 1, 1], [0, 1, 1, 1]]
        assert out["level_top"][2].tolist() == [0, 1, 1, 1] and out["level_top"][1].tolist() == [0, 0, 0, 0]
    return _case(make_state(v, seed=10), centre_of(-1, -1), 4, 4, cell_voxels=3, expect=expect)


@functools.lru_cache(maxsize=None)
def patch_state(num_classes=CLASSES):
    rng = np.random.default_rng(11)
    v = np.unique(np.stack([rng.integers(-12, 13, 900), rng.integers(-12, 13, 900), rng.integers(-2, 7, 900)], axis=1), axis=0)
    return make_state(v, num_classes=num_classes, seed=12)


def _window(width, height, center, **params):
    def expect(out):
        assert out["state"].shape == (height, width) and 0 < int(out["state"].sum())
    return _case(patch_state(), center, width, height, clearance_voxels=2, expect=expect, **params)


def _window_1x1():
    st = patch_state()
    k = int(st["key"][len(st["key"]) // 2])
    vx, vy = (k & 0x1FFFFF) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS
    def expect(out):
        assert out["state"].tolist() == [[1]] and out["neighbors"].tolist() == [[0]] and out["step"].tolist() == [[0.0]]
    return _case(st, centre_of(vx, vy), 1, 1, expect=expect)


def _edges_outside():
    # the window: x0 = 10 - 2 = 8 .. 11, y0 = -20 - 1 = -21 .. -19
    inside = [(8, -21), (11, -21), (8, -19), (11, -19), (9, -20)]
    outside = [(7, -20), (12, -20), (9, -22), (9, -18), (7, -22), (12, -18)]
    v = [(x, y, 3) for x, y in inside + outside]
    def expect(out):
        assert out["state"].tolist() == [[1, 0, 0, 1], [0, 1, 0, 0], [1, 0, 0, 1]] and out["info"]["n_voxels"] == 11
        assert (out["info"]["x0"], out["info"]["y0"]) == (8, -21)
    return _case(make_state(v, seed=13), centre_of(10, -20), 4, 3, expect=expect)


def _z_inclusive():
    v = _column(0, 0, [1, 2, 3, 4, 5]) + _column(1, 0, [1, 5])
    def expect(out):  # z_min = 1.0 is level 2, z_max = 2.0 is level 4, both seen
        assert (out["level_bottom"][0, 1], out["level_top"][0, 1], out["n_levels"][0, 1]) == (2, 4, 3)
        assert out["state"][0].tolist() == [0, 1, 0]
    return _case(make_state(v, seed=14), centre_of(0, 0), 3, 1, z_min=1.0, z_max=2.0, max_extent_voxels=5, expect=expect)


def _min_count(min_count):
    v = _column(0, 0, [0, 1]) + _column(1, 0, [0])
    count = [5, 3, 3]
    def expect(out):  # the top voxel of column 0 and the one of column 1 hold 3 points
        assert out["level_top"][0, 1] == (1 if min_count == 3 else 0) and out["state"][0, 2] == (1 if min_count == 3 else 0)
    return _case(make_state(v, count=count, label=1, seed=15), centre_of(0, 0), 3, 1, min_count=min_count, expect=expect)


def _ignore_tie(ignored):
    v = _column(0, 0, [0, 1])
    hist = [[0, 0, 4, 0, 0], [0, 2, 2, 0, 0]]  # the upper voxel's label is 1 by the tie rule alone
    def expect(out):
        assert out["state"][0, 0] == 1
        if ignored == 1:
            assert out["label"][0, 0] == 2 and out["level_top"][0, 0] == 0
        else:
            assert out["label"][0, 0] == 1 and out["level_top"][0, 0] == 1 and out["n_levels"][0, 0] == 1
    return _case(make_state(v, hist=hist, seed=16), centre_of(0, 0), 1, 1, ignore=(ignored,), expect=expect)


def _bin0_wins():
    v = _column(0, 0, [0]) + _column(1, 0, [0])
    hist = [[5, 1, 0, 0, 0], [1, 0, 0, 0, 3]]
    def expect(out):
        assert out["label"][0].tolist() == [0, 0, 4] and out["cell_class"][0].tolist() == [ref.UNKNOWN, ref.BLOCKED_LABEL, ref.FREE]
    return _case(make_state(v, hist=hist, seed=17), centre_of(0, 0), 3, 1, blocked=(0,), expect=expect)


def _no_classes():
    def expect(out):
        assert not out["label"].any() and int(out["state"].sum()) > 20
    return _case(patch_state(0), (0.1, 0.1), 9, 8, clearance_voxels=2, expect=expect)


# the cells of classes_all that are asserted by hand: name -> ((i, j), class)
CLASSES_ALL = {"road": ((1, 1), ref.FREE), "empty": ((5, 5), ref.UNKNOWN), "blocked_and_tall": ((0, 7), ref.BLOCKED_LABEL),
               "not_drivable": ((2, 7), ref.BLOCKED_LABEL), "tall_low_stepped": ((4, 7), ref.OBSTACLE),
               "low_and_stepped": ((6, 7), ref.LOW_CLEARANCE), "stepped_and_sparse": ((8, 7), ref.STEP), "lonely": ((10, 7), ref.SPARSE)}


def _classes_all():
    v, lab = [], []
    def add(cells, label):
        v.extend(cells)
        lab.extend([label] * len(cells))
    add([(i, j, 0) for i in range(4) for j in range(4)], 1)                 # the road
    for i in (0, 2, 4, 6, 8):
        add([(i, 6, 0), (i, 8, 0)], 1)                                       # a flat cell on either side of a special one
    add(_column(0, 7, [0, 1, 2, 3]), 3)                                      # blocked, and tall as well
    add(_column(2, 7, [0]), 4)                                               # a label that is not drivable
    add(_column(4, 7, [0, 1, 2, 3, 7]), 1)                                   # tall; low under level 7 and stepped as well
    add(_column(6, 7, [2, 6]), 1)                                            # low under level 6; stepped as well
    add(_column(8, 7, [2]), 1)                                               # stepped; two neighbours of the three asked for
    add(_column(10, 7, [0]), 1)                                              # nobody around
    def expect(out):
        for name, ((i, j), cls) in CLASSES_ALL.items():
            assert out["cell_class"][j, i] == cls, name
        assert all(n > 0 for n in out["info"]["n_class"][:7]) and out["info"]["n_class"][7] == 0
    # vc = (6, 4): x0 = 6 - 6 = 0, y0 = 4 - 4 = 0
    return _case(make_state(v, count=2, label=lab, frac=0.5), centre_of(6, 4), 12, 9, blocked=(3,), drivable=(1, 2, 3), max_extent_voxels=2,
                 clearance_voxels=3, min_clearance=3.0, max_step=0.6, min_neighbors=3, expect=expect)


def _stencil_edges():
    rng = np.random.default_rng(18)
    v = [(i, j, int(rng.integers(0, 4))) for i in range(4) for j in range(3)]
    def expect(out):  # corners 3, edges 5, inside 8
        assert out["neighbors"].tolist() == [[3, 5, 5, 3], [5, 8, 8, 5], [3, 5, 5, 3]] and (out["step"] >= 0).all()
    # vc = (2, 1): x0 = 0, y0 = 0
    return _case(make_state(v, seed=19), centre_of(2, 1), 4, 3, expect=expect)


def _lonely():
    def expect(out):
        assert out["state"].sum() == 1 and out["neighbors"][1, 1] == 0 and out["step"][1, 1] == 0 and out["cell_class"][1, 1] == ref.FREE
    return _case(make_state([(5, 5, 2)], seed=20), centre_of(5, 5), 3, 3, expect=expect)


def _empty_map():
    st = dict(key=np.zeros(0, np.uint64), sums=np.zeros((0, 3)), count=np.zeros(0, np.uint32), hist=np.zeros((0, CLASSES + 1), np.uint32),
              leaf_size=LEAF, num_classes=CLASSES)
    def expect(out):
        assert not out["state"].any() and out["info"]["n_class"] == [35, 0, 0, 0, 0, 0, 0, 0]
    return _case(st, (1.0, -1.0), 7, 5, expect=expect)


def _large_random():
    rng = np.random.default_rng(21)
    n = 230000
    v = np.unique(np.stack([rng.integers(-150, 151, n), rng.integers(-120, 121, n), rng.integers(-6, 7, n)], axis=1), axis=0)
    def expect(out):
        assert 190000 < out["info"]["n_voxels"] < 230000 and out["info"]["n_class"][ref.UNKNOWN] < 256 * 200 // 4
    return _case(make_state(v, leaf=0.2, num_classes=19, seed=22), (0.5, -0.7), 256, 200, clearance_voxels=2, ignore=(7, 19), max_step=0.3,
                 min_neighbors=6, min_clearance=1.0, blocked=(3,), expect=expect)


def pose():
    """a pose that is no identity: a quaternion (x, y, z, w) about a tilted axis, a translation"""
    a = np.array([0.1, -0.05, 1.0])
    a = a / np.linalg.norm(a)
    h = 0.35
    return np.concatenate([a * np.sin(h), [np.cos(h)], [0.7, -1.1, 0.4]])


def _points_posed():
    rng = np.random.default_rng(23)
    xyz = rng.uniform(-8, 8, (500, 3)).astype(np.float32)
    xyz[:, 2] = rng.uniform(-1, 3, 500)
    xyz[7, 0] = np.nan
    xyz[8, 2] = np.inf
    xyz[9] = (3.0e6, 0.0, 0.0)     # beyond the key's range at leaf 0.5, under the pose too
    xyz[10] = (0.0, -3.0e6, 1.0)
    xyz[11] = (300.0, 2.0, 1.0)    # far outside the window
    lab = rng.integers(1, CLASSES + 1, 500).astype(np.uint32)
    xyz.setflags(write=False)
    lab.setflags(write=False)
    def expect(out):
        pc, ph = out["point_cell"], out["point_height"]
        assert (pc[7:12] == -1).all() and np.isnan(ph[7:12]).all()
        inside = pc >= 0
        empty = inside & (out["state"].reshape(-1)[np.maximum(pc, 0)] == 0)
        assert inside.sum() > 100 and (~inside).sum() > 20 and empty.sum() > 10 and np.isnan(ph[empty]).all()
        assert np.isfinite(ph[inside & ~empty]).all() and (inside & ~empty).sum() > 50
    return _case(patch_state(), (0.3, -0.4), 17, 14, points=xyz, point_labels=lab, qt=pose(), clearance_voxels=2, expect=expect)


CASES = {
    "segments_b1": _segments_b1,
    "segments_b2": _segments_b2,
    "clearance_exact": _clearance_exact,
    **{"three_runs_ref_" + k: functools.partial(_three_runs, k) for k in THREE_RUNS_REF},
    "b8_full": _b8_full,
    "b3_negative": _b3_negative,
    "window_odd": functools.partial(_window, 5, 7, (0.3, 0.3)),
    "window_even": functools.partial(_window, 6, 4, (0.3, 0.3)),
    "window_negative_centre": functools.partial(_window, 7, 6, (-3.7, -4.2)),
    "window_b4_ref": functools.partial(_window, 5, 5, (-1.0, 1.0), cell_voxels=4, use_ref_z=1, ref_z=1.6),
    "window_1x1": _window_1x1,
    "window_2048x1": functools.partial(_window, 2048, 1, (0.3, 0.3)),
    "edges_outside": _edges_outside,
    "z_inclusive": _z_inclusive,
    "min_count_at": functools.partial(_min_count, 3),
    "min_count_above": functools.partial(_min_count, 4),
    "ignore_tie_winner": functools.partial(_ignore_tie, 1),
    "ignore_tie_loser": functools.partial(_ignore_tie, 2),
    "bin0_wins": _bin0_wins,
    "no_classes": _no_classes,
    "classes_all": _classes_all,
    "stencil_edges": _stencil_edges,
    "lonely": _lonely,
    "empty_map": _empty_map,
    "large_random": _large_random,
    "points_posed": _points_posed,
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
    return freeze(ref.elevation(c["state"], c["params"], c["center"], c["points"], c["qt"]))


# ---- what is refused: the keywords of params that the call refuses on a map with CLASSES classes, and their accepted neighbours
REFUSED = {
    "width 0": dict(width=0), "width 2049": dict(width=2049), "height 0": dict(height=0), "height 2049": dict(height=2049),
    "cell_voxels 0": dict(cell_voxels=0), "cell_voxels 9": dict(cell_voxels=9), "min_count 0": dict(min_count=0),
    "z_min NaN": dict(z_min=math.nan), "z_max NaN": dict(z_max=math.nan), "z_min above z_max": dict(z_min=1.0, z_max=0.5),
    "clearance_voxels 0": dict(clearance_voxels=0), "use_ref_z 2": dict(use_ref_z=2), "ref_z inf": dict(use_ref_z=1, ref_z=math.inf),
    "ref_z NaN": dict(use_ref_z=1, ref_z=math.nan), "max_extent_voxels -1": dict(max_extent_voxels=-1),
    "min_clearance -1": dict(min_clearance=-1.0), "min_clearance NaN": dict(min_clearance=math.nan), "max_step -1": dict(max_step=-0.5),
    "max_step NaN": dict(max_step=math.nan), "min_neighbors -1": dict(min_neighbors=-1), "min_neighbors 9": dict(min_neighbors=9),
    "an ignored label above num_classes": dict(ignore=(CLASSES + 1,)), "a blocked label above": dict(blocked=(1, CLASSES + 1)),
    "a drivable label above": dict(drivable=(99,)),
}
ACCEPTED = {
    "z_min = z_max": dict(z_min=0.5, z_max=0.5), "infinite z": dict(z_min=-math.inf, z_max=math.inf), "z both +inf": dict(z_min=math.inf),
    "ref_z unused": dict(use_ref_z=0, ref_z=math.nan), "max_step 0": dict(max_step=0.0), "min_neighbors 8": dict(min_neighbors=8),
    "label num_classes": dict(ignore=(CLASSES,), blocked=(0,), drivable=(CLASSES, 0)), "2048 x 2048": dict(width=2048, height=2048),
    "cell_voxels 8": dict(cell_voxels=8),
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
    """sicp_map_elevation by the header's rules, one row, one cell, one point at a time"""
    leaf, C = state["leaf_size"], state["num_classes"]
    W, H, B = p["width"], p["height"], p["cell_voxels"]
    inv = _f32(1.0) / _f32(leaf)
    vc = [int(math.floor(float(_f32(_f32(center[d]) * inv)))) for d in range(2)]
    x0 = math.floor(vc[0] / B) - W // 2
    y0 = math.floor(vc[1] / B) - H // 2
    lo, hi = _level(p["z_min"], inv, -(BIAS - 1), BIAS - 1), _level(p["z_max"], inv, -(BIAS - 1), BIAS - 1)
    vref = _level(p["ref_z"], inv, -BIAS, BIAS)
    nan = ref.NAN
    n = len(state["key"])

    def fullest(bins):
        best = 0
        for l in range(1, len(bins)):
            if bins[l] > bins[best]:
                best = l
        return best

    columns = {}  # cell -> level -> map rows, ascending
    for r in range(n):
        k = int(state["key"][r])
        vx, vy, vz = (k & 0x1FFFFF) - BIAS, ((k >> 21) & 0x1FFFFF) - BIAS, (k >> 42) - BIAS
        if int(state["count"][r]) < p["min_count"] or vz < lo or vz > hi:
            continue
        i, j = math.floor(vx / B) - x0, math.floor(vy / B) - y0
        if i < 0 or i >= W or j < 0 or j >= H:
            continue
        if len(p["ignore"]) and fullest([int(b) for b in state["hist"][r]]) in [int(l) for l in p["ignore"]]:
            continue
        columns.setdefault(j * W + i, {}).setdefault(vz, []).append(r)

    out = {name: np.zeros(W * H, dt) for name, dt in ref.CELL_ARRAYS}
    for c in range(W * H):
        for name in ("elevation", "bottom", "ceiling"):
            out[name][c] = nan
    for c, levels in columns.items():
        runs = []
        for l in sorted(levels):
            if runs and l - runs[-1][-1] <= p["clearance_voxels"]:
                runs[-1].append(l)
            else:
                runs.append([l])
        k = 0
        if p["use_ref_z"]:
            for q, run in enumerate(runs):
                if run[0] <= vref:
                    k = q

        def mean(l):
            S, N = 0.0, 0
            for r in levels[l]:
                S = S + float(state["sums"][r][2])
                N += int(state["count"][r])
            return _f32(S / float(N)), N

        t, b = runs[k][-1], runs[k][0]
        out["state"][c] = 1
        out["elevation"][c], out["count"][c] = mean(t)
        out["bottom"][c] = mean(b)[0]
        out["ceiling"][c] = mean(runs[k + 1][0])[0] if k + 1 < len(runs) else _f32(math.inf)
        if C > 0:
            bins = [0] * (C + 1)
            for r in levels[t]:
                for l in range(C + 1):
                    bins[l] += int(state["hist"][r][l])
            out["label"][c] = fullest(bins)
        out["level_top"][c], out["level_bottom"][c], out["n_levels"][c] = t, b, len(runs[k])

    n_class = [0] * 8
    for j in range(H):
        for i in range(W):
            c = j * W + i
            if not out["state"][c]:
                out["step"][c] = nan
                n_class[0] += 1
                continue
            e = out["elevation"][c]
            step, nb = _f32(0.0), 0
            for dj in (-1, 0, 1):
                for di in (-1, 0, 1):
                    ni, nj = i + di, j + dj
                    if (di or dj) and 0 <= ni < W and 0 <= nj < H and out["state"][nj * W + ni]:
                        nb += 1
                        d = abs(_f32(out["elevation"][nj * W + ni] - e))
                        if d > step:
                            step = d
            out["step"][c], out["neighbors"][c] = step, nb
            label, ceiling = int(out["label"][c]), out["ceiling"][c]
            if (len(p["blocked"]) and label in [int(l) for l in p["blocked"]]) or \
                    (len(p["drivable"]) and label not in [int(l) for l in p["drivable"]]):
                cls = 2
            elif int(out["level_top"][c]) - int(out["level_bottom"][c]) > p["max_extent_voxels"]:
                cls = 3
            elif p["min_clearance"] > 0 and math.isfinite(float(ceiling)) and float(_f32(ceiling - e)) < p["min_clearance"]:
                cls = 4
            elif float(step) > p["max_step"]:
                cls = 5
            elif nb < p["min_neighbors"]:
                cls = 6
            else:
                cls = 1
            out["cell_class"][c] = cls
            n_class[cls] += 1

    n_points = 0
    if points is not None:
        M = np_ref.qt_to_mat(np.array([0, 0, 0, 1, 0, 0, 0.0]) if qt is None else qt)
        n_points = len(points)
        pc, ph = np.full(n_points, -1, np.int32), np.full(n_points, nan, np.float32)
        for g in range(n_points):
            x, y, z = (float(a) for a in points[g])
            if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
                continue
            with np.errstate(over="ignore"):
                q = [_f32(((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]) for a in range(3)]
                v = [float(np.floor(_f32(q[a] * inv))) for a in range(3)]
            if not all(abs(a) < BIAS for a in v):
                continue
            i, j = math.floor(v[0] / B) - x0, math.floor(v[1] / B) - y0
            if i < 0 or i >= W or j < 0 or j >= H:
                continue
            pc[g] = j * W + i
            if out["state"][pc[g]]:
                ph[g] = _f32(q[2] - out["elevation"][pc[g]])
        out["point_cell"], out["point_height"] = pc, ph
    for name, _ in ref.CELL_ARRAYS:
        out[name] = out[name].reshape(H, W)
    out["info"] = dict(n_voxels=n, n_points=n_points, x0=x0, y0=y0, width=W, height=H, n_class=n_class, cell_size=B * leaf)
    return out
