"""Inputs of the tests of sicp_map_merge and the map's state calls (tests/test_map_merge_cpu.py on the restatement,
tests/test_gpu_map_merge.py through the library).  A case is (src, dst, keywords of map_merge_ref.merge): two restatement maps
built by integrating small scans, and the merge's pose, min_count and crop.  Cases are built once; case(name) hands out copies,
so a test may merge into what it gets.

general   the four posed scans of map_cases (NaN rows) split between src and dst, leaf pairs 0.2 -> 0.2, 0.1 -> 0.4 (runs of many
          rows) and 0.4 -> 0.1, a general pose; dst empty, or holding the fourth scan (overlapping) and a far lattice (disjoint)
edges     lattices: every touched voxel new and below / above / between dst's keys, none new, kept rows = touched voxels = 63,
          64, 65, 255, 256, 257, one src row, and ~300 src rows of leaf 0.01 into one dst voxel of leaf 8
classes   C = 1, 63, 64, 255 (histogram strides 2, 64, 65, 256), and a src with classes into a dst without
crop      some rows dropped by min_count and the crop; all rows dropped by either"""
from __future__ import annotations

import functools

import numpy as np

import map_cases
import map_merge_ref
import map_ref
import np_ref
import synth

LEAF, CLASSES = map_cases.LEAF, map_cases.CLASSES
EDGE_COUNTS = (63, 64, 65, 255, 256, 257)
LEAF_PAIRS = ((0.2, 0.2), (0.1, 0.4), (0.4, 0.1))
CLASS_COUNTS = (1, 63, 64, 255)
HALF_TURN = np.array([0.0, 0.0, 1.0, 0.0, 1.0, -0.5, 0.25])  # q = (0, 0, 1, 0): exactly diag(-1, -1, 1); t = (4, -2, 1) voxels of 0.25
EXACT_LEAF, EXACT_CLASSES = 0.25, 3


def pose(degrees, axis, t):
    return np_ref.mat_to_qt(synth.pose_matrix(degrees, axis, t))


GENERAL_POSE = pose(17.0, (0.2, -0.1, 1.0), (0.7, -1.3, 0.4))
SHIFT_Y = np.array([0, 0, 0, 1, 0.0, 2 * LEAF, 0.0])  # two voxels of LEAF along y


def _map(scans, leaf=LEAF, num_classes=CLASSES, qts=None):
    return map_cases.build(scans, qts, leaf=leaf, num_classes=num_classes)


def _row(n, z=5, y=0, x0=0, step=1):
    return [[x0 + step * i, y, z] for i in range(n)]


def _uniform(seed, n, num_classes, lo=-3.0, hi=3.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32), rng.integers(0, num_classes + 1, n).astype(np.uint32)


def _general(leaf_src, leaf_dst, full):
    scans, qts = map_cases.four_posed()
    src = _map(scans[:3], leaf_src, qts=qts[:3])
    far = map_cases.lattice(_row(50, z=40), 2, leaf=leaf_dst, seed=5, label=3)
    dst = _map([scans[3], far], leaf_dst, qts=[qts[3], None]) if full else map_ref.Map(leaf_dst, CLASSES)
    return src, dst, dict(qt=GENERAL_POSE)


def _edge(name):
    L = map_cases.lattice
    if name in ("below", "above"):  # z is the key's highest field
        return _map([L(_row(30, z=-3 if name == "below" else 9, y=-2), 3, label=2)]), _map([L(_row(40, y=0), 2)]), dict(qt=SHIFT_Y)
    if name == "between":
        return _map([L(_row(30, x0=1, step=2), 3, label=2)]), _map([L(_row(40, step=2), 2)]), dict(qt=None)
    if name == "none_new":
        return _map([L(_row(25, x0=7, y=-2), 3, label=2)]), _map([L(_row(40), 2)]), dict(qt=SHIFT_Y)
    if name == "one_row":
        return _map([L([[3, -2, 5]], 4, label=4)]), _map([L(_row(40), 2)]), dict(qt=SHIFT_Y)
    if name == "long_run":  # ~300 rows of leaf 0.01 land in dst's voxel (0, 0, 0) of leaf 8, which holds five points already
        xyz, lab = _uniform(11, 300, CLASSES, 1.0, 2.0)
        src = _map([(xyz, lab)], 0.01)
        dst = _map([map_cases.lattice([[0, 0, 0]], 5, leaf=8.0, seed=3), map_cases.lattice(_row(10, z=2), 1, leaf=8.0, seed=4)], 8.0)
        return src, dst, dict(qt=pose(25.0, (1.0, 0.3, -0.2), (2.5, 3.0, 1.5)))
    n = int(name[1:])  # "n63" ...: n kept rows into n touched voxels, the upper half of them new
    return _map([L(_row(n, y=-2), 2, seed=1, label=2)]), _map([L(_row(n, x0=-(n // 2)), 1, seed=2)]), dict(qt=SHIFT_Y)


def _classes(C, dst_classes=None):
    src = _map([_uniform(21, 500, C), _uniform(22, 500, C)], num_classes=C)
    dst = _map([_uniform(23, 500, C)], num_classes=C if dst_classes is None else dst_classes)
    return src, dst, dict(qt=GENERAL_POSE)


def _crop(name):
    src, dst, kw = _general(0.2, 0.2, True)
    if name == "crop_min":
        kw.update(min_count=2, center=(0.5, -1.0, 0.3), crop_range=2.5)
    elif name == "all_dropped_min":
        kw.update(min_count=1000)
    else:
        kw.update(center=(500.0, 0.0, 0.0), crop_range=1.0)
    return src, dst, kw


GENERAL = tuple(f"g_{a}_{b}_{'full' if full else 'empty'}" for a, b in LEAF_PAIRS for full in (False, True))
EDGES = ("below", "above", "between", "none_new", "one_row", "long_run") + tuple(f"n{n}" for n in EDGE_COUNTS)
CLASSED = tuple(f"c{C}" for C in CLASS_COUNTS) + ("c_dst0",)
CROPPED = ("crop_min", "all_dropped_min", "all_dropped_crop")
ALL = GENERAL + EDGES + CLASSED + CROPPED


@functools.lru_cache(maxsize=None)
def _built(name):
    if name in GENERAL:
        _, a, b, full = name.split("_")
        return _general(float(a), float(b), full == "full")
    if name in EDGES:
        return _edge(name)
    if name == "c_dst0":
        return _classes(CLASSES, 0)
    if name in CLASSED:
        return _classes(int(name[1:]))
    if name in CROPPED:
        return _crop(name)
    raise KeyError(name)


def case(name):
    """(src, dst, merge keywords): fresh copies of the case's two restatement maps"""
    src, dst, kw = _built(name)
    return map_merge_ref.copy_of(src), map_merge_ref.copy_of(dst), dict(kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the merged dst's state, the merge's info) by the restatement; read-only"""
    src, dst, kw = case(name)
    info = map_merge_ref.merge(dst, src, **kw)
    st = map_merge_ref.state(dst)
    for v in st.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return st, info


# ---- the exact scene: an oracle that does not go through the restatement of the merge ---------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_scans():
    """three scans of 1500 points at (k + 0.5) * 2^-10, never on a face of the 0.25 grid, labels 1..3, and their poses INSIDE the
    submap: identities and one translation by whole voxels.  With a few points a voxel every sum is exact in double."""
    rng = np.random.default_rng(77)
    scans = []
    for _ in range(3):
        k = rng.integers(-1024, 1024, (1500, 3))
        xyz = ((k + 0.5) / 1024.0).astype(np.float32)
        lab = rng.integers(1, EXACT_CLASSES + 1, 1500).astype(np.uint32)
        xyz.setflags(write=False)
        lab.setflags(write=False)
        scans.append((xyz, lab))
    inner = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0.5, 0.25, -0.25]], dtype=np.float64)
    return tuple(scans), inner


def exact_composed():
    """the poses of the scans in dst's frame: HALF_TURN after the inner pose -- rotation diag(-1, -1, 1), so t = R t_inner + t"""
    _, inner = exact_scans()
    out = np.tile(HALF_TURN, (len(inner), 1))
    out[:, 4:] = inner[:, 4:] * np.array([-1.0, -1.0, 1.0]) + HALF_TURN[4:]
    return out
