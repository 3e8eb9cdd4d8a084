"""Inputs of the free-space carving tests (tests/test_map_carve_cpu.py on the restatement, tests/test_gpu_map_carve.py through
the library).

fifth()          a fifth 1500-point scan for the map of map_cases.four(): uniform in [-3, 3]^3, so rays from ORIGIN cross the
                 whole map; with bad > 0 a share of NaN rows
general_rays()   seeded rays in general position: (leaf, origins, returns)
HAND             rays whose walk is known by hand: name -> (origin, return, end_margin, the voxels v_0 .. v_n); leaf 0.5, so
                 the grid's 1 / leaf is the exact 2
box_map()        a scan with one point in every voxel of [-6, 6]^3: on that map a dry run's miss counts ARE the visited voxels
scene()          a wall, a ground plane and a "car" that stands in scans 1 - 2 and has driven off in scan 3
References are computed once and are read-only."""
from __future__ import annotations

import functools

import numpy as np

import map_cases
import map_carve_ref
import map_ref
import merge_cases

LEAF, CLASSES = map_cases.LEAF, map_cases.CLASSES
ORIGIN = (0.3, -0.4, 0.2)


@functools.lru_cache(maxsize=None)
def fifth(bad=0.0):
    rng = np.random.default_rng(2027)
    xyz = rng.uniform(-3, 3, (1500, 3)).astype(np.float32)
    lab = rng.integers(1, CLASSES + 1, 1500).astype(np.uint32)
    rows = rng.choice(1500, int(round(bad * 1500)), replace=False)
    xyz[rows, rng.integers(0, 3, len(rows))] = np.nan
    xyz.setflags(write=False)
    lab.setflags(write=False)
    return xyz, lab


def pose():
    """the fifth pose of merge_cases.track: a rotation about a skew axis and a translation"""
    return merge_cases.track(5)[4]


def four_map():
    """the restatement's map of map_cases.four(): 1676 voxels at leaf 0.5 (a fresh one: carve changes it)"""
    return map_cases.build(map_cases.four())


@functools.lru_cache(maxsize=None)
def general_rays():
    rng = np.random.default_rng(0)
    out = []
    for n, half, leaf in ((300, 2.0, 0.5), (100, 1.5, 0.2)):
        o = rng.uniform(-half, half, (n, 3)).astype(np.float32)
        p = rng.uniform(-half, half, (n, 3)).astype(np.float32)
        o.setflags(write=False)
        p.setflags(write=False)
        out.append((leaf, o, p))
    return tuple(out)


def _line(start, axis, step, n):
    v = list(start)
    out = [tuple(v)]
    for _ in range(n):
        v[axis] += step
        out.append(tuple(v))
    return out


def _hand():
    H = {}
    c = (0.25, 0.25, 0.25)  # the middle of voxel (0, 0, 0)
    for axis, name in enumerate("xyz"):
        for sign in (+1, -1):
            p = list(c)
            p[axis] += sign * 1.5  # three voxels along the axis
            H[f"{'+' if sign > 0 else '-'}{name}"] = (c, tuple(p), 0, _line((0, 0, 0), axis, sign, 3))
    # the exact diagonal: the three tmax are equal at every step, so the order is x, y, z repeated
    H["diagonal"] = (c, (1.75, 1.75, 1.75), 0,
                     [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)])
    H["zero_length"] = (c, (0.4, 0.1, 0.3), 0, [(0, 0, 0)])
    H["neighbour_margin1"] = (c, (0.75, 0.25, 0.25), 1, [(0, 0, 0), (1, 0, 0)])  # n = 1 <= end_margin: no candidate
    H["three_steps_margin3"] = (c, (1.75, 0.25, 0.25), 3, _line((0, 0, 0), 0, 1, 3))  # n = 3 <= end_margin
    H["four_steps_margin3"] = (c, (2.25, 0.25, 0.25), 3, _line((0, 0, 0), 0, 1, 4))   # one candidate: v_0
    # origin and return on voxel boundaries: u = 0, w = (2, 1, 0); tmax x = 0.5 then 1.0, tmax y = 1.0: x, x (the tie), y
    H["boundaries"] = ((0.0, 0.0, 0.0), (1.0, 0.5, 0.0), 0, [(0, 0, 0), (1, 0, 0), (2, 0, 0), (2, 1, 0)])
    # negative coordinates: from voxel (-1, -1, -1) down x to -4 and down y to -2; tmax x = 1/6, 1/2, 5/6, tmax y = 0.714
    H["negative"] = ((-0.25, -0.25, -0.25), (-1.75, -0.6, -0.25), 0,
                     [(-1, -1, -1), (-2, -1, -1), (-3, -1, -1), (-3, -2, -1), (-4, -2, -1)])
    return H


HAND = _hand()
BOX = 6


@functools.lru_cache(maxsize=None)
def box_map():
    """(xyz, labels): one point in every voxel of [-BOX, BOX]^3 at leaf 0.5, labels 1..CLASSES"""
    r = np.arange(-BOX, BOX + 1)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    xyz, _ = map_cases.lattice(cells, seed=21)
    lab = (np.arange(len(xyz)) % CLASSES + 1).astype(np.uint32)
    xyz.setflags(write=False)
    lab.setflags(write=False)
    return xyz, lab


def visited_on_box(m: map_ref.Map, miss):
    """the voxels of the box map whose miss count is not zero, as a set of tuples"""
    k = m.key[np.asarray(miss) > 0]
    B = map_ref.BIAS
    return {(int(a & 0x1fffff) - B, int((a >> 21) & 0x1fffff) - B, int((a >> 42) & 0x1fffff) - B) for a in k}


def seeded_rays(n, seed=5, half=2.9):
    rng = np.random.default_rng([seed, n])
    return rng.uniform(-half, half, (n, 3)).astype(np.float32)


# ---- the scene ----------------------------------------------------------------------------------------------------------------
GROUND, WALL, CAR = 1, 2, 3
SENSOR = (0.0, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def scene():
    """{"scans": three (xyz, labels) in the map's frame, "car_voxels": the voxels only the car occupies}.  The sensor stands at
    SENSOR.  Ground: z = 0.05 over [-6, 6]^2 (label 1); wall: x = 6.2, y in [-6, 6], z in [0, 3] (label 2); car: the surface of
    the box [2, 3] x [-0.5, 0.5] x [0.5, 1.5] (label 3), in scans 1 and 2 only.  Scan 3 has no ground returns in the strip
    x in [3.2, 6], |y| < 1.5 -- the ground the low wall rays graze -- so those ground voxels are seen through and not hit."""
    rng = np.random.default_rng(31)

    def ground(hole):
        g = np.stack(np.meshgrid(np.arange(-6, 6.01, 0.25), np.arange(-6, 6.01, 0.25), indexing="ij"), axis=-1).reshape(-1, 2)
        g = g + rng.uniform(-0.05, 0.05, g.shape)
        if hole:
            g = g[~((g[:, 0] > 3.2) & (np.abs(g[:, 1]) < 1.5))]
        return np.column_stack([g, np.full(len(g), 0.05)])

    def wall():
        w = np.stack(np.meshgrid(np.arange(-6, 6.01, 0.1), np.arange(0.02, 3.0, 0.1), indexing="ij"), axis=-1).reshape(-1, 2)
        w = w + rng.uniform(-0.02, 0.02, w.shape)
        return np.column_stack([np.full(len(w), 6.2), w])

    def car():
        u = rng.uniform(0, 1, (600, 3))
        face = rng.integers(0, 6, 600)
        for a in range(3):
            u[face == 2 * a, a] = 0.0
            u[face == 2 * a + 1, a] = 1.0
        return u * np.array([0.98, 0.98, 0.98]) + np.array([2.01, -0.49, 0.51])

    scans = []
    for k in range(3):
        parts = [(ground(k == 2), GROUND), (wall(), WALL)] + ([(car(), CAR)] if k < 2 else [])
        xyz = np.concatenate([p for p, _ in parts]).astype(np.float32)
        lab = np.concatenate([np.full(len(p), l) for p, l in parts]).astype(np.uint32)
        xyz.setflags(write=False)
        lab.setflags(write=False)
        scans.append((xyz, lab))
    v_car, _ = map_carve_ref.voxels_of(scans[0][0][scans[0][1] == CAR], LEAF)
    v_rest, _ = map_carve_ref.voxels_of(scans[0][0][scans[0][1] != CAR], LEAF)
    car_voxels = {tuple(v) for v in v_car.tolist()} - {tuple(v) for v in v_rest.tolist()}
    return dict(scans=tuple(scans), car_voxels=frozenset(car_voxels))


def scene_map():
    """the restatement's map after scans 1 and 2 of the scene (a fresh one)"""
    return map_cases.build(scene()["scans"][:2], num_classes=3)
