"""Inputs of the ray-casting tests (tests/test_map_raycast_cpu.py on the restatement, tests/test_gpu_map_raycast.py through the
library).

sparse_scans()   two scans of 800 points uniform in [-6, 6]^3, labels 1..4, leaf 0.5: the first alone gives 780 voxels of which
                 rays from map_carve_cases.ORIGIN hit some and pass the rest; the second puts a second point into some voxels,
                 so that min_count = 2 leaves enough opaque ones.  (map_cases.four() is too dense for a ray cast: every ray of
                 map_carve_cases.fifth() hits within a step or two and 6 rows are visible.)
sparse_ends()    1500 ends uniform in [-6, 6]^3
PARITY           the parameter sets of the parity tests: name -> (scans integrated, keywords)
scene_rays()     a 16 x 180 lidar pattern from map_carve_cases.SENSOR on the map of the scene's scans 1 - 2
References are computed once and are read-only."""
from __future__ import annotations

import functools
import importlib

import numpy as np

import map_carve_cases
import map_cases
import map_raycast_ref

LEAF, CLASSES = map_cases.LEAF, map_cases.CLASSES
ORIGIN = map_carve_cases.ORIGIN


@functools.lru_cache(maxsize=None)
def sparse_scans():
    out = []
    for seed in (41, 42):
        rng = np.random.default_rng(seed)
        xyz = rng.uniform(-6, 6, (800, 3)).astype(np.float32)
        lab = rng.integers(1, CLASSES + 1, 800).astype(np.uint32)
        xyz.setflags(write=False)
        lab.setflags(write=False)
        out.append((xyz, lab))
    return tuple(out)


def sparse_map(n_scans=1):
    """the restatement's map of the first n_scans sparse scans (a fresh one)"""
    return map_cases.build(sparse_scans()[:n_scans])


@functools.lru_cache(maxsize=None)
def sparse_ends(bad=0.0):
    rng = np.random.default_rng(43)
    xyz = rng.uniform(-6, 6, (1500, 3)).astype(np.float32)
    rows = rng.choice(1500, int(round(bad * 1500)), replace=False)
    xyz[rows, rng.integers(0, 3, len(rows))] = np.nan
    xyz.setflags(write=False)
    return xyz


# name -> (scans in the map, the keywords of the params)
PARITY = {
    "defaults": (1, dict()),
    "margin0": (1, dict(start_margin=0)),
    "margin3": (1, dict(start_margin=3)),
    "min_count2": (1, dict(min_count=2)),
    "min_count2_two_scans": (2, dict(min_count=2)),
    "ignore": (1, dict(ignore=(1, 3))),
    "ignore_bin0_range": (1, dict(ignore=(0, 4), max_range=2.5)),
    "ignore_bin0_range_two_scans": (2, dict(ignore=(0, 4), max_range=2.5)),
    "range4": (1, dict(max_range=4.0)),
}


# the one set that misses "at least 20 rays with a hit" on the one-scan map: the range leaves 61 rays, 18 of them hit.  It runs
# all the same; its twin on the two-scan map (28 hits, 33 without) is the one the condition holds for.
BELOW_CONDITION = ("ignore_bin0_range",)


@functools.lru_cache(maxsize=None)
def parity_reference(name):
    """the restatement's answer to sparse_ends() from ORIGIN under PARITY[name]"""
    n_scans, kw = PARITY[name]
    out = map_raycast_ref.raycast(sparse_map(n_scans), sparse_ends(), None, ORIGIN, map_raycast_ref.defaults(**kw))
    for k in map_raycast_ref.ARRAYS:
        out[k].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def scene_rays():
    sicp = importlib.import_module("semantic-icp_amd")
    ends = sicp.lidar_ray_ends(16, 180, -25.0, 15.0, 12.0, origin=map_carve_cases.SENSOR)
    ends.setflags(write=False)
    return ends


@functools.lru_cache(maxsize=None)
def scene_reference(ignore=()):
    out = map_raycast_ref.raycast(map_carve_cases.scene_map(), scene_rays(), None, map_carve_cases.SENSOR,
                                  map_raycast_ref.defaults(ignore=tuple(ignore)))
    for k in map_raycast_ref.ARRAYS:
        out[k].setflags(write=False)
    return out


def shell_map():
    """(xyz, labels) with one point in every voxel of the two outer layers of the cube [-3, 3]^3 of voxels: a shell two voxels
    thick around a sensor in the middle, of which only the inner layer can be seen"""
    r = np.arange(-3, 4)
    cells = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    ring = np.abs(cells).max(axis=1)
    cells = cells[ring >= 2]
    xyz, _ = map_cases.lattice(cells, seed=22)
    lab = (np.arange(len(xyz)) % CLASSES + 1).astype(np.uint32)
    return xyz, lab, cells
