"""Inputs of the voxel map's tests (tests/test_map_cpu.py on the restatement, tests/test_gpu_map.py through the library).

four()        4 scans of 1500 uniform points in [-3, 3]^3, labels 1..4, leaf 0.5: ~1700 voxels of at most a dozen points, every
              voxel seen by several scans -- the input on which the chained merge loses centroids and labels
four_posed()  the same with 3 % NaN rows, poses along merge_cases.track and a crop of 3.2 about CENTER
References are computed once and are read-only."""
from __future__ import annotations

import functools

import numpy as np

import map_ref
import merge_cases
import merge_ref

LEAF, CLASSES = 0.5, 4
CENTER, RANGE = (0.3, -0.2, 0.1), 3.2


@functools.lru_cache(maxsize=None)
def four(bad=0.0):
    rng = np.random.default_rng(2026)
    scans = []
    for _ in range(4):
        xyz = rng.uniform(-3, 3, (1500, 3)).astype(np.float32)
        lab = rng.integers(1, CLASSES + 1, 1500).astype(np.uint32)
        rows = rng.choice(1500, int(round(bad * 1500)), replace=False)
        xyz[rows, rng.integers(0, 3, len(rows))] = np.nan
        xyz.setflags(write=False)
        lab.setflags(write=False)
        scans.append((xyz, lab))
    return tuple(scans)


def four_posed():
    return four(0.03), merge_cases.track(4)


def unlabelled(scans):
    return [(xyz, None) for xyz, _ in scans]


def build(scans, qts=None, leaf=LEAF, num_classes=CLASSES, center=(0.0, 0.0, 0.0), crop_range=0.0, cls=map_ref.Map):
    """the restatement's map after integrating `scans` in order"""
    m = cls(leaf, num_classes)
    for i, (xyz, lab) in enumerate(scans):
        m.integrate(xyz, lab, None if qts is None else qts[i], center, crop_range)
    return m


@functools.lru_cache(maxsize=None)
def reference(posed, labelled, crop):
    """(the map's extract, merge_ref.merge of the same scans) for the four scans: plain or posed, with or without labels and crop"""
    scans, qts = four_posed() if posed else (four(), None)
    parts = list(scans) if labelled else unlabelled(scans)
    rng = RANGE if crop else 0.0
    got = build(parts, qts, num_classes=CLASSES if labelled else 0, center=CENTER, crop_range=rng).extract()
    want = merge_ref.merge(parts, qts, LEAF, CENTER, rng)
    for d in (got, want):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return got, want


def lattice(cells, per_cell=1, leaf=LEAF, seed=0, label=1):
    """per_cell points strictly inside each voxel of `cells` ([n, 3] integer voxel coordinates), in the order given: a scan whose
    voxels are exactly those"""
    rng = np.random.default_rng(seed)
    cells = np.repeat(np.asarray(cells, dtype=np.int64).reshape(-1, 3), per_cell, axis=0)
    xyz = ((cells + rng.uniform(0.2, 0.8, cells.shape)) * leaf).astype(np.float32)
    return xyz, np.full(len(xyz), label, np.uint32)
