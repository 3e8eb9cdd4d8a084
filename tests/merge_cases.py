"""Inputs of the sicp_merge_clouds tests (tests/test_merge_cpu.py asserts their properties on the restatement's output,
tests/test_gpu_merge.py runs them through the library): parts of 255 / 256 / 257 / 1 / 3000 points -- the sizes straddle
the workgroup of 256 -- with 3 % non-finite rows and labels that include 0 and 0xFFFFFFFF, posed along a short track.

A case is {"parts": [(xyz float32 [n, 3], labels uint32 or None)], "qts": [n_parts, 7] or None, "leaf", "center",
"crop_range"}; reference(name) is tests/merge_ref.py on it, computed once and read-only."""
from __future__ import annotations

import functools

import numpy as np

import merge_ref
import np_ref
import synth

SIZES = (255, 256, 257, 1, 3000)
LABELS = np.array([0, 1, 7, 0xFFFFFFFF], dtype=np.uint32)
CENTER = (0.5, -0.25, 0.1)
FAR = 4  # index (in the five-part cases) of the part whose pose carries it out of every crop


def scan(seed, n, labelled=True, bad=0.03):
    """n points in a 12 x 12 x 2 m slab about the origin (negative coordinates, so negative voxels), `bad` of the rows with a
    NaN or an infinity in one coordinate (at least one row when n >= 30), labels drawn from LABELS"""
    rng = np.random.default_rng(seed)
    xyz = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(-1, 1, n)], axis=1).astype(np.float32)
    n_bad = int(round(bad * n)) if n >= 30 else 0
    rows = rng.choice(n, n_bad, replace=False)
    xyz[rows, rng.integers(0, 3, n_bad)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), n_bad)
    lab = LABELS[rng.integers(0, len(LABELS), n)] if labelled else None
    return xyz, lab


def track(n, far=None):
    """poses along a gentle curve: 0.4 m and 2 degrees a step; pose `far` is 100 m away"""
    qts = []
    for i in range(n):
        t = (0.4 * i, 0.05 * i * i, 0.01 * i) if i != far else (100.0, 3.0, 0.0)
        qts.append(np_ref.mat_to_qt(synth.pose_matrix(2.0 * i + 1.0, (0.1, -0.2, 1.0), t)))
    return np.stack(qts)


def _blob():
    """5500 points inside the voxel [0.2, 0.4)^3 of a 0.2 m grid, exactly half of them label 5 and half label 3 (a tie: 3 wins),
    and 500 scattered points in a second part"""
    rng = np.random.default_rng(77)
    xyz = rng.uniform(0.21, 0.39, (5500, 3)).astype(np.float32)
    lab = rng.permutation(np.repeat(np.array([5, 3], np.uint32), 2750))
    return [(xyz, lab), scan(78, 500, bad=0.0)]


def _crop_edge():
    """about the centre (1, 0, 0) with range 5: (4, 4, 0) lies at d^2 = 25 exactly and stays; its float32 neighbours outside go"""
    up = np.nextafter(np.float32(4), np.float32(9))
    xyz = np.array([[4, 4, 0], [up, 4, 0], [4, 4, 0.01], [1, 0, 5], [1, 0, np.nextafter(np.float32(5), np.float32(9))],
                    [-2, -4, 0], [1, 0, 0], [6.5, 0, 0]], dtype=np.float32)
    return [(xyz, np.arange(8, dtype=np.uint32))]


@functools.lru_cache(maxsize=None)
def case(name):
    five = [scan(100 + i, n) for i, n in enumerate(SIZES)]
    five = five[:3] + [five[4], five[3]]  # 255 256 257 3000 1: the one-point part last, the one that the crop loses whole
    if name == "one":
        return dict(parts=[scan(1, 3000)], qts=track(2)[1:], leaf=0.2, center=(0, 0, 0), crop_range=0.0)
    if name == "two":
        return dict(parts=[scan(2, 255), scan(3, 257)], qts=track(2), leaf=0.5, center=CENTER, crop_range=5.0)
    if name == "five":
        return dict(parts=five, qts=track(5, far=FAR), leaf=0.2, center=CENTER, crop_range=8.0)
    if name == "five_far_256":  # a whole workgroup's part is cropped away
        parts = [five[0], five[2], five[1]]
        return dict(parts=parts, qts=track(3, far=2), leaf=0.2, center=CENTER, crop_range=8.0)
    if name == "five_nocrop":
        return dict(parts=five, qts=track(5, far=FAR), leaf=0.2, center=CENTER, crop_range=0.0)
    if name == "five_inf":
        return dict(parts=five, qts=track(5, far=FAR), leaf=0.2, center=CENTER, crop_range=np.inf)
    if name == "five_leaf0":
        return dict(parts=five, qts=track(5, far=FAR), leaf=0.0, center=CENTER, crop_range=8.0)
    if name == "five_identity":
        return dict(parts=five, qts=None, leaf=0.3, center=(0, 0, 0), crop_range=0.0)
    if name == "blob":
        return dict(parts=_blob(), qts=None, leaf=0.2, center=(0, 0, 0), crop_range=0.0)
    if name == "crop_edge":
        return dict(parts=_crop_edge(), qts=None, leaf=0.0, center=(1, 0, 0), crop_range=5.0)
    if name == "unlabelled":
        return dict(parts=[scan(4, 257, labelled=False), scan(5, 300, labelled=False)], qts=track(2), leaf=0.25, center=CENTER, crop_range=6.0)
    raise KeyError(name)


NAMES = ("one", "two", "five", "five_far_256", "five_nocrop", "five_inf", "five_leaf0", "five_identity", "blob", "crop_edge", "unlabelled")


def run_ref(c, fn=merge_ref.merge):
    return fn(c["parts"], c["qts"], c["leaf"], c["center"], c["crop_range"])


@functools.lru_cache(maxsize=None)
def reference(name):
    out = run_ref(case(name))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
