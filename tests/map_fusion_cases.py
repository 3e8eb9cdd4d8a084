"""Inputs of the label-fusion tests (tests/test_map_fusion_cpu.py on the restatement, tests/test_gpu_map_fusion.py through the
library): map_cases.four() / four_posed() with seeded labels 0..C, a seeded diagonally dominant column-normalised confusion
matrix per C, and a fifth scan to relabel.  CLASS_COUNTS puts one C on each side of a wave's 64 lanes and of the bound up to
which the kernels stage log cm in LDS (64), and reaches the largest a map takes.  References are computed once and are
read-only."""
from __future__ import annotations

import functools

import numpy as np

import map_cases
import map_fusion_ref as F
import map_ref
import merge_cases

LEAF = map_cases.LEAF
CLASS_COUNTS = (1, 2, 4, 19, 64, 65, 255)
MIN_COUNTS = (1, 3)


@functools.lru_cache(maxsize=None)
def matrix(C, seed=7):
    """cm[r, s]: how often class s + 1 shows as label r + 1; every column sums to 1 and its diagonal entry is the largest"""
    rng = np.random.default_rng([seed, C])
    cm = rng.uniform(0.05, 1.0, (C, C)) + 2.0 * C * np.eye(C)
    cm = cm / cm.sum(axis=0, keepdims=True)
    cm.setflags(write=False)
    return cm


@functools.lru_cache(maxsize=None)
def scans(posed, C):
    """(scans, poses or None, centre, range): the four clouds with labels 0..C drawn afresh"""
    base, qts = map_cases.four_posed() if posed else (map_cases.four(), None)
    rng = np.random.default_rng([31, C, int(posed)])
    out = []
    for xyz, _ in base:
        lab = rng.integers(0, C + 1, len(xyz)).astype(np.uint32)
        lab.setflags(write=False)
        out.append((xyz, lab))
    return tuple(out), qts, map_cases.CENTER, (map_cases.RANGE if posed else 0.0)


@functools.lru_cache(maxsize=None)
def built(posed, C):
    """the restatement's map of the four scans (read-only by convention) and log cm"""
    sc, qts, center, rng = scans(posed, C)
    return map_cases.build(sc, qts, num_classes=C, center=center, crop_range=rng), F.log_matrix(matrix(C))


@functools.lru_cache(maxsize=None)
def reference(posed, C, min_count):
    """the restatement's extract_fused of the case, under the crop the scans were integrated with"""
    m, L = built(posed, C)
    _, _, center, rng = scans(posed, C)
    out = F.extract_fused(m, L, min_count, center, rng)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def probe(C, labelled=True):
    """(xyz, labels or None, pose): a fifth scan to relabel -- 2000 points a little wider than the map, 3 % NaN rows, a dozen
    points far outside every voxel and two beyond the key's range -- at a pose of its own"""
    rng = np.random.default_rng([57, C])
    xyz = rng.uniform(-3.6, 3.6, (2000, 3)).astype(np.float32)
    xyz[:12] += np.float32(60.0)
    xyz[12] = (1e7, 0.0, 0.0)
    xyz[13] = (0.0, -3e6, 0.5)
    rows = rng.choice(np.arange(14, 2000), 60, replace=False)
    xyz[rows, rng.integers(0, 3, len(rows))] = np.nan
    xyz[rows[:5], 0] = np.inf
    lab = rng.integers(0, C + 1, 2000).astype(np.uint32)
    xyz.setflags(write=False)
    lab.setflags(write=False)
    return xyz, (lab if labelled else None), merge_cases.track(5)[4]


def vote_unique(hist):
    """rows whose fullest bin is unique and not bin 0: where a majority vote is a statement about a class"""
    hist = np.asarray(hist, dtype=np.int64)
    top = hist.max(axis=1)
    return ((hist == top[:, None]).sum(axis=1) == 1) & (np.argmax(hist, axis=1) > 0)


# ---- the edge matrices and the vote's input (C = 4) -----------------------------------------------------------------------------
def zero_matrix():
    """mostly zeros: classes 3 and 4 only ever show as themselves, 1 and 2 are confused with each other -- a voxel that saw
    labels 3 and 4 (or 1 and 3 ...) has every class ruled out"""
    return np.array([[0.8, 0.3, 0.0, 0.0], [0.2, 0.7, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])


def twin_matrix():
    """columns 2 and 3 are the same numbers: their scores are the same bits, and the tie goes to class 2"""
    cm = np.array(matrix(4))
    cm[:, 2] = cm[:, 1]
    return cm


def vote_matrix(a=0.7, b=0.1):
    return np.full((4, 4), b) + (a - b) * np.eye(4)


@functools.lru_cache(maxsize=None)
def vote_scan():
    """300 voxels of 6 points whose labels come from 0 and two classes of the voxel's own: a score is a sum of at most two
    terms, so equal counts tie exactly (the sum commutes) and every other gap is wide"""
    rng = np.random.default_rng(91)
    cells = [[i % 20, i // 20, 1] for i in range(300)]
    xyz, _ = map_cases.lattice(cells, per_cell=6, seed=4)
    lab = np.empty(len(xyz), np.uint32)
    for i in range(300):
        pair = rng.choice(4, 2, replace=False) + 1
        lab[6 * i:6 * i + 6] = rng.choice(np.array([0, pair[0], pair[1]]), 6)
    xyz.setflags(write=False)
    lab.setflags(write=False)
    return xyz, lab


def score_sets():
    """(name, scores, evidence) of every row the GPU tests compare labels on: the extract cases (all voxels: min_count 3 selects
    among them), the relabelled probe with and without its own label at both min_counts, the edge matrices, the vote"""
    for posed in (False, True):
        for C in CLASS_COUNTS:
            m, L = built(posed, C)
            sc, added = F.scores(m.hist, L)
            yield f"extract posed={int(posed)} C={C}", sc, F.posterior(sc, added)[2]
    for C in (4, 65):
        m, L = built(True, C)
        xyz, lab, qt = probe(C)
        for own in (False, True):
            for mc in MIN_COUNTS:
                sc, ev = probe_scores(m, L, xyz, lab, qt, own, mc)
                yield f"relabel C={C} own={int(own)} min_count={mc}", sc, ev
    m, _ = built(False, 4)
    for name, cm in (("zero", zero_matrix()), ("twin", twin_matrix())):
        sc, added = F.scores(m.hist, F.log_matrix(cm))
        yield name, sc, F.posterior(sc, added)[2]
    vm = map_cases.build([vote_scan()], num_classes=4)
    sc, added = F.scores(vm.hist, F.log_matrix(vote_matrix()))
    yield "vote", sc, F.posterior(sc, added)[2]


def probe_scores(m, L, xyz, lab, qt, include_own, min_count):
    """the scores behind map_fusion_ref.fused_labels for the finite points of a probe"""
    import merge_ref
    import np_ref
    xyz = np.asarray(xyz, dtype=np.float32)
    fin = np.isfinite(xyz).all(axis=1)
    p = np_ref.transform_points(np_ref.qt_to_mat(qt), xyz[fin])
    v = np.floor((p * (np.float32(1.0) / np.float32(m.leaf))).astype(np.float32))
    ok = (np.abs(v) < merge_ref.LIMIT).all(axis=1)
    hist = np.zeros((len(p), m.C + 1), np.uint32)
    k = map_ref.keys_of(v[ok].astype(np.int64))
    r = np.minimum(np.searchsorted(m.key, k), len(m.key) - 1)
    found = (m.key[r] == k) & (m.cnt[r] >= min_count)
    hist[np.flatnonzero(ok)[found]] = m.hist[r[found]]
    sc, added = F.scores(hist, L, lab[fin] if include_own else None)
    return sc, F.posterior(sc, added)[2]
