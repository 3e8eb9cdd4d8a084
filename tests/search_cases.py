"""Inputs of the search edge tests (tests/test_gpu_search_edges.py, tests/test_search_edges_cpu.py): clouds on which an exact
k-NN search can go wrong without a LiDAR-like cloud noticing -- equal distances across the k-th / (k+1)-th cut, degenerate
boxes, many points with one curve code, label segments of a few points -- and a numpy restatement of the search.  Every
generator is seeded and returns float32; the caller's point order is shuffled, so the caller index is never the curve order.
numpy only: no library, no GPU."""
from __future__ import annotations

import functools

import numpy as np

import synth

KS = (1, 4, 20, 32)                      # the list lengths of the search kernels
SEGMENT_SIZES = (1, 2, 15, 16, 17, 20, 21, 63, 64, 65, 257, 1025)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _shuffled(p, seed):
    p = _f32(p)
    return p[np.random.default_rng(seed).permutation(len(p))]


# ---- numpy restatement ----------------------------------------------------------------------------------------------------
def np_knn(q, t, k, chunk=256):
    """k nearest targets of every query: float32 ((dx*dx)+dy*dy)+dz*dz, every product and sum rounded on its own, ordered by
    (distance, lower index) with np.lexsort; -1 / +inf past the end of a target shorter than k"""
    q, t = _f32(q), _f32(t)
    nq, nt = len(q), len(t)
    idx = np.full((nq, k), -1, dtype=np.int32)
    d2 = np.full((nq, k), np.inf, dtype=np.float32)
    m = min(k, nt)
    for a in range(0, nq, chunk):
        dx = q[a:a + chunk, None, 0] - t[None, :, 0]
        dy = q[a:a + chunk, None, 1] - t[None, :, 1]
        dz = q[a:a + chunk, None, 2] - t[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        assert d.dtype == np.float32
        index = np.broadcast_to(np.arange(nt), d.shape)
        order = np.lexsort((index, d), axis=-1)[:, :m]
        idx[a:a + chunk, :m] = order
        d2[a:a + chunk, :m] = np.take_along_axis(d, order, axis=1)
    return idx, d2


def tie_share(d2_k_plus_1, k):
    """share of the rows of a (k + 1)-list whose k-th and (k + 1)-th distances are equal"""
    return float((d2_k_plus_1[:, k - 1] == d2_k_plus_1[:, k]).mean())


# ---- the integer lattice ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice(n=17):
    """the n^3 points (i, j, k), 0 <= i, j, k < n: every distance is an exact small integer, ties everywhere"""
    r = np.arange(n)
    k, j, i = np.meshgrid(r, r, r, indexing="ij")
    return _shuffled(np.stack([i.ravel(), j.ravel(), k.ravel()], 1), 100 + n)


@functools.lru_cache(maxsize=None)
def cell_centres(n=17):
    """the (n - 1)^3 cell centres of lattice(n): eight targets at d^2 = 0.75 exactly"""
    r = np.arange(n - 1) + 0.5
    k, j, i = np.meshgrid(r, r, r, indexing="ij")
    return _shuffled(np.stack([i.ravel(), j.ravel(), k.ravel()], 1), 200 + n)


@functools.lru_cache(maxsize=None)
def face_centres(n=17):
    """the centres of the cells' faces, all three orientations: four targets at d^2 = 0.5 exactly"""
    h, w = np.arange(n - 1) + 0.5, np.arange(n).astype(np.float64)
    out = []
    for axis in range(3):
        g = np.meshgrid(*[w if a == axis else h for a in range(3)], indexing="ij")
        out.append(np.stack([c.ravel() for c in g], 1))
    return _shuffled(np.concatenate(out), 300 + n)


# ---- one generator per geometry: name -> (target, {query set name: queries}); the set named "self" is the target ------------
def _lattice_case():
    t = lattice(17)
    return t, {"self": t, "cells": cell_centres(17), "faces": face_centres(17)}


def _duplicates_case():
    """40 positions x 100 copies: every position fills more than one 64-point leaf group with one point"""
    rng = np.random.default_rng(31)
    pos = rng.uniform(-5, 5, (40, 3)).astype(np.float32)
    t = _shuffled(np.repeat(pos, 100, axis=0), 32)
    near = (pos[rng.integers(0, 40, 600)] + rng.normal(0, 0.3, (600, 3))).astype(np.float32)
    return t, {"self": t, "near": near}


def _line_case():
    """3000 points at integer x on the x axis; the queries (i + 0.5, 1, 0) are d^2 = 1.25 from points i and i + 1"""
    x = np.arange(3000, dtype=np.float64)
    t = _shuffled(np.stack([x, 0 * x, 0 * x], 1), 33)
    q = _shuffled(np.stack([x[:-1] + 0.5, 0 * x[:-1] + 1, 0 * x[:-1]], 1), 34)
    return t, {"self": t, "between": q}


def _plane_case():
    """a 64 x 64 integer grid at z = 0; the queries hover over the cell centres (four targets at d^2 = 0.5625)"""
    r = np.arange(64, dtype=np.float64)
    j, i = np.meshgrid(r, r, indexing="ij")
    t = _shuffled(np.stack([i.ravel(), j.ravel(), 0 * i.ravel()], 1), 35)
    h = r[:-1] + 0.5
    j, i = np.meshgrid(h, h, indexing="ij")
    q = _shuffled(np.stack([i.ravel(), j.ravel(), 0 * i.ravel() + 0.25], 1), 36)
    return t, {"self": t, "centres": q}


def _needle_case():
    """x in [0, 1e4], y and z in [0, 1e-3]: every point quantizes to curve cell 0 on two axes"""
    rng = np.random.default_rng(37)
    scale = np.array([1e4, 1e-3, 1e-3])
    t = (rng.uniform(0, 1, (5000, 3)) * scale).astype(np.float32)
    q = (rng.uniform(-0.02, 1.02, (1500, 3)) * scale).astype(np.float32)
    return t, {"self": t, "around": q}


def _one_cell_case():
    """5000 points inside a cube of 1e-6 x the cloud's extent (one cell of the 21-bit curve grid is 4.8e-7 of it: the leaves of
    these points share their first curve code up to a handful of cells) and 3000 spread over 100 m"""
    rng = np.random.default_rng(38)
    corner = np.array([37.0, 61.0, 12.0])
    dense = corner + rng.uniform(0, 1e-4, (5000, 3))
    wide = rng.uniform(0, 100, (3000, 3))
    t = _shuffled(np.concatenate([dense, wide]), 39)
    q = np.concatenate([corner + rng.uniform(-1e-4, 2e-4, (1000, 3)), rng.uniform(0, 100, (1000, 3))])
    return t, {"self": t, "mixed": _shuffled(q, 40)}


def _offset_case():
    """a LiDAR-like pair of 6000 points translated by (65536, -131072, 32768): float32 spacing of 1/128 .. 1/64 m"""
    src, _, tgt, _, _, _ = synth.lidar_pair(seed=4, n_points=6000)
    off = np.array([65536.0, -131072.0, 32768.0])
    t = (tgt.astype(np.float64) + off).astype(np.float32)
    q = (src.astype(np.float64) + off).astype(np.float32)
    return _shuffled(t, 41), {"self": None, "source": _shuffled(q, 42)}


def _denormal_case():
    """64 points 1e-20 apart on x (their float32 d^2 = m^2 1e-40 is denormal up to m = 10) among 1000 ordinary ones"""
    rng = np.random.default_rng(43)
    m = np.arange(64, dtype=np.float64)
    close = np.stack([m * 1e-20, 0 * m, 0 * m], 1)
    t = _shuffled(np.concatenate([close, rng.uniform(-3, 3, (1000, 3))]), 44)
    probe = np.stack([(m + 0.5) * 1e-20, 0 * m, 0 * m], 1)
    return t, {"self": t, "probe": _f32(probe)}


def _outside_case():
    """the target in the unit cube, the queries 100 away on every side: beyond every face, edge and corner of the root box"""
    rng = np.random.default_rng(45)
    t = rng.uniform(0, 1, (2000, 3)).astype(np.float32)
    dirs = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)], dtype=np.float64)
    q = rng.uniform(0, 1, (26 * 20, 3)) + 100.0 * np.repeat(dirs, 20, axis=0)
    return t, {"far": _shuffled(q, 46)}


_GENERATORS = dict(lattice=_lattice_case, duplicates=_duplicates_case, line=_line_case, plane=_plane_case, needle=_needle_case,
                   one_cell=_one_cell_case, offset=_offset_case, denormal=_denormal_case, outside=_outside_case)
# (case, query set) of every geometry, in a fixed order: the parameters of the tests
QUERY_SETS = (("lattice", "self"), ("lattice", "cells"), ("lattice", "faces"), ("duplicates", "self"), ("duplicates", "near"),
              ("line", "self"), ("line", "between"), ("plane", "self"), ("plane", "centres"), ("needle", "self"),
              ("needle", "around"), ("one_cell", "self"), ("one_cell", "mixed"), ("offset", "self"), ("offset", "source"),
              ("denormal", "self"), ("denormal", "probe"), ("outside", "far"))
SELF_CASES = tuple(c for c, s in QUERY_SETS if s == "self")


@functools.lru_cache(maxsize=None)
def case(name):
    """(target, {query set: queries}) of one geometry"""
    t, qs = _GENERATORS[name]()
    qs = {k: (t if v is None else v) for k, v in qs.items()}
    return t, qs


def queries(name, qset):
    t, qs = case(name)
    return qs[qset], t


# ---- label segments ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def segments():
    """two labelled clouds whose label segments have the sizes SEGMENT_SIZES (label l has SEGMENT_SIZES[l - 1] target points
    and the size five places on in the source, so small source segments meet large target segments and the other way round);
    label 13 has 30 source points and no target point, label 14 has 40 target points and no source point.
    Returns src, src_labels, tgt, tgt_labels."""
    rng = np.random.default_rng(47)
    n = len(SEGMENT_SIZES)
    centre = rng.uniform(-20, 20, (n + 2, 3))
    src, sl, tgt, tl = [], [], [], []
    for l in range(1, n + 1):
        nt, ns = SEGMENT_SIZES[l - 1], SEGMENT_SIZES[(l - 1 + 5) % n]
        tgt.append(centre[l - 1] + rng.normal(0, 2.0, (nt, 3))); tl += [l] * nt
        src.append(centre[l - 1] + rng.normal(0, 2.0, (ns, 3))); sl += [l] * ns
    src.append(centre[n] + rng.normal(0, 2.0, (30, 3))); sl += [n + 1] * 30
    tgt.append(centre[n + 1] + rng.normal(0, 2.0, (40, 3))); tl += [n + 2] * 40
    src, tgt = _f32(np.concatenate(src)), _f32(np.concatenate(tgt))
    sl, tl = np.array(sl, dtype=np.uint32), np.array(tl, dtype=np.uint32)
    ps, pt = rng.permutation(len(src)), rng.permutation(len(tgt))
    return src[ps], sl[ps], tgt[pt], tl[pt]


# ---- tree shapes ------------------------------------------------------------------------------------------------------------
TREE_TARGETS = (1, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16385, 65537)
TREE_SOURCES = (1, 15, 16, 17, 63, 65, 1000)
SELF_SIZES = (1, 15, 16, 17, 19, 20, 21, 63, 64, 65, 255, 256, 257, 1025, 4097)
K_COVS = (1, 2, 4, 5, 20, 21, 32)
HEIGHT9_POINTS = 16 * 4 ** 8 + 16        # one leaf more than a tree of height 8 holds
TALL_TREES = (16 * 4 ** 7 + 16, HEIGHT9_POINTS)   # heights 8 and 9: the third round trip of the path phase starts at 9


def tree_height(n):
    """height `top` of the search tree over n points: 4^top leaves of 16 points hold them"""
    leaves, top = max(1, -(-n // 16)), 0
    while 4 ** top < leaves:
        top += 1
    return top


def tree_sources(n_t):
    """the two source sizes paired with a target size"""
    i = TREE_TARGETS.index(n_t)
    return TREE_SOURCES[i % 7], TREE_SOURCES[(i + 3) % 7]


@functools.lru_cache(maxsize=None)
def uniform_cloud(n, seed, side=10.0):
    return np.random.default_rng(seed).uniform(0, side, (n, 3)).astype(np.float32)


def sources_under(M, n, seed, side=10.0):
    """n source points that the 4 x 4 pose M carries into and a little around the cube of uniform_cloud()"""
    q = np.random.default_rng(seed).uniform(-0.1 * side, 1.1 * side, (n, 3))
    return _f32((q - M[:3, 3]) @ M[:3, :3])
