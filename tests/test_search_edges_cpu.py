"""The inputs of tests/test_gpu_search_edges.py, checked without a GPU: the reference those tests compare with (the oracle's
plain brute force) agrees bit for bit with the oracle's kd-tree and with the numpy restatement on every case, and the
cases still hold what they were built for -- equal distances across the k-th / (k+1)-th cut, denormal distances, tree
heights, segment sizes -- so that a generator cannot quietly stop producing them."""
import numpy as np
import pytest

import oracle_lib as O
import search_cases as SC

NP_ROWS = 500      # rows compared with the numpy restatement (it forms the whole distance matrix)


def _rows(q):
    return q if len(q) <= NP_ROWS else q[np.linspace(0, len(q) - 1, NP_ROWS).astype(np.int64)]


@pytest.mark.parametrize("name,qset", SC.QUERY_SETS)
def test_brute_force_kdtree_and_numpy_agree(name, qset):
    q, t = SC.queries(name, qset)
    qs = _rows(q)
    for k in SC.KS:
        bi, bd = O.knn(q, t, k, kdtree=False)
        ki, kd = O.knn(q, t, k, kdtree=True)
        assert np.array_equal(bi, ki) and np.array_equal(bd, kd), k
        si, sd = O.knn(qs, t, k, kdtree=False)
        ni, nd = SC.np_knn(qs, t, k)
        assert np.array_equal(si, ni) and np.array_equal(sd, nd), k
        assert (bi >= 0).all() and (np.diff(bd, axis=1) >= 0).all()


def test_numpy_restatement_past_the_end_of_a_short_target():
    t = SC.uniform_cloud(19, 1)
    bi, bd = O.knn(t, t, 20, kdtree=False)
    ni, nd = SC.np_knn(t, t, 20)
    assert np.array_equal(bi, ni) and np.array_equal(bd, nd)
    assert (ni[:, 19] == -1).all() and np.isinf(nd[:, 19]).all() and (np.sort(ni[:, :19], axis=1) == np.arange(19)).all()


@pytest.mark.parametrize("name,qset,k,least", [
    ("lattice", "self", 4, 0.99), ("lattice", "self", 20, 0.99), ("lattice", "self", 32, 0.75),
    ("lattice", "cells", 1, 1.0), ("lattice", "cells", 4, 1.0),
    ("duplicates", "self", 1, 1.0), ("duplicates", "self", 4, 1.0), ("duplicates", "self", 20, 1.0), ("duplicates", "self", 32, 1.0),
    ("line", "between", 1, 1.0)])
def test_share_of_rows_with_a_tie_across_the_cut(name, qset, k, least):
    q, t = SC.queries(name, qset)
    _, d = O.knn(q, t, k + 1, kdtree=False)
    share = SC.tie_share(d, k)
    print(f"{name}/{qset} k={k}: tie share {share:.4f}")
    assert share >= least


def test_exact_distances_of_the_lattice_queries():
    t = SC.lattice(17)
    assert len(t) == 4913 and len(SC.cell_centres(17)) == 16 ** 3
    _, d = O.knn(SC.cell_centres(17), t, 9, kdtree=False)
    assert (d[:, :8] == np.float32(0.75)).all() and (d[:, 8] > np.float32(0.75)).all()
    _, d = O.knn(SC.face_centres(17), t, 5, kdtree=False)
    assert (d[:, :4] == np.float32(0.5)).all() and (d[:, 4] > np.float32(0.5)).all()
    # the tied targets of a row lie in different leaves of 16 curve-consecutive points however the curve runs: a leaf
    # holds at most 16 of the lattice's points, the eight corners of a cell are found among lists of 4913 shuffled indices
    i, _ = O.knn(SC.cell_centres(17), t, 8, kdtree=False)
    assert (np.diff(i, axis=1) > 0).all()     # tied entries come lowest caller index first


def test_denormal_distances():
    q, t = SC.queries("denormal", "self")
    _, d = O.knn(q, t, 4, kdtree=False)
    tiny = np.finfo(np.float32).tiny
    sub = (d > 0) & (d < tiny)
    assert sub.sum() >= 64 * 3                 # the 64 close points: three denormal distances each (the first is 0, the point itself)
    q, t = SC.queries("denormal", "probe")
    _, d = O.knn(q, t, 4, kdtree=False)
    assert ((d > 0) & (d < tiny)).all()        # between two of them: four denormal distances, none of them zero


def test_duplicates_fill_more_than_a_leaf_group():
    q, t = SC.queries("duplicates", "self")
    uniq, counts = np.unique(t, axis=0, return_counts=True)
    assert len(uniq) == 40 and (counts == 100).all() and counts.min() > 64
    i, d = O.knn(q, t, 32, kdtree=False)
    assert (d == 0).all() and (np.diff(i, axis=1) > 0).all()


def test_degenerate_extents():
    t, _ = SC.case("line")
    assert (t[:, 1:] == 0).all()
    t, _ = SC.case("plane")
    assert (t[:, 2] == 0).all() and len(t) == 4096
    t, _ = SC.case("needle")
    ext = t.max(axis=0) - t.min(axis=0)
    assert ext[0] / ext[1] > 0.9e7 and ext[0] / ext[2] > 0.9e7
    t, _ = SC.case("one_cell")
    ext = (t.max(axis=0) - t.min(axis=0)).max()
    inside = ((t >= [37, 61, 12]) & (t <= np.array([37, 61, 12]) + 1.04e-4)).all(axis=1)   # (float32 spacing at 61 is 3.8e-6)
    assert inside.sum() >= 5000 and 1e-4 / ext < 1.01e-6
    t, _ = SC.case("offset")
    assert np.abs(t).min(axis=0).min() > 30000 and np.spacing(np.abs(t)).max() >= 2.0 ** -7
    q, t = SC.queries("outside", "far")
    assert (np.abs(q - 0.5).max(axis=1) > 99).all() and len(np.unique(np.sign(np.round(q / 100)), axis=0)) == 26


def test_tree_heights_and_segment_sizes():
    assert sorted({SC.tree_height(n) for n in SC.TREE_TARGETS}) == list(range(8))
    assert [SC.tree_height(n) for n in SC.TALL_TREES] == [8, 9]
    assert SC.tree_height(SC.HEIGHT9_POINTS) == 9 and SC.tree_height(SC.HEIGHT9_POINTS - 16) == 8
    assert [SC.tree_height(n) for n in (16, 17, 64, 65, 4096, 4097)] == [0, 1, 1, 2, 4, 5]
    for n in SC.TREE_TARGETS:
        assert len(set(SC.tree_sources(n))) == 2
    assert {s for n in SC.TREE_TARGETS for s in SC.tree_sources(n)} == set(SC.TREE_SOURCES)
    src, sl, tgt, tl = SC.segments()
    assert sorted(np.bincount(tl)[1:13]) == sorted(SC.SEGMENT_SIZES) and sorted(np.bincount(sl)[1:13]) == sorted(SC.SEGMENT_SIZES)
    assert (sl == 13).sum() == 30 and (tl == 13).sum() == 0 and (tl == 14).sum() == 40 and (sl == 14).sum() == 0
    assert (np.diff(sl.astype(np.int64)) != 0).mean() > 0.5   # shuffled: segments are not contiguous in the caller's order
