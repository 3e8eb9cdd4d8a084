"""The exact k-NN search (csrc/knn_kernels.hip over the tree of csrc/build_tree.hip) at the edges of its tree shapes and at tied
distances, on an MI355X (-m gpu).  Every test goes through the public hooks Engine.correspondences and Engine.covariances,
runs all three engines (nn_method 0, 1, 2) unless it says otherwise, and compares EVERY row with the oracle's plain brute force
(oracle_lib.knn(..., kdtree=False): order (distance, lower caller index)) -- indices and float32 distances with
np.array_equal, so there is no tolerance anywhere.  The inputs are those of tests/search_cases.py; what they contain is
asserted without a GPU in tests/test_search_edges_cpu.py."""
import functools
import importlib
import time

import numpy as np
import pytest

import oracle_lib as O
import search_cases as SC
import synth
from np_ref import mat_to_qt

pytestmark = pytest.mark.gpu

sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
POSE = mat_to_qt(synth.pose_matrix(37.0, (1, 2, 3), (0.3, -0.2, 0.1)))   # a generic pose: the transform path runs
NO_GATE = 1e30
MODE_K = ((sicp.MODE_GICP, 1), (sicp.MODE_EM, 4))


@pytest.fixture(params=[0, 1, 2], ids=["bruteforce", "boxtree", "boxtree_per_query"])
def nn(request):
    return request.param


def make_engine(mode, nn_method, C=3, **kw):
    """EM-mode handles carry labels of all ones under a C-class confusion matrix (the search does not read them)"""
    p = sicp.default_params(mode)
    p.num_classes = C if mode == sicp.MODE_EM else 0
    p.nn_method = nn_method
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    if mode == sicp.MODE_EM:
        e.set_confusion(synth.confusion_matrix(C) if C > 1 else np.ones((1, 1)))
    return e


def ones(n):
    return np.ones(n, dtype=np.uint32)


def gated(idx, d2, gate_sq):
    """the reference's indices behind the gate: strict <, float32 compare (tests/test_gpu_parity.py)"""
    return np.where(d2 < np.float32(gate_sq), idx, -1).astype(np.int32)


def first_difference(got, want):
    bad = np.nonzero((got != want).any(axis=1))[0]
    return None if len(bad) == 0 else (int(bad[0]), len(bad), got[bad[0]].tolist(), want[bad[0]].tolist())


def assert_lists_equal(idx, d2, want_i, want_d, what):
    assert np.array_equal(idx, want_i), (what, "row, rows differing, got, want", first_difference(idx, want_i))
    if d2 is not None:
        assert np.array_equal(d2, want_d), (what, "row, rows differing, got, want", first_difference(d2, want_d))


@functools.lru_cache(maxsize=None)
def reference(kind, name, qset, k):
    """oracle brute force of a query set of search_cases (cached: shared by the three engines, never written to)"""
    q, t = SC.queries(name, qset)
    i, d = O.knn(q, t, k, kdtree=False)
    i.setflags(write=False); d.setflags(write=False)
    return i, d


def search(mode, nn_method, src, tgt, qt, gate_sq=NO_GATE):
    with make_engine(mode, nn_method, gate_sq=gate_sq) as e:
        em = mode == sicp.MODE_EM
        e.set_source(src, ones(len(src)) if em else None)
        e.set_target(tgt, ones(len(tgt)) if em else None)
        idx, d2, _ = e.correspondences(qt)
    return idx, d2


# ------------------------------------------------------------------------------------------------------------------------------
# tree shapes: every height 0..7, sizes one below / at / one above a full leaf, leaf group and level
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t", SC.TREE_TARGETS)
def test_tree_shapes_correspondences(n_t, nn):
    tgt = SC.uniform_cloud(n_t, 1000 + n_t)
    M = O.se3_matrix(POSE)
    for n_s in SC.tree_sources(n_t):
        src = SC.sources_under(M, n_s, 2000 + n_t + n_s)
        q = O.transform_points(M, src)
        for mode, K in MODE_K:
            if n_t < K:
                continue      # EM refuses a target smaller than K (tests/test_gpu_parity.py)
            idx, d2 = search(mode, nn, src, tgt, POSE)
            want_i, want_d = O.knn(q, tgt, K, kdtree=False)
            assert_lists_equal(idx, d2, gated(want_i, want_d, NO_GATE), want_d, (n_t, n_s, K, "height", SC.tree_height(n_t)))


@functools.lru_cache(maxsize=None)
def self_reference(n, k):
    p = SC.uniform_cloud(n, 3000 + n)
    i, _ = O.knn(p, p, k, kdtree=False)
    i.setflags(write=False)
    return i


@pytest.mark.parametrize("n", SC.SELF_SIZES)
def test_tree_shapes_self_search(n, nn):
    """k_cov neighbours of every point of a cloud in itself: lists shorter than k_cov end in -1 (17..19 points at k_cov = 20:
    the K >= 16 seed sorts a leaf group that is partly sentinel points), and the label histograms are the lists' counts"""
    p = SC.uniform_cloud(n, 3000 + n)
    for C in (1, 16, 17):
        lab = np.random.default_rng(n + C).integers(1, C + 1, n).astype(np.uint32)
        with make_engine(sicp.MODE_EM, nn, C=C) as e:
            e.set_source(p, lab)
            for k in SC.K_COVS:
                prm = e.get_params()
                prm.k_cov = k
                e.set_params(prm)
                _, _, hist, nbr = e.covariances(sicp.SOURCE, want_hist=True, want_nn=True)
                want = self_reference(n, k)
                assert_lists_equal(nbr, None, want, None, (n, k, C))
                assert (nbr[:, min(n, k):] == -1).all() and (nbr[:, :min(n, k)] >= 0).all()
                counts = np.zeros((n, C), dtype=np.int64)
                for c in range(k):
                    ok = want[:, c] >= 0
                    np.add.at(counts, (np.nonzero(ok)[0], lab[want[ok, c]].astype(np.int64) - 1), 1)
                assert hist.dtype == np.uint8 and np.array_equal(hist, counts), (n, k, C)


# ------------------------------------------------------------------------------------------------------------------------------
# heights 8 and 9 (9: the third round trip of the path phase, more than 16 * 4^8 points in one segment)
# ------------------------------------------------------------------------------------------------------------------------------
TALL_QUERIES = 1024


@functools.lru_cache(maxsize=None)
def tall_case(n_t):
    tgt = SC.uniform_cloud(n_t, 77, side=100.0)
    M = O.se3_matrix(POSE)
    src = SC.sources_under(M, TALL_QUERIES, 78, side=100.0)
    q = O.transform_points(M, src)
    rows = np.sort(np.random.default_rng(79).choice(n_t, TALL_QUERIES, replace=False))
    i4, d4 = O.knn(q, tgt, 4, kdtree=False)
    ref = {4: (i4, d4), 1: (i4[:, :1], d4[:, :1])}   # (the first of a (distance, lower index) list IS the list of one)
    ref["self"] = O.knn(tgt[rows], tgt, 20, kdtree=False)[0]
    return tgt, src, rows, ref


@pytest.mark.parametrize("nn_method", [1, 2], ids=["boxtree", "boxtree_per_query"])
@pytest.mark.parametrize("n_t", SC.TALL_TREES)
def test_tall_trees(n_t, nn_method):
    """(the brute-force engine is left out: its k = 20 self-search of a million points is 10^12 distances)"""
    tgt, src, rows, ref = tall_case(n_t)
    assert SC.tree_height(n_t) == (9 if n_t == SC.HEIGHT9_POINTS else 8)
    t0 = time.perf_counter()
    with make_engine(sicp.MODE_EM, nn_method, gate_sq=NO_GATE) as e:
        e.set_source(src, ones(len(src)))
        e.set_target(tgt, ones(len(tgt)))
        idx, d2, _ = e.correspondences(POSE)
        assert_lists_equal(idx, d2, gated(*ref[4], NO_GATE), ref[4][1], (n_t, 4))
        prm = e.get_params()
        prm.mode, prm.knn = sicp.MODE_GICP, 1        # K = 1 on the same tree
        e.set_params(prm)
        idx, d2, _ = e.correspondences(POSE)
        assert_lists_equal(idx, d2, gated(*ref[1], NO_GATE), ref[1][1], (n_t, 1))
        _, _, _, nbr = e.covariances(sicp.TARGET, want_nn=True)
        assert_lists_equal(nbr[rows], None, ref["self"], None, (n_t, "self"))
    print(f"tall tree n_t={n_t} nn_method={nn_method}: {time.perf_counter() - t0:.2f} s on the device side")


# ------------------------------------------------------------------------------------------------------------------------------
# geometries: ties across the cut, degenerate boxes, one curve cell, coarse float32 spacing, denormal distances
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,qset", SC.QUERY_SETS)
def test_geometries_correspondences(name, qset, nn):
    q, t = SC.queries(name, qset)
    for mode, K in MODE_K:
        idx, d2 = search(mode, nn, q, t, IDENT)      # (the identity in float64 leaves every float32 coordinate as it is)
        want_i, want_d = reference("corr", name, qset, K)
        assert_lists_equal(idx, d2, gated(want_i, want_d, NO_GATE), want_d, (name, qset, K))


@pytest.mark.parametrize("name", SC.SELF_CASES)
def test_geometries_self_search(name, nn):
    t, _ = SC.case(name)
    with make_engine(sicp.MODE_GICP, nn) as e:
        e.set_source(t)
        for k in (20, 32):
            prm = e.get_params()
            prm.k_cov = k
            e.set_params(prm)
            _, _, _, nbr = e.covariances(sicp.SOURCE, want_nn=True)
            assert_lists_equal(nbr, None, reference("self", name, "self", k)[0], None, (name, k))


# ------------------------------------------------------------------------------------------------------------------------------
# the gate: strict float32 <, at a distance that equals it exactly
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,K", MODE_K, ids=["gicp1", "em4"])
def test_gate_at_exactly_the_distance(mode, K, nn):
    q, t = SC.queries("lattice", "cells")
    want_i, want_d = reference("corr", "lattice", "cells", K)
    assert (want_d == np.float32(0.75)).all()
    idx, d2 = search(mode, nn, q, t, IDENT, gate_sq=0.75)
    assert (idx == -1).all()                       # 0.75 < 0.75 is false: every slot is gated out ...
    assert np.array_equal(d2, want_d)              # ... and still reports its distance
    just_above = float(np.nextafter(np.float32(0.75), np.float32(1)))
    idx, d2 = search(mode, nn, q, t, IDENT, gate_sq=just_above)
    assert_lists_equal(idx, d2, want_i, want_d, ("gate one ulp above", K))   # the lowest of the eight tied indices first
    assert (idx >= 0).all()


# ------------------------------------------------------------------------------------------------------------------------------
# seed hints: valid but stale by exactly one lattice cell, and all gated out (-1)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qset", ["self", "cells"])
def test_stale_and_gated_hints_on_the_lattice(qset, nn):
    q, t = SC.queries("lattice", qset)
    shift = np.array([0, 0, 0, 1, 1.0, 0, 0])          # one cell along x: every hint names a target one cell away
    away = np.array([0, 0, 0, 1, 1000.0, 0, 0])        # every slot beyond the default gate (250): every hint is -1
    with make_engine(sicp.MODE_EM, nn) as e:
        gate = np.float32(e.get_params().gate_sq)
        e.set_source(q, ones(len(q)))
        e.set_target(t, ones(len(t)))
        for step, qt in enumerate((IDENT, shift, away, IDENT)):
            idx, d2, _ = e.correspondences(qt)
            want_i, want_d = O.knn(O.transform_points(O.se3_matrix(qt), q), t, 4, kdtree=False)
            assert_lists_equal(idx, d2, gated(want_i, want_d, gate), want_d, (qset, "call", step))
            assert (idx == -1).all() == (step == 2)


# ------------------------------------------------------------------------------------------------------------------------------
# semantic mode: one tree per label segment, segments of 1..1025 points
# ------------------------------------------------------------------------------------------------------------------------------
def test_semantic_segments_of_every_size(nn):
    src, sl, tgt, tl = SC.segments()
    with make_engine(sicp.MODE_SEMANTIC, nn, min_class_pts=0) as e:
        gate = np.float32(e.get_params().gate_sq)
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        for step, qt in enumerate((IDENT, POSE, IDENT)):       # (the later calls start from the hints of the one before)
            idx, d2, _ = e.correspondences(qt)
            q = O.transform_points(O.se3_matrix(qt), src)
            want_i = np.full((len(src), 1), -1, dtype=np.int32)
            want_d = np.full((len(src), 1), np.inf, dtype=np.float32)
            for l in np.unique(sl):
                si, ti = np.nonzero(sl == l)[0], np.nonzero(tl == l)[0]
                if len(ti) == 0:
                    continue                                   # label 13: no target segment, -1 / +inf
                oi, od = O.knn(q[si], tgt[ti], 1, kdtree=False)
                want_i[si, 0] = np.where(od[:, 0] < gate, ti[oi[:, 0]], -1)
                want_d[si] = od
            assert_lists_equal(idx, d2, want_i, want_d, ("semantic call", step))
            assert (idx[sl == 13] == -1).all()
