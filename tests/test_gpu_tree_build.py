"""The tree build (csrc/build_tree.hip) at the shapes where "one segment" and "several segments" used to be separate code, on an
MI355X (-m gpu): a SICP_MODE_SEMANTIC cloud of ONE label (a segment table of one, with a caller-index array), a table that
holds a segment with a wide level (more than 1024 nodes: more than 65 536 points) next to segments of 1 and 17 points and one
whose level 1 has exactly 1024 nodes, and a table whose length changes between uploads through one handle.  No API reads a
tree back, so every check is the exact search over it: Engine.correspondences against the oracle's plain brute force
(oracle_lib.knn(..., kdtree=False)), indices and float32 distances with np.array_equal, as in tests/test_gpu_search_edges.py."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import search_cases as SC
from test_gpu_search_edges import IDENT, POSE, assert_lists_equal, gated, make_engine, sicp

pytestmark = pytest.mark.gpu

ONE_LABEL_SIZES = (1, 16, 17, 1025, 65537)     # 65 537: 4097 real leaves, top = 7, level 1 has 4096 nodes (a launch of its own)
MIXED_SIZES = {1: 65537, 2: 1, 3: 17, 4: 16385}  # 16 385: 1025 real leaves, top = 6, level 1 has exactly 1024 nodes (not wide)


def semantic_reference(src, sl, tgt, tl, qt, gate):
    """per-label brute force: a source point searches the target points of its own label; -1 / +inf where there are none"""
    q = O.transform_points(O.se3_matrix(qt), src)
    want_i = np.full((len(src), 1), -1, dtype=np.int32)
    want_d = np.full((len(src), 1), np.inf, dtype=np.float32)
    for l in np.unique(sl):
        si, ti = np.nonzero(sl == l)[0], np.nonzero(tl == l)[0]
        if len(ti) == 0:
            continue
        oi, od = O.knn(q[si], tgt[ti], 1, kdtree=False)
        want_i[si, 0] = np.where(od[:, 0] < gate, ti[oi[:, 0]], -1)
        want_d[si] = od
    return want_i, want_d


# ------------------------------------------------------------------------------------------------------------------------------
# a one-label SEMANTIC cloud is the flat cloud
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_t,nn_method", [(n, 1) for n in ONE_LABEL_SIZES] + [(65537, 2)])
def test_one_label_semantic_cloud_is_the_flat_cloud(n_t, nn_method):
    tgt = SC.uniform_cloud(n_t, 5000 + n_t)
    src = SC.sources_under(O.se3_matrix(POSE), 1000, 6000 + n_t)
    with make_engine(sicp.MODE_SEMANTIC, nn_method, min_class_pts=0) as es:
        gate = es.get_params().gate_sq
        es.set_source(src, np.full(len(src), 3, dtype=np.uint32))
        es.set_target(tgt, np.full(n_t, 3, dtype=np.uint32))
        with make_engine(sicp.MODE_GICP, nn_method, gate_sq=gate) as ef:
            ef.set_source(src)
            ef.set_target(tgt)
            for qt in (IDENT, POSE):
                si, sd, _ = es.correspondences(qt)
                fi, fd, _ = ef.correspondences(qt)
                assert_lists_equal(si, sd, fi, fd, (n_t, "semantic against flat", qt is POSE))
                want_i, want_d = O.knn(O.transform_points(O.se3_matrix(qt), src), tgt, 1, kdtree=False)
                assert_lists_equal(fi, fd, gated(want_i, want_d, gate), want_d, (n_t, "flat against oracle", qt is POSE))


# ------------------------------------------------------------------------------------------------------------------------------
# big and tiny segments in one table
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_clouds():
    """a target of the four labels of MIXED_SIZES in shuffled point order (the caller-index array is not the identity), and
    300 sources per label plus 50 of label 5, which the target lacks.  Returns src, src_labels, tgt, tgt_labels (read-only)."""
    M = O.se3_matrix(POSE)
    tgt = np.concatenate([SC.uniform_cloud(n, 7000 + l) for l, n in MIXED_SIZES.items()])
    tl = np.concatenate([np.full(n, l, dtype=np.uint32) for l, n in MIXED_SIZES.items()])
    src = np.concatenate([SC.sources_under(M, 300 if l < 5 else 50, 8000 + l) for l in (1, 2, 3, 4, 5)])
    sl = np.repeat(np.arange(1, 6, dtype=np.uint32), (300, 300, 300, 300, 50))
    rng = np.random.default_rng(48)
    ps, pt = rng.permutation(len(src)), rng.permutation(len(tgt))
    out = src[ps], sl[ps], tgt[pt], tl[pt]
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def mixed_reference(pose_name):
    src, sl, tgt, tl = mixed_clouds()
    gate = np.float32(sicp.default_params(sicp.MODE_SEMANTIC).gate_sq)
    i, d = semantic_reference(src, sl, tgt, tl, dict(ident=IDENT, pose=POSE)[pose_name], gate)
    i.setflags(write=False); d.setflags(write=False)
    return i, d


def test_big_and_tiny_segments_in_one_table():
    src, sl, tgt, tl = mixed_clouds()
    with make_engine(sicp.MODE_SEMANTIC, 1, min_class_pts=0) as e:
        assert np.float32(e.get_params().gate_sq) == np.float32(sicp.default_params(sicp.MODE_SEMANTIC).gate_sq)
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        for step, (name, qt) in enumerate((("ident", IDENT), ("pose", POSE), ("ident", IDENT))):   # (the later calls start from hints)
            idx, d2, _ = e.correspondences(qt)
            assert_lists_equal(idx, d2, *mixed_reference(name), ("mixed table call", step))
            assert (idx[sl == 5] == -1).all() and np.isposinf(d2[sl == 5]).all()


# ------------------------------------------------------------------------------------------------------------------------------
# a re-upload through the same cloud changes the table's length
# ------------------------------------------------------------------------------------------------------------------------------
def test_reupload_changes_the_table_length():
    src, sl, tgt, tl = mixed_clouds()
    small = SC.uniform_cloud(17, 9000)
    small_l = np.full(17, 3, dtype=np.uint32)
    with make_engine(sicp.MODE_SEMANTIC, 1, min_class_pts=0) as e:
        gate = np.float32(e.get_params().gate_sq)
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        first = [e.correspondences(qt)[:2] for qt in (IDENT, POSE)]
        e.set_target(small, small_l)
        for qt in (IDENT, POSE):
            idx, d2, _ = e.correspondences(qt)
            assert_lists_equal(idx, d2, *semantic_reference(src, sl, small, small_l, qt, gate), ("one-label re-upload", qt is POSE))
        e.set_target(tgt, tl)
        for (want_i, want_d), qt in zip(first, (IDENT, POSE)):
            idx, d2, _ = e.correspondences(qt)
            assert idx.tobytes() == want_i.tobytes() and d2.tobytes() == want_d.tobytes(), ("third upload", qt is POSE)
