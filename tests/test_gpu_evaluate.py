"""GPU tests of sicp_evaluate / sicp_evaluate_batch: the per-point outputs are, bit for bit, the K = 1 correspondences of a
GICP-mode handle whose gate is max_dist_sq -- on handles in every mode, the SEMANTIC one merging one search per label tree --
the aggregates are tests/evaluate_ref.py applied to them, the handle is left as it was, and every row of a batch has the bytes
of its lone call."""
import functools
import importlib
import math

import numpy as np
import pytest

import evaluate_ref as ref
import np_ref
import search_cases
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
CLOUDS = ("lidar2000", "lidar20000", "lattice", "three_labels")


@functools.lru_cache(maxsize=None)
def cloud(name):
    """src, src_labels, tgt, tgt_labels, qt, max_dist_sq"""
    if name.startswith("lidar"):
        n = int(name[5:])
        src, sl, tgt, tl, T_gt, _ = synth.lidar_pair(seed=11 if n == 2000 else 12, n_points=n)
        return src, sl, tgt, tl, np_ref.mat_to_qt(T_gt), 0.25  # (inliers and outliers both occur: asserted below)
    if name == "lattice":
        # every query has eight targets at d^2 = 0.75 exactly; with the labels below they lie in three label trees
        tgt, src = search_cases.lattice(17), search_cases.cell_centres(17)
        tl = (1 + np.arange(len(tgt)) % 3).astype(np.uint32)
        sl = (1 + np.arange(len(src)) % 3).astype(np.uint32)
        return src, sl, tgt, tl, IDENT, 1.0
    if name == "three_labels":
        # target segments of 1, 17 and 500 points: a one-point tree, a tree of two leaves, and the merge across them
        rng = np.random.default_rng(21)
        tgt = rng.uniform(0, 10, (518, 3)).astype(np.float32)
        tl = rng.permutation(np.repeat([1, 2, 3], [1, 17, 500])).astype(np.uint32)
        src = rng.uniform(-0.5, 10.5, (601, 3)).astype(np.float32)
        sl = rng.integers(1, 4, 601).astype(np.uint32)
        qt = np_ref.mat_to_qt(synth.pose_matrix(2.0, (1, 2, 3), (0.1, -0.05, 0.02)))
        return src, sl, tgt, tl, qt, 0.5
    raise KeyError(name)


def _engine(mode, src, sl, tgt, tl, num_classes=11, confusion=False, **kw):
    p = sicp.default_params(mode)
    p.num_classes = num_classes
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    if confusion:
        e.set_confusion(synth.confusion_matrix(num_classes))
    if src is not None:
        e.set_source(src, sl)
    if tgt is not None:
        e.set_target(tgt, tl)
    return e


@functools.lru_cache(maxsize=None)
def correspondences_k1(name):
    """the reference of the per-point outputs: sicp_correspondences of a GICP-mode handle with knn = 1, gate_sq = max_dist_sq"""
    src, sl, tgt, tl, qt, gate = cloud(name)
    with _engine(G, src, sl, tgt, tl, knn=1, gate_sq=gate) as e:
        idx, d2, _ = e.correspondences(qt)
    idx, d2 = idx[:, 0].copy(), d2[:, 0].copy()
    idx.setflags(write=False)
    d2.setflags(write=False)
    return idx, d2


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- per-point bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
@pytest.mark.parametrize("name", CLOUDS)
def test_per_point_outputs_are_the_k1_correspondences(name, mode):
    """the EM handle has no confusion matrix; the SEMANTIC handle's target holds one tree per label, so its result is the merge
    of their winners; params.knn (4 in EM mode) and gate_sq (250) are the modes' defaults and play no part"""
    src, sl, tgt, tl, qt, gate = cloud(name)
    want_idx, want_d2 = correspondences_k1(name)
    with _engine(mode, src, sl, tgt, tl) as e:
        r = e.evaluate(qt, gate, per_point=True)
    assert _same_bits(r["nn_idx"], want_idx)
    assert _same_bits(r["nn_d2"], want_d2)
    assert r["n_source"] == len(src) and r["inliers"] == int((want_idx >= 0).sum())
    if name.startswith("lidar"):
        assert 0 < r["inliers"] < r["n_source"]
    if name == "lattice":
        assert (r["nn_d2"] == 0.75).all() and r["inliers"] == len(src)


@pytest.mark.parametrize("name", ["lattice", "three_labels"])
def test_per_point_outputs_match_the_numpy_restatement(name):
    """ties across label trees go to the lower caller index: of the eight lattice targets at d^2 = 0.75 the restatement's"""
    src, sl, tgt, tl, qt, gate = cloud(name)
    want = ref.evaluate(src, tgt, qt, gate)
    with _engine(S, src, sl, tgt, tl) as e:
        r = e.evaluate(qt, gate, per_point=True)
    assert _same_bits(r["nn_idx"], want["nn_idx"]) and _same_bits(r["nn_d2"], want["nn_d2"])


# ---- aggregates -------------------------------------------------------------------------------------------------------------
def _check_aggregates(r, sl, tl, classes):
    want = ref.reduce(r["nn_idx"], r["nn_d2"], sl, tl, classes)
    for f in ("n_source", "inliers", "label_agree", "label_outside"):
        assert r[f] == want[f], f
    if classes is not None:
        assert r["confusion"].dtype == np.int64 and np.array_equal(r["confusion"], want["confusion"])
        assert r["label_outside"] + int(r["confusion"].sum()) == r["inliers"]
    # the worst case of a double sum of n non-negative terms in any order
    assert abs(r["sum_d2"] - want["sum_d2"]) <= r["n_source"] * 2.0 ** -53 * want["sum_d2"]
    assert r["fitness"] == (r["inliers"] / r["n_source"] if r["n_source"] else 0.0)
    if r["inliers"]:
        assert r["inlier_rmse"] == math.sqrt(r["sum_d2"] / r["inliers"])
    else:
        assert math.isnan(r["inlier_rmse"])


# C = 3 is below the largest lidar label (11): label_outside counts; 40: the table privatised in LDS; 64 / 65: the largest
# table kept in LDS and the smallest counted in HBM directly
@pytest.mark.parametrize("classes", [3, 40, 64, 65])
@pytest.mark.parametrize("name,mode", [("lidar2000", G), ("lidar20000", E), ("lattice", S), ("three_labels", S)],
                         ids=["lidar2000-gicp", "lidar20000-em", "lattice-semantic", "three_labels-semantic"])
def test_aggregates_are_the_restatement_of_the_per_point_outputs(name, mode, classes):
    src, sl, tgt, tl, qt, gate = cloud(name)
    with _engine(mode, src, sl, tgt, tl) as e:
        r = e.evaluate(qt, gate, num_classes=classes, per_point=True)
        plain = e.evaluate(qt, gate)  # without a table, without per-point outputs
    _check_aggregates(r, sl, tl, classes)
    if name.startswith("lidar") and classes == 3:
        assert r["label_outside"] > 0
    assert plain["label_outside"] == 0 and "confusion" not in plain and "nn_idx" not in plain
    for f in ("n_source", "inliers", "label_agree", "sum_d2", "fitness", "inlier_rmse"):
        assert plain[f] == r[f], f


def test_clouds_without_labels():
    src, _, tgt, _, qt, gate = cloud("lidar2000")
    with _engine(G, src, None, tgt, None) as e:
        r = e.evaluate(qt, gate, per_point=True)
        assert r["label_agree"] == 0 and r["inliers"] == int((correspondences_k1("lidar2000")[0] >= 0).sum())
        with pytest.raises(sicp.SicpError) as err:
            e.evaluate(qt, gate, num_classes=3)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT


# ---- neutrality -------------------------------------------------------------------------------------------------------------
def _stats_bytes(e):
    st = sicp.SicpStats()
    assert sicp.lib().sicp_get_stats(e._h, C.byref(st)) == sicp.OK
    return bytes(st)


@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
def test_evaluate_leaves_the_handle_as_it_was(mode):
    src, sl, tgt, tl, qt, gate = cloud("lidar2000")
    other = np_ref.mat_to_qt(np_ref.qt_to_mat(qt) @ synth.pose_matrix(1.0, (0, 1, 0), (0.3, 0.1, -0.2)))
    with _engine(mode, src, sl, tgt, tl, confusion=(mode == E), min_class_pts=40) as e:
        e.align(qt)  # (statistics that are not all zero)
        c0 = e.correspondences(qt)
        a0 = e.accumulate(qt)
        s0 = _stats_bytes(e)
        r = e.evaluate(other, gate, num_classes=11, per_point=True)
        assert r["inliers"] > 0
        assert _stats_bytes(e) == s0
        a1 = e.accumulate(qt)  # on the correspondences the handle held before the evaluation
        c1 = e.correspondences(qt)
    assert a0.tobytes() == a1.tobytes()
    for x, y in zip(c0, c1):
        assert _same_bits(x, y)


# ---- edges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [G, S], ids=["gicp", "semantic"])
def test_non_finite_points_are_left_out(mode):
    src, sl, tgt, tl, qt, gate = cloud("lidar2000")
    src, tgt = src.copy(), tgt.copy()
    src[[0, 77, 1999]] = np.nan
    src[500, 1] = np.inf
    tgt[[5, 1000]] = np.nan
    want = ref.evaluate(src, tgt, qt, gate, sl, tl, 11)
    with _engine(mode, src, sl, tgt, tl) as e:
        r = e.evaluate(qt, gate, num_classes=11, per_point=True)
    dropped = [0, 77, 500, 1999]
    assert r["n_source"] == 1996 and (r["nn_idx"][dropped] == -1).all() and np.isnan(r["nn_d2"][dropped]).all()
    assert _same_bits(r["nn_idx"], want["nn_idx"]) and np.array_equal(r["nn_d2"], want["nn_d2"], equal_nan=True)
    assert not np.isin([5, 1000], r["nn_idx"]).any()
    _check_aggregates(r, sl, tl, 11)
    assert np.array_equal(r["confusion"], want["confusion"])


def test_gates_at_both_ends():
    src, sl, tgt, tl, qt, _ = cloud("three_labels")
    found = correspondences_k1("three_labels")[1]
    with _engine(S, src, sl, tgt, tl) as e:
        none = e.evaluate(qt, 1e-12, num_classes=3, per_point=True)
        every = e.evaluate(qt, float("inf"), num_classes=3, per_point=True)
    assert none["inliers"] == 0 and none["sum_d2"] == 0.0 and none["fitness"] == 0.0 and math.isnan(none["inlier_rmse"])
    assert (none["nn_idx"] == -1).all() and _same_bits(none["nn_d2"], found) and none["confusion"].sum() == 0
    assert every["inliers"] == every["n_source"] == len(src) and every["fitness"] == 1.0
    assert (every["nn_idx"] >= 0).all() and _same_bits(every["nn_d2"], found) and every["confusion"].sum() == len(src)
    _check_aggregates(every, sl, tl, 3)


def test_missing_and_empty_clouds():
    src, sl, tgt, tl, qt, gate = cloud("three_labels")
    with _engine(G, src, sl, None, None) as e:
        with pytest.raises(sicp.SicpError) as err:
            e.evaluate(qt, gate)
        assert err.value.status == sicp.ERR_NOT_READY
    with _engine(G, None, None, tgt, tl) as e:
        with pytest.raises(sicp.SicpError) as err:
            e.evaluate(qt, gate)
        assert err.value.status == sicp.ERR_NOT_READY
    with _engine(G, src, sl, np.full_like(tgt, np.nan), tl) as e:
        with pytest.raises(sicp.SicpError) as err:
            e.evaluate(qt, gate)
        assert err.value.status == sicp.ERR_TOO_FEW_POINTS
    with _engine(E, np.full_like(src, np.nan), sl, tgt, tl) as e:  # no finite source point: nothing to ask, nothing wrong
        r = e.evaluate(qt, gate, num_classes=3, per_point=True)
    assert r["n_source"] == r["inliers"] == 0 and r["fitness"] == 0.0 and math.isnan(r["inlier_rmse"]) and r["sum_d2"] == 0.0
    assert (r["nn_idx"] == -1).all() and np.isnan(r["nn_d2"]).all() and r["confusion"].sum() == 0


# ---- repeatability and batch ------------------------------------------------------------------------------------------------
def _lone(e, qt, gate, classes):
    r = sicp.SicpEvaluateResult()
    conf = np.full((classes, classes), 77, dtype=np.int64)
    q = np.ascontiguousarray(qt, dtype=np.float64)
    rc = sicp.lib().sicp_evaluate(e._h, sicp._ptr(q, sicp._dp), gate, classes, sicp._ptr(conf, C.POINTER(C.c_int64)), None, None, C.byref(r))
    return rc, bytes(r), conf


def _batch(es, qts, gate, classes):
    n = len(es)
    out = (sicp.SicpEvaluateResult * n)()
    C.memset(out, 0x5A, C.sizeof(out))
    status = np.full(n, 99, dtype=np.int32)
    conf = np.full((n, classes, classes), 77, dtype=np.int64)
    q = np.ascontiguousarray(np.stack(qts), dtype=np.float64)
    rc = sicp.lib().sicp_evaluate_batch(sicp._handles(es), n, sicp._ptr(q, sicp._dp), gate, classes, sicp._ptr(conf, C.POINTER(C.c_int64)),
                                        out, sicp._ptr(status, sicp._ip))
    return rc, status, [bytes(out[k]) for k in range(n)], conf


def test_two_calls_give_identical_bytes():
    src, sl, tgt, tl, qt, gate = cloud("lidar20000")
    with _engine(S, src, sl, tgt, tl) as e:
        a, b = _lone(e, qt, gate, 11), _lone(e, qt, gate, 11)
    assert a[0] == b[0] == sicp.OK and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[2].sum() > 0


def test_batch_rows_are_their_lone_calls():
    """five rows in mixed modes: handle 0 twice (at two poses: two groups), handles 0 (GICP) and 1 (SEMANTIC) share a target --
    which each of them lays out its own way, so they cannot share a group either -- and handle 3 has no target"""
    src, sl, tgt, tl, qt, gate = cloud("lidar2000")
    s3, sl3, t3, tl3, qt3, _ = cloud("three_labels")
    other = np_ref.mat_to_qt(np_ref.qt_to_mat(qt) @ synth.pose_matrix(0.5, (0, 0, 1), (0.2, 0.0, 0.0)))
    es = []
    try:
        e0 = _engine(G, src, sl, tgt, tl)
        es.append(e0)
        e1 = _engine(S, src[::2].copy(), sl[::2].copy(), None, None)
        es.append(e1)
        e1.share_cloud(sicp.TARGET, e0, sicp.TARGET)
        es.append(_engine(E, s3, sl3, t3, tl3))
        es.append(_engine(G, src, sl, None, None))
        rows = [es[0], es[1], es[2], es[3], es[0]]
        qts = [qt, qt, qt3, qt, other]
        good = [0, 1, 2, 4]
        lone = {k: _lone(rows[k], qts[k], gate, 11) for k in good}
        assert all(lone[k][0] == sicp.OK for k in good) and lone[0][1] != lone[4][1]
        assert _lone(rows[3], qts[3], gate, 11)[0] == sicp.ERR_NOT_READY
        first = _batch(rows, qts, gate, 11)
        again = _batch(rows, qts, gate, 11)
        for rc, status, out, conf in (first, again):
            assert rc == sicp.ERR_NOT_READY
            assert list(status) == [sicp.OK, sicp.OK, sicp.OK, sicp.ERR_NOT_READY, sicp.OK]
            for k in good:
                assert out[k] == lone[k][1], k
                assert np.array_equal(conf[k], lone[k][2]), k
            assert out[3] == b"\x5a" * C.sizeof(sicp.SicpEvaluateResult) and (conf[3] == 77).all()
        # the Python form of the same call
        res = sicp.evaluate_batch(rows, np.stack(qts), gate, num_classes=11)
        assert [s for s, _ in res] == [sicp.OK, sicp.OK, sicp.OK, sicp.ERR_NOT_READY, sicp.OK] and res[3][1] is None
        assert np.array_equal(res[1][1]["confusion"], lone[1][2]) and res[1][1]["inliers"] > 0
        # the lone calls still give what they gave (the shared target has gone through both layouts meanwhile)
        for k in good:
            rc, b, conf = _lone(rows[k], qts[k], gate, 11)
            assert rc == sicp.OK and b == lone[k][1] and np.array_equal(conf, lone[k][2]), k
    finally:
        for e in es:
            e.close()


def test_a_batch_row_without_source_points_owns_no_workgroup():
    """three pairs in one group, one whose source has no finite point -- a job without workgroups -- at position 0, 1 and 2:
    every row and table is its lone call's, the empty pair's says so"""
    src, sl, tgt, tl, qt, gate = cloud("lidar2000")
    s3, sl3, t3, tl3, qt3, _ = cloud("three_labels")
    full = [(src, sl, tgt, tl, qt), (s3, sl3, t3, tl3, qt3)]
    empty = (np.full_like(s3, np.nan), sl3, tgt, tl, qt)
    for at in range(3):
        pairs = list(full)
        pairs.insert(at, empty)
        es = [_engine(G, a, al, b, bl) for a, al, b, bl, _ in pairs]
        try:
            qts = [q for *_, q in pairs]
            lone = [_lone(e, q, gate, 11) for e, q in zip(es, qts)]
            assert all(rc == sicp.OK for rc, _, _ in lone)
            rc, status, out, conf = _batch(es, qts, gate, 11)
            assert rc == sicp.OK and list(status) == [sicp.OK] * 3
            for k in range(3):
                assert out[k] == lone[k][1], (at, k)
                assert np.array_equal(conf[k], lone[k][2]), (at, k)
            r = sicp.SicpEvaluateResult.from_buffer_copy(out[at])
            assert r.n_source == r.inliers == 0 and conf[at].sum() == 0
            others = [sicp.SicpEvaluateResult.from_buffer_copy(out[k]) for k in range(3) if k != at]
            assert all(o.inliers > 0 for o in others)
        finally:
            for e in es:
                e.close()
