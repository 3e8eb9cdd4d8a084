"""GPU tests of the label-aware initial alignment (sicp_bootstrap_semantic and its batch and hooks) against the numpy
restatement tests/bootstrap_semantic_ref.py, on the inputs of tests/bootstrap_semantic_cases.py: keypoints and their voted
labels, the label-restricted feature neighbours, the label-aware scores, the symmetric scene only the labels resolve, the
three bit-for-bit invariants that tie it to sicp_bootstrap, the batch and the refusals.  Tolerances: those of
tests/test_gpu_bootstrap.py for the same quantities."""
import ctypes as C
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import bootstrap_cases as BC
import bootstrap_ref as R
import bootstrap_semantic_cases as SC
import bootstrap_semantic_ref as S

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])


def _mat(qt):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    return T


def _engine(src, sl, tgt, tl, mode=sicp.MODE_GICP):
    e = sicp.Engine(0, sicp.default_params(mode))
    e.set_source(src, sl)
    e.set_target(tgt, tl)
    return e


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


COUNTS = ("n_source_keypoints", "n_target_keypoints", "max_neighbours", "best_iteration", "best_error")


def _same_result(a, b):
    return np.array_equal(a[0], b[0]) and all(a[1][k] == b[1][k] for k in COUNTS)


# ---- 1. keypoints and labels ----------------------------------------------------------------------------------------
def test_keypoints_and_labels_of_a_lidar_cloud_match_the_restatement():
    src, sl, tgt, tl, _ = BC.lidar_sub(2000)
    with _engine(src, sl, tgt, tl) as e:
        for which, cloud, lab in ((sicp.SOURCE, src, sl), (sicp.TARGET, tgt, tl)):
            xyz, kl = e.bootstrap_semantic_keypoints(which)
            kp, rl = S.voxel_keypoints(cloud, lab)
            assert _same_bits(xyz, kp) and kl.dtype == np.uint32 and np.array_equal(kl, rl)
            assert len(np.unique(rl)) > 3


@pytest.mark.parametrize("ignore", [(), (SC.IGNORED,), (SC.IGNORED, 123456, 6)])
def test_keypoints_and_labels_of_the_vote_cloud_match_the_restatement(ignore):
    cloud, lab, vox = SC.vote_cloud()
    lp = sicp.default_bootstrap_label_params(ignore=ignore)
    with _engine(cloud, lab, cloud, lab) as e:
        xyz, kl = e.bootstrap_semantic_keypoints(sicp.TARGET, None, lp)
    kp, rl = S.voxel_keypoints(cloud, lab, ignore=ignore)
    assert _same_bits(xyz, kp) and np.array_equal(kl, rl)
    at = {k: SC.keypoint_at(xyz, v) for k, v in vox.items()}
    assert kl[at["tie"]] == 3 and kl[at["pair"]] == 2 and kl[at["edge"]] == 4
    assert kl[at["extremes"]] == 0 and kl[at["top"]] == SC.BIG
    if SC.IGNORED in ignore:
        assert at["emptied"] is None and kl[at["swayed"]] == 5
    else:
        assert at["emptied"] is not None and kl[at["swayed"]] == SC.IGNORED
    assert kl[at["crowd"]] == 5


# ---- 2. / 3. feature neighbours, scores and matrices ----------------------------------------------------------------
def test_label_feature_neighbours_and_scores_match_the_restatement():
    c = SC.relabelled_pair()
    p = sicp.default_bootstrap_params()
    a, b = SC.near_identity_samples(c["skp"], c["tkp"])
    with _engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e:
        skp, skl = e.bootstrap_semantic_keypoints(sicp.SOURCE)
        tkp, tkl = e.bootstrap_semantic_keypoints(sicp.TARGET)
        _, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE)
        _, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET)
        M, err, knn = e.bootstrap_semantic_score(a, b, p, None, n_source_keypoints=len(skp))
        # each flag alone
        lp_m = sicp.default_bootstrap_label_params(score_same_label=0)
        lp_s = sicp.default_bootstrap_label_params(match_same_label=0)
        M_m, err_m, knn_m = e.bootstrap_semantic_score(a, b, p, lp_m, n_source_keypoints=len(skp))
        M_s, err_s, knn_s = e.bootstrap_semantic_score(a, b, p, lp_s, n_source_keypoints=len(skp))
        M_0, err_0, knn_0 = e.bootstrap_score(a, b, p, n_source_keypoints=len(skp))
    assert _same_bits(skp, c["skp"]) and _same_bits(tkp, c["tkp"])
    assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
    # neighbour lists equal (on the GPU's own features, as tests/test_gpu_bootstrap.py compares them)
    k = p.k_correspondences
    ref_knn = S.feature_knn(sf, tf, k, skl, tkl)
    assert np.array_equal(knn, ref_knn) and np.array_equal(knn_m, ref_knn)
    assert np.array_equal(knn_s, knn_0) and np.array_equal(knn_0, R.feature_knn(sf, tf, k))
    has_f = ~np.isnan(sf[:, 0])
    assert (knn[skl == SC.ABSENT] == -1).all() and (has_f & (skl == SC.ABSENT)).any()
    rare = has_f & (skl == SC.RARE)
    assert rare.any() and ((knn[rare] >= 0).sum(axis=1) == 3).all()
    assert len(np.unique(knn[has_f & (skl == SC.STRADDLE)] // 64)) >= 3
    # scores and matrices within 1e-9
    tree = R.cKDTree(tkp.astype(np.float64))
    wrong = 0
    for i in range(len(a)):
        Mr = R.umeyama(skp[a[i]], tkp[b[i]])
        assert np.abs(M[i] - Mr).max() < 1e-9
        er, w = S.truncated_error(M[i], skp, skl, tree, tkp, tkl, p.max_corr_distance, True)
        e0, _ = S.truncated_error(M[i], skp, skl, tree, tkp, tkl, p.max_corr_distance, False)
        wrong += w
        assert abs(err[i] - er) <= 1e-9 * max(1.0, abs(er)), (i, err[i], er)
        assert abs(err_s[i] - er) <= 1e-9 * max(1.0, abs(er))
        assert abs(err_m[i] - e0) <= 1e-9 * max(1.0, abs(e0)) and err_m[i] == err_0[i]
        assert w == 0 or err[i] > err_0[i]
    assert wrong >= 1
    assert np.array_equal(M, M_m) and np.array_equal(M, M_s) and np.array_equal(M, M_0)


# ---- 4. the symmetric scene -----------------------------------------------------------------------------------------
def test_the_labels_resolve_the_symmetric_scene():
    s, sl, t, tl, T = SC.symmetric_scene()
    ref_skp, ref_skl = S.voxel_keypoints(s, sl)
    ref_tkp, ref_tkl = S.voxel_keypoints(t, tl)
    p = sicp.default_bootstrap_params(seed=SC.SEED)
    with _engine(s, sl, t, tl) as e:
        skp, skl = e.bootstrap_semantic_keypoints(sicp.SOURCE)
        tkp, tkl = e.bootstrap_semantic_keypoints(sicp.TARGET)
        _, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE)
        _, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET)
        q1, info1 = e.bootstrap_semantic(p)
        q2, info2 = e.bootstrap_semantic(p)
        qb, infob = e.bootstrap(p)
    assert _same_bits(skp, ref_skp) and _same_bits(tkp, ref_tkp)
    assert np.array_equal(skl, ref_skl) and np.array_equal(tkl, ref_tkl)
    assert np.array_equal(q1, q2) and all(info1[k] == info2[k] for k in COUNTS)
    assert info1["n_source_keypoints"] == 1705 and info1["n_target_keypoints"] == 1930
    # the restatement on the GPU's own features (bin decisions on an edge may differ between the two FPFH computations)
    best, err, errs, Ms = S.sac_ia(skp, sf, skl, tkp, tf, tkl, seed=SC.SEED)
    gb = info1["best_iteration"]
    assert gb == best or abs(errs[gb] - err) <= 1e-9 * max(1.0, err)
    assert abs(info1["best_error"] - errs[gb]) <= 1e-9 * max(1.0, errs[gb])
    assert np.abs(_mat(q1)[:3] - Ms[gb]).max() < 1e-9
    rot, tr = SC.mat_delta(T, _mat(q1))
    assert rot < 5.0 and tr < 1.0, (rot, tr)
    rot_b, tr_b = SC.mat_delta(T, _mat(qb))
    assert rot_b > 170.0, (rot_b, tr_b)


# ---- 5. the invariants ----------------------------------------------------------------------------------------------
def test_without_flags_and_on_one_label_it_is_sicp_bootstrap_bit_for_bit():
    src, sl, tgt, tl, _ = BC.lidar_sub(3000)
    p = sicp.default_bootstrap_params(max_iterations=200, seed=7)
    off = sicp.default_bootstrap_label_params(match_same_label=0, score_same_label=0)
    with _engine(src, sl, tgt, tl) as e:
        plain = e.bootstrap(p)
        assert _same_result(e.bootstrap_semantic(p, off), plain)                      # a
    one_s, one_t = np.full(len(src), 4000000000, np.uint32), np.full(len(tgt), 4000000000, np.uint32)
    with _engine(src, one_s, tgt, one_t) as e:
        assert _same_result(e.bootstrap_semantic(p), plain)                           # b
    L = 4
    assert 0.05 < (sl == L).mean() < 0.5 and 0.05 < (tl == L).mean() < 0.5
    with _engine(src, sl, tgt, tl) as e, _engine(src[sl != L], sl[sl != L], tgt[tl != L], tl[tl != L]) as cut:
        ign = sicp.default_bootstrap_label_params(ignore=(L,), match_same_label=0, score_same_label=0)
        removed = cut.bootstrap(p)
        assert _same_result(e.bootstrap_semantic(p, ign), removed)                    # c
        assert removed[1]["n_source_keypoints"] < plain[1]["n_source_keypoints"]


# ---- 6. batch -------------------------------------------------------------------------------------------------------
def test_batch_rows_are_the_lone_calls_bit_for_bit():
    s, sl, t, tl, _ = SC.symmetric_scene()
    a_src, a_sl, a_tgt, a_tl, _ = BC.lidar_sub(3000)
    b_src, b_sl = BC.lidar_sub(2000)[:2]
    f_src, f_sl, f_tgt, f_tl = SC.too_few_pair()
    p = sicp.default_bootstrap_params(max_iterations=150, seed=SC.SEED)
    lp = sicp.default_bootstrap_label_params()
    with _engine(s, sl, t, tl) as e0, _engine(a_src, a_sl, a_tgt, a_tl) as e1, _engine(f_src, f_sl, f_tgt, f_tl) as e2, \
            sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e3:
        e3.set_source(b_src, b_sl)
        e3.share_cloud(sicp.TARGET, e1, sicp.TARGET)
        engines = [e0, e1, e2, e3]
        lone = []
        for e in engines:
            try:
                lone.append(e.bootstrap_semantic(p, lp))
            except sicp.SicpError as ex:
                lone.append(ex)
        res = sicp.bootstrap_semantic_batch(engines, p, lp)
        # the raw call: the failing pair's row and info stay as they were
        n = len(engines)
        out = np.full((n, 7), -7.5)
        status = np.full(n, -99, dtype=np.int32)
        infos = (sicp.SicpBootstrapInfo * n)()
        infos[2].best_iteration = -5
        hs = (C.c_void_p * n)(*[e._h for e in engines])
        rc = sicp.lib().sicp_bootstrap_semantic_batch(hs, n, C.byref(p), C.byref(lp), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                      status.ctypes.data_as(C.POINTER(C.c_int32)), infos)
    assert isinstance(lone[2], sicp.SicpError) and lone[2].status == sicp.ERR_TOO_FEW_POINTS
    assert [r[0] for r in res] == [sicp.OK, sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK]
    assert res[2][1] is None and "pair 2" in res[2][2]["error"]
    for i in (0, 1, 3):
        assert _same_result((res[i][1], res[i][2]), lone[i]), i
        assert np.array_equal(out[i], lone[i][0]) and infos[i].best_error == lone[i][1]["best_error"]
    assert rc == sicp.ERR_TOO_FEW_POINTS and list(status) == [sicp.OK, sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK]
    assert (out[2] == -7.5).all() and infos[2].best_iteration == -5


# ---- 7. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_handle_as_it_was():
    src, sl, tgt, tl, _ = BC.lidar_sub(3000)
    p = sicp.default_bootstrap_params()
    with _engine(src, sl, tgt, tl) as e, _engine(src, sl, tgt, tl) as fresh, _engine(src, None, tgt, tl) as bare:
        before = e.align(IDENT)
        cases = [(bare, sicp.default_bootstrap_label_params(), "no labels"),
                 (e, sicp.default_bootstrap_label_params(n_ignore=65), "n_ignore"),
                 (e, sicp.default_bootstrap_label_params(n_ignore=-1), "n_ignore"),
                 (e, sicp.default_bootstrap_label_params(match_same_label=2), "match_same_label"),
                 (e, sicp.default_bootstrap_label_params(score_same_label=2), "score_same_label")]
        for eng, lp, word in cases:
            with pytest.raises(sicp.SicpError) as ex:
                eng.bootstrap_semantic(p, lp)
            assert ex.value.status == sicp.ERR_INVALID_ARGUMENT and word in str(ex.value), str(ex.value)
            with pytest.raises(sicp.SicpError) as ex:
                eng.bootstrap_semantic_score(np.zeros((1, 3), np.int32), np.zeros((1, 3), np.int32), p, lp)
            assert ex.value.status == sicp.ERR_INVALID_ARGUMENT and word in str(ex.value), str(ex.value)
        # a NULL lp, through the raw entry points; nothing is written
        qt = np.full(7, -7.5)
        info = sicp.SicpBootstrapInfo()
        info.best_iteration = -5
        rc = sicp.lib().sicp_bootstrap_semantic(e._h, C.byref(p), None, qt.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
        assert rc == sicp.ERR_INVALID_ARGUMENT and "label params is NULL" in sicp.lib().sicp_last_error(e._h).decode()
        assert (qt == -7.5).all() and info.best_iteration == -5
        hs = (C.c_void_p * 1)(e._h)
        st = np.full(1, -99, dtype=np.int32)
        rc = sicp.lib().sicp_bootstrap_semantic_batch(hs, 1, C.byref(p), None, qt.ctypes.data_as(C.POINTER(C.c_double)),
                                                      st.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == sicp.ERR_INVALID_ARGUMENT and "label params is NULL" in sicp.lib().sicp_last_error(e._h).decode()
        assert (qt == -7.5).all() and st[0] == -99
        n = C.c_int32(-3)
        rc = sicp.lib().sicp_bootstrap_semantic_keypoints(e._h, sicp.SOURCE, C.byref(p), None, 0, C.byref(n), None, None)
        assert rc == sicp.ERR_INVALID_ARGUMENT and n.value == -3
        # in a batch a cloud without labels fails its own pair alone
        res = sicp.bootstrap_semantic_batch([bare, e], sicp.default_bootstrap_params(max_iterations=20))
        assert res[0][0] == sicp.ERR_INVALID_ARGUMENT and "no labels" in res[0][2]["error"] and res[1][0] == sicp.OK
        after = e.align(IDENT)
        qf = fresh.align(IDENT)
    assert np.array_equal(before[0], after[0]) and before[1]["outer_iters"] == after[1]["outer_iters"]
    assert np.array_equal(after[0], qf[0]) and after[1]["outer_iters"] == qf[1]["outer_iters"]
