"""GPU tests of the label-aware bootstrap (sicp_bootstrap_semantic, its batch and hooks) at the edges of its three kernels and
of the host logic that consumes them, against the numpy restatement tests/bootstrap_semantic_ref.py:
A. the label vote at point counts around the wave, voxels of distinct labels, ties that the unsigned order decides, clouds
   of 1 .. 5 keypoints, the full ignore list, every handle mode and slot;
B. the label k-NN at the keypoint counts of tests/test_gpu_bootstrap_edges.py under seven label patterns, exact ties between
   twins of one label and of two, and its two invariants against the blind table;
C. the label-aware error at source keypoint counts around the 256-lane stride, three and eight pairs a hypothesis;
D. the whole call on a pair whose neighbour rows are short or empty, its refusals, invariants and batch.
The inputs come from tests/bootstrap_semantic_cases.py, and tests/test_bootstrap_semantic_edges_cpu.py asserts on the CPU
that each reaches its branch.  The acceptance rules are those of tests/test_gpu_bootstrap_semantic.py and of _check_sac in
tests/test_gpu_bootstrap_edges.py: bits between library runs and for keypoints, labels, tables and counts; 1e-9 (relative to
max(1, |e|)) for errors against the restatement and 1e-9 for matrices.  A test cannot know the device order of a search
tree, so "rows from 256 on" are reached by counts: 257 rows that all hold an inlier of another label have one there."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import bootstrap_cases as K
import bootstrap_ref as R
import bootstrap_semantic_cases as SC
import bootstrap_semantic_ref as S
import test_gpu_bootstrap_semantic as G

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
MODES = (sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC)
IDENT = G.IDENT


def _bits(a):
    return (a.dtype, a.shape, a.tobytes())


def _same_pose_and_info(a, b):
    """two (qt, info) of library runs: pose and counts to the bit"""
    return np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and all(
        np.float64(a[1][k]).view(np.uint64) == np.float64(b[1][k]).view(np.uint64) for k in G.COUNTS)


def _no_hypotheses(p):
    z = np.zeros((0, p.nr_samples), np.int32)
    return z, z


def _features(e, p=None):
    skp, _, sf, _, _ = e.bootstrap_keypoints(sicp.SOURCE, p)
    tkp, _, tf, _, _ = e.bootstrap_keypoints(sicp.TARGET, p)
    return skp, sf, tkp, tf


# ---- A. the label vote ------------------------------------------------------------------------------------------------
def _vote(cloud, lab, ignore=(), mode=sicp.MODE_GICP, which=sicp.TARGET):
    lp = sicp.default_bootstrap_label_params(ignore=ignore)
    with G._engine(cloud, lab, cloud, lab, mode) as e:
        return e.bootstrap_semantic_keypoints(which, None, lp)


def _check_vote(cloud, lab, ignore=(), **kw):
    xyz, kl = _vote(cloud, lab, ignore, **kw)
    kp, rl = S.voxel_keypoints(cloud, lab, ignore=ignore)
    assert G._same_bits(xyz, kp) and kl.dtype == np.uint32 and np.array_equal(kl, rl)
    return xyz, kl


def test_vote_at_point_counts_distinct_labels_and_unsigned_ties():
    cloud, lab, vox = SC.vote_edge_cloud()
    xyz, kl = _check_vote(cloud, lab)
    got = {name: int(kl[SC.keypoint_at(xyz, ijk)]) for name, (ijk, _) in vox.items()}
    assert got == {name: want for name, (_, want) in vox.items()}


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_vote_of_a_cloud_of_a_few_keypoints(n):
    cloud, lab, vox = SC.small_vote_cloud(n)
    xyz, kl = _check_vote(cloud, lab)
    assert len(xyz) == n
    for name, (ijk, want) in vox.items():
        assert kl[SC.keypoint_at(xyz, ijk)] == want


def test_vote_under_a_full_ignore_list():
    cloud, lab, vox = SC.full_ignore_cloud()
    assert len(SC.FULL_IGNORE) == sicp.BOOTSTRAP_MAX_IGNORE
    xyz, kl = _check_vote(cloud, lab, SC.FULL_IGNORE)
    xyz0, kl0 = _check_vote(cloud, lab)
    for name, (ijk, (with_list, without)) in vox.items():
        at = SC.keypoint_at(xyz, ijk)
        assert (at is None) if with_list is None else kl[at] == with_list, name
        assert kl0[SC.keypoint_at(xyz0, ijk)] == without, name


def test_ignore_list_that_empties_the_cloud():
    cloud, _, _ = SC.full_ignore_cloud()
    lab = np.resize(np.array(SC.FULL_IGNORE, np.uint32), len(cloud))
    lp = sicp.default_bootstrap_label_params(ignore=SC.FULL_IGNORE)
    kp, rl = S.voxel_keypoints(cloud, lab, ignore=SC.FULL_IGNORE)
    assert len(kp) == 0 and np.isfinite(cloud).all(axis=1).any()
    with G._engine(cloud, lab, cloud, lab) as e:
        for which in (sicp.SOURCE, sicp.TARGET):
            xyz, kl = e.bootstrap_semantic_keypoints(which, None, lp)
            assert xyz.shape == kp.shape and kl.shape == rl.shape
        with pytest.raises(sicp.SicpError) as ex:
            e.bootstrap_semantic(None, lp)
        assert ex.value.status == sicp.ERR_TOO_FEW_POINTS
        # (without the list the same handle has keypoints)
        assert len(e.bootstrap_semantic_keypoints(sicp.SOURCE)[0]) > 0


def test_vote_gives_the_same_bytes_on_every_handle_and_slot():
    cloud, lab, vox = SC.vote_edge_cloud(distinct=False, nan_rows=9)
    outs = []
    for mode in MODES:
        with G._engine(cloud, lab, cloud, lab, mode) as e, sicp.Engine(0, sicp.default_params(mode)) as other:
            outs.append(e.bootstrap_semantic_keypoints(sicp.SOURCE))
            outs.append(e.bootstrap_semantic_keypoints(sicp.TARGET))
            other.share_cloud(sicp.SOURCE, e, sicp.TARGET)
            other.share_cloud(sicp.TARGET, e, sicp.SOURCE)
            outs.append(other.bootstrap_semantic_keypoints(sicp.SOURCE))
    kp, rl = S.voxel_keypoints(cloud, lab)
    assert G._same_bits(outs[0][0], kp) and np.array_equal(outs[0][1], rl)
    for o in outs[1:]:
        assert _bits(o[0]) == _bits(outs[0][0]) and _bits(o[1]) == _bits(outs[0][1])
    for name, (ijk, want) in vox.items():
        assert rl[SC.keypoint_at(kp, ijk)] == want


# ---- B. the label k-NN ------------------------------------------------------------------------------------------------
def _label_knn(src, sl, tgt, tl, k, params=None, lp=None, blind=False):
    """(GPU keypoint labels and features of both clouds, the label table, optionally the blind table)"""
    p = sicp.default_bootstrap_params(k_correspondences=k, **(params or {}))
    with G._engine(src, sl, tgt, tl) as e:
        skp, skl = e.bootstrap_semantic_keypoints(sicp.SOURCE, p)
        tkp, tkl = e.bootstrap_semantic_keypoints(sicp.TARGET, p)
        _, sf, _, tf = _features(e, p)
        _, _, knn = e.bootstrap_semantic_score(*_no_hypotheses(p), p, lp, n_source_keypoints=len(skp))
        knn0 = e.bootstrap_score(*_no_hypotheses(p), p, n_source_keypoints=len(skp))[2] if blind else None
    assert knn.shape == (len(skp), k)
    return dict(skl=skl, tkl=tkl, sf=sf, tf=tf, knn=knn, knn0=knn0)


@pytest.mark.parametrize("ns,nt,k,iso,pattern", SC.KNN_LABEL_CASES)
def test_label_knn_at_chosen_keypoint_counts(ns, nt, k, iso, pattern):
    c = SC.knn_label_case(ns, nt, k, iso, pattern)
    o = _label_knn(c["s"], c["sl"], c["t"], c["tl"], k)
    skl, tkl, knn = o["skl"], o["tkl"], o["knn"]
    assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"]) and (len(skl), len(tkl)) == (ns, nt)
    assert np.array_equal(knn, S.feature_knn(o["sf"], o["tf"], k, skl, tkl))
    # what the pattern is about, on the GPU's own features
    sv, tv = ~np.isnan(o["sf"][:, 0]), ~np.isnan(o["tf"][:, 0])
    sel = knn >= 0
    assert (knn < nt).all() and (knn >= -1).all() and tv[knn[sel]].all() and (tkl[knn[sel]] == np.repeat(skl, k).reshape(-1, k)[sel]).all()
    rows = sel.sum(axis=1)
    for lab in np.unique(skl):  # no row is longer (or shorter) than its label's target count allows
        assert (rows[sv & (skl == lab)] == min(k, int((tv & (tkl == lab)).sum()))).all()
    assert (rows[~sv] == 0).all()
    if pattern == "exact" and sv.any():
        assert [int((tv & (tkl == l)).sum()) for l in (11, 12, 13)] == [k - 1, k, k + 1]
    if pattern == "absent":
        assert (knn[skl == SC.ABSENT] == -1).all()
    if pattern == "extremes":
        assert (rows[sv & (skl == 0)] == 3).all() and sv[skl == 0].any()


@pytest.mark.parametrize("k", [1, 2, 10, 16])
@pytest.mark.parametrize("kind", ["same", "split"])
def test_label_knn_ties_between_twins(kind, k):
    c = SC.tie_label_case(kind)
    m = c["m"]
    o = _label_knn(c["src"], c["sl"], c["tgt"], c["tl"], k, K.TIE_PARAMS, blind=True)
    skl, tkl, tf, knn = o["skl"], o["tkl"], o["tf"], o["knn"]
    assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
    assert np.array_equal(knn, S.feature_knn(o["sf"], tf, k, skl, tkl))
    twins = (tf[:m].view(np.uint32) == tf[m:].view(np.uint32)).all(axis=1) & ~np.isnan(tf[:m, 0])
    assert twins.mean() > 0.9, twins.mean()
    if kind == "same":  # one label: the blind table, a twin pair lower index first
        assert np.array_equal(knn, o["knn0"])
        if k >= 2:
            first = knn[:, 0]
            assert ((knn[:, 1] == first + m) & twins[np.minimum(first, m - 1)]).mean() > 0.5
        else:
            assert (knn[:, 0] < m)[twins[knn[:, 0] % m]].all()
    else:  # two labels: every row holds the twins of its own label only -- the higher index where the blind search lists the lower
        two = skl == 2
        assert (knn[two] >= m).all() and (knn[~two] < m).all() and (knn >= 0).all()
        blind = o["knn0"][:, 0]
        moved = two & twins[blind % m] & (blind < m)
        assert moved.sum() > 50 and (knn[moved, 0] == blind[moved] + m).all()


@pytest.mark.parametrize("ns,nt,k,iso", list(SC.KNN_APPLIES))
def test_label_knn_is_the_blind_table_on_one_label_and_without_the_flag(ns, nt, k, iso):
    c = SC.knn_label_case(ns, nt, k, iso, "alternate")
    off = sicp.default_bootstrap_label_params(match_same_label=0)
    o = _label_knn(c["s"], c["sl"], c["t"], c["tl"], k, lp=off, blind=True)
    assert np.array_equal(o["knn"], o["knn0"]) and len(np.unique(o["skl"])) == min(ns, 2)
    one_s, one_t = np.full(len(c["s"]), SC.BIG, np.uint32), np.full(len(c["t"]), SC.BIG, np.uint32)
    one = _label_knn(c["s"], one_s, c["t"], one_t, k)
    assert np.array_equal(one["knn"], o["knn0"]) and (one["skl"] == SC.BIG).all()
    assert np.array_equal(o["knn0"], R.feature_knn(o["sf"], o["tf"], k))


# ---- C. the label-aware error -----------------------------------------------------------------------------------------
def _scores(c, nr, lp=None, blind=False):
    p = sicp.default_bootstrap_params(nr_samples=nr)
    with G._engine(c["s"], c["sl"], c["t"], c["tl"]) as e:
        skp, skl = e.bootstrap_semantic_keypoints(sicp.SOURCE, p)
        tkp, tkl = e.bootstrap_semantic_keypoints(sicp.TARGET, p)
        a, b = SC.near_samples(skp, tkp, nr)
        M, err, _ = e.bootstrap_semantic_score(a, b, p, lp)
        blind_out = e.bootstrap_score(a, b, p) if blind else None
    assert G._same_bits(skp, c["skp"]) and G._same_bits(tkp, c["tkp"])
    assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
    return dict(p=p, skp=skp, skl=skl, tkp=tkp, tkl=tkl, a=a, b=b, M=M, err=err, blind=blind_out)


@pytest.mark.parametrize("nr", [3, 8])
@pytest.mark.parametrize("pattern", SC.ERROR_PATTERNS)
@pytest.mark.parametrize("ns", SC.ERROR_COUNTS)
def test_label_error_at_chosen_source_keypoint_counts(ns, pattern, nr):
    o = _scores(SC.error_label_case(ns, pattern), nr)
    skp, skl, tkp, tkl = o["skp"], o["skl"], o["tkp"], o["tkl"]
    tree = R.cKDTree(tkp.astype(np.float64))
    wrong = right = 0
    for i in range(len(o["a"])):
        if R.fit_rank_ratio(skp[o["a"][i]], tkp[o["b"][i]]) >= 1e-6:  # (one optimal transform: any two solvers agree on it)
            assert np.abs(o["M"][i] - R.umeyama(skp[o["a"][i]], tkp[o["b"][i]])).max() < 1e-9
        else:
            assert ns < nr
        er, w = S.truncated_error(o["M"][i], skp, skl, tree, tkp, tkl, o["p"].max_corr_distance, True)
        assert abs(o["err"][i] - er) <= 1e-9 * max(1.0, abs(er)), (i, o["err"][i], er)
        wrong += w
        right += er < ns
    assert wrong >= 1 or (ns == 1 and pattern == "scatter")
    assert right >= 1 or (ns == 1 and pattern == "wrong")


@pytest.mark.parametrize("nr", [3, 8])
@pytest.mark.parametrize("ns", SC.ERROR_COUNTS)
def test_label_error_is_the_row_count_when_the_target_has_none_of_the_source_labels(ns, nr):
    o = _scores(SC.error_label_case(ns, "absent"), nr, blind=True)
    assert not np.isin(o["skl"], o["tkl"]).any()
    assert (o["err"] == float(ns)).all(), o["err"]  # every term is 1.0
    assert (o["blind"][1] < ns).all()               # (and every hypothesis had an inlier to refuse)


@pytest.mark.parametrize("ns", SC.ERROR_COUNTS)
def test_label_error_is_the_blind_error_on_one_label_and_without_the_flag(ns):
    one = _scores(SC.error_label_case(ns, "one"), 3, blind=True)
    assert _bits(one["err"]) == _bits(one["blind"][1]) and _bits(one["M"]) == _bits(one["blind"][0])
    off = sicp.default_bootstrap_label_params(score_same_label=0)
    o = _scores(SC.error_label_case(ns, "wrong"), 3, lp=off, blind=True)
    assert _bits(o["err"]) == _bits(o["blind"][1]) and _bits(o["err"]) == _bits(one["err"])
    on = _scores(SC.error_label_case(ns, "wrong"), 3)
    assert (on["err"] > o["err"]).any()


# ---- D. the whole call on ragged rows ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _relabelled():
    """the GPU's keypoints, labels and features of relabelled_pair() -- computed once, and left unchanged"""
    c = SC.relabelled_pair()
    with G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e:
        skp, skl = e.bootstrap_semantic_keypoints(sicp.SOURCE)
        tkp, tkl = e.bootstrap_semantic_keypoints(sicp.TARGET)
        _, sf, _, tf = _features(e)
    assert G._same_bits(skp, c["skp"]) and G._same_bits(tkp, c["tkp"]) and np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
    return dict(skp=skp, skl=skl, tkp=tkp, tkl=tkl, sf=sf, tf=tf)


@functools.lru_cache(maxsize=None)
def _relabelled_knn(k, match):
    g = _relabelled()
    return S.feature_knn(g["sf"], g["tf"], k, g["skl"], g["tkl"]) if match else R.feature_knn(g["sf"], g["tf"], k)


@pytest.mark.parametrize("seed", SC.SAC_SEEDS)
@pytest.mark.parametrize("k", SC.SAC_KS)
@pytest.mark.parametrize("nr", SC.SAC_SAMPLES)
def test_whole_call_on_short_and_empty_rows(nr, k, seed):
    c, g = SC.relabelled_pair(), _relabelled()
    kw = dict(max_iterations=SC.SAC_ITERATIONS, nr_samples=nr, k_correspondences=k, seed=seed)
    p = sicp.default_bootstrap_params(**kw)
    has_f = ~np.isnan(g["sf"][:, 0])
    with G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e:
        runs = [e.bootstrap_semantic(p, sicp.default_bootstrap_label_params(match_same_label=m, score_same_label=s))
                for m, s in SC.FLAG_SETS]
    for (m, s), (qt, info) in zip(SC.FLAG_SETS, runs):
        assert info["n_source_keypoints"] == len(g["skp"]) and info["n_target_keypoints"] == len(g["tkp"])
        stats = {}
        best, err, errs, Ms = S.sac_ia(g["skp"], g["sf"], g["skl"], g["tkp"], g["tf"], g["tkl"], match_same_label=bool(m),
                                       score_same_label=bool(s), knn=_relabelled_knn(k, m), stats=stats, **kw)
        assert stats["ambiguous"] == [], (m, s, stats["ambiguous"])
        gb = info["best_iteration"]
        assert 0 <= gb < len(errs)
        assert gb == best or abs(errs[gb] - err) <= 1e-9 * max(1.0, err), (m, s, gb, best)
        assert abs(info["best_error"] - errs[gb]) <= 1e-9 * max(1.0, errs[gb]), (m, s)
        assert np.abs(G._mat(qt)[:3] - Ms[gb]).max() < 1e-9, (m, s)
        drawn = np.array([x for smp, _ in stats["samples"] for x in smp])
        if m:
            assert stats["unsampleable"] == (has_f & (g["skl"] == SC.ABSENT)).sum() > 0
            assert stats["short_rows"] > 0 or k <= 3
            assert (g["skl"][drawn] == SC.RARE).any() and not (g["skl"][drawn] == SC.ABSENT).any()
        else:
            assert stats["unsampleable"] == 0


def _raw_call(e, p, lp):
    """sicp_bootstrap_semantic through the raw entry point: (status, out_qt, info) with out_qt and info pre-filled"""
    qt = np.full(7, -7.5)
    info = sicp.SicpBootstrapInfo()
    info.best_iteration = -5
    info.best_error = -2.5
    rc = sicp.lib().sicp_bootstrap_semantic(e._h, C.byref(p), C.byref(lp), qt.ctypes.data_as(C.POINTER(C.c_double)), C.byref(info))
    return rc, qt, info


@pytest.mark.parametrize("nr", [3, 6, 8])
def test_too_few_sampleable_keypoints_are_refused_and_nothing_is_written(nr):
    c, d = SC.unsampleable_pair(nr), SC.disjoint_pair()
    p = sicp.default_bootstrap_params(nr_samples=nr, max_iterations=20)
    lp = sicp.default_bootstrap_label_params()
    with G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e, G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as fresh, \
            G._engine(d["src"], d["sl"], d["tgt"], d["tl"]) as e2:
        before = e.align(IDENT)
        skl = e.bootstrap_semantic_keypoints(sicp.SOURCE)[1]
        _, sf, _, tf = _features(e)
        has_f = ~np.isnan(sf[:, 0])
        assert (has_f & (skl == SC.REST)).sum() == nr - 1 and (has_f & (skl == SC.ABSENT)).sum() > 100
        for eng in (e, e2):
            rc, qt, info = _raw_call(eng, p, lp)
            assert rc == sicp.ERR_TOO_FEW_POINTS and (qt == -7.5).all() and info.best_iteration == -5 and info.best_error == -2.5
            with pytest.raises(sicp.SicpError) as ex:
                eng.bootstrap_semantic(p, lp)
            assert ex.value.status == sicp.ERR_TOO_FEW_POINTS
        assert (~np.isnan(tf[:, 0])).sum() > 100
        # the same clouds are enough without the matching rule, and with one sample fewer
        ok = e.bootstrap_semantic(p, sicp.default_bootstrap_label_params(match_same_label=0))
        assert ok[1]["n_source_keypoints"] == len(skl)
        if nr > 3:
            e.bootstrap_semantic(sicp.default_bootstrap_params(nr_samples=nr - 1, max_iterations=2), lp)
        after = e.align(IDENT)
        qf = fresh.align(IDENT)
    assert np.array_equal(before[0], after[0]) and before[1]["outer_iters"] == after[1]["outer_iters"]
    assert np.array_equal(after[0], qf[0]) and after[1]["outer_iters"] == qf[1]["outer_iters"]


SAC_P = dict(max_iterations=SC.SAC_ITERATIONS, nr_samples=6, k_correspondences=10, seed=2)


def test_whole_call_is_unchanged_by_an_increasing_label_map():
    c = SC.relabelled_pair()
    sl, tl = SC.increasing_map(c["sl"], c["tl"])
    assert (sl == SC.BIG).any() or (tl == SC.BIG).any()
    p = sicp.default_bootstrap_params(**SAC_P)
    with G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e, G._engine(c["src"], sl, c["tgt"], tl) as f:
        for m, s in SC.FLAG_SETS:
            lp = sicp.default_bootstrap_label_params(match_same_label=m, score_same_label=s)
            assert _same_pose_and_info(e.bootstrap_semantic(p, lp), f.bootstrap_semantic(p, lp)), (m, s)
        kl = f.bootstrap_semantic_keypoints(sicp.SOURCE)[1]
    assert np.array_equal(kl, SC.increasing_map(c["skl"], np.r_[c["sl"], c["tl"]])[0])


def test_ignoring_a_label_with_both_flags_on_is_the_call_without_its_points():
    src, sl, tgt, tl, _ = K.lidar_sub(3000)
    p = sicp.default_bootstrap_params(max_iterations=100, seed=7)
    L = 4
    assert 0.05 < (sl == L).mean() < 0.5 and 0.05 < (tl == L).mean() < 0.5
    # the list also names labels the clouds do not have, and L twice
    lp = sicp.default_bootstrap_label_params(ignore=(4000000000, L, 123456, L))
    with G._engine(src, sl, tgt, tl) as e, G._engine(src[sl != L], sl[sl != L], tgt[tl != L], tl[tl != L]) as cut:
        whole = e.bootstrap_semantic(p)
        ignored = e.bootstrap_semantic(p, lp)
        removed = cut.bootstrap_semantic(p)
    assert _same_pose_and_info(ignored, removed)
    assert removed[1]["n_source_keypoints"] < whole[1]["n_source_keypoints"]


def test_whole_call_gives_the_same_bytes_on_every_handle_and_twice():
    c = SC.relabelled_pair()
    p = sicp.default_bootstrap_params(**SAC_P)
    outs = []
    for mode in MODES:
        with G._engine(c["src"], c["sl"], c["tgt"], c["tl"], mode) as e:
            outs += [e.bootstrap_semantic(p), e.bootstrap_semantic(p)]
            M, err, knn = e.bootstrap_semantic_score(*SC.near_identity_samples(c["skp"], c["tkp"]), None, None, n_source_keypoints=len(c["skp"]))
            outs[-1] = outs[-1] + (M, err, knn)
    for o in outs[1:]:
        assert _same_pose_and_info(o, outs[0])
    for o in outs[3::2]:
        for x, y in zip(o[2:], outs[1][2:]):
            assert _bits(x) == _bits(y)


def test_batch_over_ragged_refused_shared_and_semantic_pairs_equals_the_lone_calls():
    c, u, d = SC.relabelled_pair(), SC.unsampleable_pair(6), SC.disjoint_pair()
    b_src, b_sl = K.lidar_sub(2000)[:2]
    b_sl = SC.labels_by_keypoint(b_src, np.array([SC.STRADDLE, SC.REST, SC.ABSENT], np.uint32)[np.arange(len(R.voxel_keypoints(b_src))) % 3])
    p = sicp.default_bootstrap_params(**SAC_P)
    lp = sicp.default_bootstrap_label_params()
    with G._engine(c["src"], c["sl"], c["tgt"], c["tl"]) as e0, G._engine(u["src"], u["sl"], u["tgt"], u["tl"]) as e1, \
            G._engine(c["src"], c["sl"], c["tgt"], c["tl"], sicp.MODE_SEMANTIC) as e2, \
            G._engine(d["src"], d["sl"], d["tgt"], d["tl"]) as e3, sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e4:
        e4.set_source(b_src, b_sl)
        e4.share_cloud(sicp.TARGET, e0, sicp.TARGET)
        engines = [e0, e1, e2, e3, e4]
        lone = []
        for e in engines:
            try:
                lone.append(e.bootstrap_semantic(p, lp))
            except sicp.SicpError as ex:
                lone.append(ex)
        res = sicp.bootstrap_semantic_batch(engines, p, lp)
        n = len(engines)
        out = np.full((n, 7), -7.5)
        status = np.full(n, -99, dtype=np.int32)
        infos = (sicp.SicpBootstrapInfo * n)()
        for i in (1, 3):
            infos[i].best_iteration = -5
        hs = (C.c_void_p * n)(*[e._h for e in engines])
        rc = sicp.lib().sicp_bootstrap_semantic_batch(hs, n, C.byref(p), C.byref(lp), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                      status.ctypes.data_as(C.POINTER(C.c_int32)), infos)
    want = [sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.OK]
    assert [r[0] for r in res] == want and list(status) == want and rc == sicp.ERR_TOO_FEW_POINTS
    for i in (1, 3):
        assert isinstance(lone[i], sicp.SicpError) and lone[i].status == sicp.ERR_TOO_FEW_POINTS
        assert res[i][1] is None and f"pair {i}" in res[i][2]["error"]
        assert (out[i] == -7.5).all() and infos[i].best_iteration == -5
    assert "5 source" in res[1][2]["error"] and "0 source" in res[3][2]["error"]
    for i in (0, 2, 4):
        assert _same_pose_and_info((res[i][1], res[i][2]), lone[i]), i
        assert np.array_equal(out[i].view(np.uint64), lone[i][0].view(np.uint64))
        assert np.float64(infos[i].best_error).view(np.uint64) == np.float64(lone[i][1]["best_error"]).view(np.uint64)
    assert _same_pose_and_info(lone[2], lone[0])  # the SEMANTIC handle holds the first pair's clouds
    assert not np.array_equal(lone[4][0], lone[0][0])
