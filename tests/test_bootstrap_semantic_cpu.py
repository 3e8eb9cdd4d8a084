"""CPU tests of the label-aware bootstrap's numpy restatement (tests/bootstrap_semantic_ref.py) and of the inputs the GPU
tests use (tests/bootstrap_semantic_cases.py): on a single label it is bootstrap_ref exactly, its label vote is
merge_ref's, the symmetric scene behaves as the GPU test relies on, and every crafted case reaches its branch.  No GPU
and no library."""
import numpy as np

import bootstrap_cases as C
import bootstrap_ref as R
import bootstrap_semantic_cases as SC
import bootstrap_semantic_ref as S
import merge_ref


def test_on_a_single_label_the_restatement_is_bootstrap_ref_exactly():
    src, _, tgt, _, _ = C.lidar_sub(2000)
    one_s, one_t = np.full(len(src), 6, np.uint32), np.full(len(tgt), 6, np.uint32)
    skp, skl = S.voxel_keypoints(src, one_s)
    tkp, tkl = S.voxel_keypoints(tgt, one_t)
    assert np.array_equal(skp.view(np.uint32), R.voxel_keypoints(src).view(np.uint32)) and (skl == 6).all() and (tkl == 6).all()
    sf, tf = R.features(skp)["fpfh"], R.features(tkp)["fpfh"]
    assert np.array_equal(S.feature_knn(sf, tf, 10, skl, tkl), R.feature_knn(sf, tf, 10))
    kw = dict(max_iterations=60, seed=5)
    a_stats, b_stats = {}, {}
    a = S.sac_ia(skp, sf, skl, tkp, tf, tkl, stats=a_stats, **kw)
    b = R.sac_ia(skp, sf, tkp, tf, stats=b_stats, **kw)
    assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a_stats["samples"] == b_stats["samples"] and a_stats["draws"] == b_stats["draws"]
    assert a_stats["short_rows"] == 0 and a_stats["unsampleable"] == 0 and max(a_stats["label_rejects"]) == 0


def test_keypoint_labels_are_merge_refs_vote_on_the_same_voxels():
    for cloud, lab, ignore in ((C.lidar_sub(2000)[0], C.lidar_sub(2000)[1], ()), SC.vote_cloud()[:2] + ((),),
                               SC.vote_cloud()[:2] + ((SC.IGNORED,),)):
        kp, kl = S.voxel_keypoints(cloud, lab, ignore=ignore)
        p, l = S.kept(cloud, lab, ignore=ignore)
        m = merge_ref.merge([(p, l)], leaf=0.4)
        # merge_ref orders its voxels by (vz, vy, vx) on an absolute grid: the bootstrap's ascending index on its own
        assert m["n_out"] == len(kp)
        assert np.array_equal(m["xyz"].view(np.uint32), kp.view(np.uint32))
        assert np.array_equal(m["labels"], kl)


def test_the_vote_cloud_reaches_every_branch():
    cloud, lab, vox = SC.vote_cloud()
    assert np.isnan(cloud).any() and np.isinf(cloud).any()
    st, st_i = {}, {}
    kp, kl = S.voxel_keypoints(cloud, lab, stats=st)
    kpi, kli = S.voxel_keypoints(cloud, lab, ignore=(SC.IGNORED,), stats=st_i)
    at = {k: SC.keypoint_at(kp, v) for k, v in vox.items()}
    ati = {k: SC.keypoint_at(kpi, v) for k, v in vox.items()}
    # a 2-2 tie goes to the smaller label
    assert st["counts"][at["tie"]] == 4 and st["ties"][at["tie"]] and kl[at["tie"]] == 3
    # a voxel of 300 points with three labels
    assert st["counts"][at["crowd"]] == 300 and st["n_labels"][at["crowd"]] == 3 and kl[at["crowd"]] == 5
    # the labels 0 and 2^32 - 1, each winning a voxel against the other
    assert kl[at["extremes"]] == 0 and kl[at["top"]] == SC.BIG
    # ignoring a label empties one voxel and changes another's winner
    assert at["emptied"] is not None and ati["emptied"] is None and len(kpi) < len(kp)
    assert kl[at["swayed"]] == SC.IGNORED and kli[ati["swayed"]] == 5
    assert SC.IGNORED not in kli
    # small voxels beside the crowd: the vote runs over two points and over several hundred
    assert st["counts"].min() == 1 and st["counts"][at["pair"]] == 2 and st["ties"][at["pair"]] and kl[at["pair"]] == 2
    assert st["counts"][at["edge"]] == 65 and kl[at["edge"]] == 4


def test_the_symmetric_scene_fools_the_label_blind_bootstrap_only():
    ref = SC.symmetric_reference()
    assert len(ref["skp"]) == 1705 and len(ref["tkp"]) == 1930
    T = ref["T"]
    b_best, _, _, b_M = ref["blind"]
    a_best, _, _, a_M = ref["aware"]
    rot, tr = SC.mat_delta(T, SC.mat4(b_M[b_best]))
    assert rot > 170.0, (rot, tr)
    rot, tr = SC.mat_delta(T, SC.mat4(a_M[a_best]))
    assert rot < 5.0 and tr < 1.0, (rot, tr)
    assert b_best not in ref["blind_stats"]["ambiguous"] and a_best not in ref["aware_stats"]["ambiguous"]
    # the labels decide through both rules: the aware run rejects inliers of the other label in its hypotheses
    assert max(ref["aware_stats"]["label_rejects"]) > 0


def test_the_relabelled_pair_reaches_every_branch_of_the_label_knn():
    c = SC.relabelled_pair()
    k = 10
    # the point labels vote back to the keypoint labels they were built from
    skp, skl = S.voxel_keypoints(c["src"], c["sl"])
    tkp, tkl = S.voxel_keypoints(c["tgt"], c["tl"])
    assert np.array_equal(skp.view(np.uint32), c["skp"].view(np.uint32)) and np.array_equal(skl, c["skl"])
    assert np.array_equal(tkp.view(np.uint32), c["tkp"].view(np.uint32)) and np.array_equal(tkl, c["tkl"])
    assert len(tkp) > 64 * 4
    knn = S.feature_knn(c["sf"], c["tf"], k, skl, tkl)
    has_f = ~np.isnan(c["sf"][:, 0])
    # a source label absent from the target: rows all -1, never sampled
    absent = skl == SC.ABSENT
    assert (has_f & absent).sum() > 0 and (knn[absent] == -1).all() and SC.ABSENT not in tkl
    # a label with three target keypoints with a feature, fewer than k: rows end in -1
    rare = has_f & (skl == SC.RARE)
    assert rare.sum() > 0 and ((knn[rare] >= 0).sum(axis=1) == 3).all() and (knn[rare][:, 3:] == -1).all()
    assert np.array_equal(np.sort(knn[rare][:, :3], axis=1), np.tile(np.sort(c["rare"]), (rare.sum(), 1)))
    # a label whose target keypoints straddle tile boundaries: its rows hold neighbours from several 64-row tiles
    straddle = has_f & (skl == SC.STRADDLE)
    tiles = np.unique(knn[straddle] // 64)
    assert (tkl[knn[straddle]] == SC.STRADDLE).all() and len(tiles) >= 3 and set(np.flatnonzero(tkl == SC.STRADDLE) // 64) == {0, 1, 2, 3}
    # and every other row holds its own label only
    sel = knn >= 0
    assert (tkl[knn[sel]] == np.repeat(skl, k).reshape(-1, k)[sel]).all()
    st = {}
    S.sac_ia(skp, c["sf"], skl, tkp, c["tf"], tkl, knn=knn, stats=st, max_iterations=40)
    assert st["unsampleable"] == (has_f & absent).sum() and st["short_rows"] >= rare.sum()
    assert not np.isin(np.flatnonzero(absent), [s for smp, _ in st["samples"] for s in smp]).any()
    assert any(skl[s] == SC.RARE for smp, _ in st["samples"] for s in smp)


def test_the_score_hypotheses_meet_inliers_of_another_label():
    c = SC.relabelled_pair()
    a, b = SC.near_identity_samples(c["skp"], c["tkp"])
    assert len(a) == 8
    tree = R.cKDTree(c["tkp"].astype(np.float64))
    wrong = []
    for i in range(len(a)):
        M = R.umeyama(c["skp"][a[i]], c["tkp"][b[i]])
        e_on, w = S.truncated_error(M, c["skp"], c["skl"], tree, c["tkp"], c["tkl"], 0.8, True)
        e_off, _ = S.truncated_error(M, c["skp"], c["skl"], tree, c["tkp"], c["tkl"], 0.8, False)
        assert e_off == R.truncated_error(M, c["skp"], tree, c["tkp"], 0.8)
        assert e_on >= e_off and (e_on > e_off) == (w > 0)
        wrong.append(w)
    assert min(wrong) >= 1, wrong


def test_the_too_few_pair_cannot_be_sampled():
    s, sl, t, tl = SC.too_few_pair()
    skp, _ = S.voxel_keypoints(s, sl)
    assert len(skp) == 1 or len(skp) == 2
    assert len(skp) < R.DEFAULTS["nr_samples"]
