"""CPU tests of the inputs of tests/test_gpu_bootstrap_semantic_edges.py (the second half of
tests/bootstrap_semantic_cases.py): every case builder reaches, in the numpy restatement alone, the branch it was built
for.  No GPU and no library."""
import numpy as np
import pytest

import bootstrap_cases as C
import bootstrap_ref as R
import bootstrap_semantic_cases as SC
import bootstrap_semantic_ref as S
from bootstrap_cases import TIE_PARAMS
from test_gpu_bootstrap_edges import KNN_CASES


def _sorted_labels(cloud, lab, ijk, ignore=()):
    """the labels of the points of voxel ijk in the order the voxel sort leaves them (ascending caller index)"""
    p, l = S.kept(cloud, lab, ignore=ignore)
    inside = (np.floor(p * (np.float32(1) / SC.LEAF)).astype(np.int64) == np.array(ijk)).all(axis=1)
    return l[inside]


# ---- A. the vote ------------------------------------------------------------------------------------------------------
def test_the_vote_edge_cloud_reaches_every_branch():
    cloud, lab, vox = SC.vote_edge_cloud()
    st = {}
    kp, kl = S.voxel_keypoints(cloud, lab, stats=st)
    assert len(kp) == len(vox)
    at = {k: SC.keypoint_at(kp, v[0]) for k, v in vox.items()}
    for name, (ijk, want) in vox.items():
        assert kl[at[name]] == want, name
    for n in SC.VOTE_COUNTS:
        ls = _sorted_labels(cloud, lab, vox[f"count{n}"][0])
        assert len(ls) == n == st["counts"][at[f"count{n}"]]
        # counts that differ by one, the larger label ahead, its surplus point last: without it the vote is a tie and goes
        # the other way
        assert (ls == 12).sum() == (ls == 11).sum() + 1 and ls[-1] == 12
        if n > 1:
            u, c = np.unique(ls[:-1], return_counts=True)
            assert u[np.argmax(c)] == 11
    assert st["n_labels"][at["distinct64"]] == 64 == st["counts"][at["distinct64"]] and st["ties"][at["distinct64"]]
    assert st["n_labels"][at["distinct65"]] == 65 == st["counts"][at["distinct65"]] and st["ties"][at["distinct65"]]
    assert st["n_labels"][at["twice"]] == 200 and st["counts"][at["twice"]] == 201 and not st["ties"][at["twice"]]
    assert 1000 < vox["twice"][1] < 1199
    # ties that the unsigned order decides; read as int32 the first and the third go the other way
    for name in ("mid", "high", "ends"):
        assert st["ties"][at[name]] and st["n_labels"][at[name]] == 2
        ls = _sorted_labels(cloud, lab, vox[name][0])
        assert kl[at[name]] == ls.min()
    assert kl[at["mid"]] == SC.MID and np.int32(SC.MID) > np.uint32(SC.HIGH).view(np.int32)
    assert kl[at["ends"]] == 0 and np.uint32(SC.BIG).view(np.int32) < 0
    assert kl[at["high"]] == SC.BIG - 1


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_small_vote_clouds_have_exactly_n_keypoints(n):
    cloud, lab, vox = SC.small_vote_cloud(n)
    st = {}
    kp, kl = S.voxel_keypoints(cloud, lab, stats=st)
    assert len(kp) == n
    for name, (ijk, want) in vox.items():
        assert kl[SC.keypoint_at(kp, ijk)] == want
    assert st["ties"].sum() == n // 2 and (st["n_labels"] == 2).all()


def test_the_full_ignore_list_reaches_every_branch():
    cloud, lab, vox = SC.full_ignore_cloud()
    ign = SC.FULL_IGNORE
    assert len(ign) == 64 and 0 in ign and SC.BIG in ign and len(set(ign)) < 64 and ign[-1] == 159
    st = {}
    kp, kl = S.voxel_keypoints(cloud, lab, ignore=ign, stats=st)
    kp0, kl0 = S.voxel_keypoints(cloud, lab)
    for name, (ijk, (with_list, without)) in vox.items():
        a, b = SC.keypoint_at(kp, ijk), SC.keypoint_at(kp0, ijk)
        assert kl0[b] == without, name
        assert (a is None) if with_list is None else kl[a] == with_list, name
    assert st["ties"][SC.keypoint_at(kp, vox["tie_after"][0])]
    assert len(kp) == len(kp0) - 1 and not np.isin(kl, ign).any()
    # dropping the list's last entry, or either extreme, changes the result
    for drop in (159, 0, SC.BIG):
        kl_d = S.voxel_keypoints(cloud, lab, ignore=[v for v in ign if v != drop])[1]
        assert len(kl_d) != len(kl) or not np.array_equal(kl_d, kl), drop
    # a list that holds every label of the cloud empties it
    all_listed = np.resize(np.array(ign, np.uint32), len(cloud))
    assert len(S.voxel_keypoints(cloud, all_listed, ignore=ign)[0]) == 0


def test_the_every_handle_cloud_is_permuted_by_a_label_grouped_layout():
    cloud, lab, vox = SC.vote_edge_cloud(distinct=False, nan_rows=9)
    assert np.isnan(cloud).any(axis=1).sum() == 9
    finite = np.isfinite(cloud).all(axis=1)
    first = {}
    for l in lab[finite]:
        first.setdefault(int(l), len(first))
    seg = np.array([first[int(l)] for l in lab[finite]])
    assert (np.diff(seg) < 0).sum() > 100  # grouping by label in order of first appearance moves hundreds of points
    kp, kl = S.voxel_keypoints(cloud, lab)
    for name, (ijk, want) in vox.items():
        assert kl[SC.keypoint_at(kp, ijk)] == want


# ---- B. the label k-NN ------------------------------------------------------------------------------------------------
def test_every_knn_pattern_applies_somewhere_and_votes_back():
    seen = {p: 0 for p in SC.KNN_PATTERNS}
    assert list(SC.KNN_APPLIES) == KNN_CASES
    for ns, nt, k, iso in KNN_CASES:
        for p in SC.KNN_PATTERNS:
            c = SC.knn_label_case(ns, nt, k, iso, p)
            assert (c is not None) == (p in SC.KNN_APPLIES[(ns, nt, k, iso)]), (ns, nt, k, iso, p)
            if c is None:
                continue
            seen[p] += 1
            skp, skl = S.voxel_keypoints(c["s"], c["sl"])
            tkp, tkl = S.voxel_keypoints(c["t"], c["tl"])
            assert (len(skp), len(tkp)) == (ns, nt)
            assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
    assert all(v >= 2 for v in seen.values()), seen


@pytest.mark.parametrize("ns,nt,k,iso", KNN_CASES)
def test_the_knn_label_patterns_reach_their_branches(ns, nt, k, iso):
    for p in SC.KNN_PATTERNS:
        c = SC.knn_label_case(ns, nt, k, iso, p)
        if c is None:
            continue
        skl, tkl, sf, tf = c["skl"], c["tkl"], c["sf"], c["tf"]
        knn = S.feature_knn(sf, tf, k, skl, tkl)
        sv, tv = ~np.isnan(sf[:, 0]), ~np.isnan(tf[:, 0])
        sel = knn >= 0
        assert (knn < nt).all() and (tkl[knn[sel]] == np.repeat(skl, k).reshape(-1, k)[sel]).all() and tv[knn[sel]].all()
        rows = sel.sum(axis=1)
        per = lambda lab: int((tv & (tkl == lab)).sum())
        for lab in np.unique(skl):
            assert (rows[sv & (skl == lab)] == min(k, per(lab))).all()
        if not sv.any() or not tv.any():
            assert (knn == -1).all()
            continue
        tile = lambda lab: set((np.flatnonzero(tv & (tkl == lab)) // 64).tolist())
        if p == "alternate":
            for t0 in range(0, nt, 64):
                assert nt - t0 < 2 or len(np.unique(tkl[t0:t0 + 64])) == 2
        elif p == "last_tile":
            # (where the cloud has keypoints without a feature they are its last ones: the label then has no feature at all)
            assert tile(5) <= {(nt - 1) // 64} and 0 < nt - (nt - 1) // 64 * 64 < 64 and (per(5) >= 1 or iso)
            assert set((np.flatnonzero(tkl == 5) // 64).tolist()) == {(nt - 1) // 64}
        elif p == "tile0":
            assert tile(5) == {0} and len(set((np.flatnonzero(tkl == 6) // 64).tolist())) >= 2 and (tkl[:64] == 6).any()
        elif p == "exact":
            assert [per(l) for l in (11, 12, 13)] == [k - 1, k, k + 1]
            full = lambda lab: (knn[sv & (skl == lab)] >= 0).all(axis=1)
            assert full(12).all() and full(13).all() and not full(11).any()
        elif p == "featureless":
            assert ((tkl == 5) & ~tv).sum() >= iso and per(5) == 2 and (rows[sv & (skl == 5)] == min(k, 2)).all()
        elif p == "absent":
            assert SC.ABSENT not in tkl and (sv & (skl == SC.ABSENT)).any() and (knn[skl == SC.ABSENT] == -1).all()
        elif p == "extremes":
            assert per(0) == 3 < k and 0 in tile(0) and tkl[nt - 1] == 0 and nt % 64 == 1  # 0 in the one-row last tile
            assert (rows[sv & (skl == 0)] == 3).all() and (tkl[tv] == SC.BIG).sum() > k


@pytest.mark.parametrize("kind", ["same", "split"])
def test_the_tie_label_cases_vote_back_and_split_the_twins(kind):
    c = SC.tie_label_case(kind)
    vk = dict(leaf=TIE_PARAMS["leaf_size"])
    skp, skl = S.voxel_keypoints(c["src"], c["sl"], **vk)
    tkp, tkl = S.voxel_keypoints(c["tgt"], c["tl"], **vk)
    m = c["m"]
    assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"]) and len(tkp) == 2 * m
    assert np.array_equal(tkp[:m], tkp[m:] - np.float32([0, 0, 8]))
    fk = dict(normal_radius=TIE_PARAMS["normal_radius"], feature_radius=TIE_PARAMS["feature_radius"])
    sf, tf = R.features(skp, **fk)["fpfh"], R.features(tkp, **fk)["fpfh"]
    twins = (tf[:m].view(np.uint32) == tf[m:].view(np.uint32)).all(axis=1) & ~np.isnan(tf[:m, 0])
    assert twins.mean() > 0.9
    knn = S.feature_knn(sf, tf, 2, skl, tkl)
    if kind == "same":
        assert np.array_equal(knn, R.feature_knn(sf, tf, 2))
        assert ((knn[:, 1] == knn[:, 0] + m) & twins[np.minimum(knn[:, 0], m - 1)]).mean() > 0.5
    else:
        blind = R.feature_knn(sf, tf, 1)[:, 0]
        two = skl == 2
        assert (knn[two] >= m).all() and (knn[~two] < m).all()
        # the label keeps the twin of the higher index where the blind search lists the lower
        moved = two & twins[blind % m] & (blind < m)
        assert moved.sum() > 50 and (knn[moved, 0] == blind[moved] + m).all()


# ---- C. the label-aware error -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", SC.ERROR_COUNTS)
def test_the_error_cases_have_inliers_of_the_right_and_of_the_wrong_label(ns):
    for pattern in SC.ERROR_PATTERNS + ("absent", "one"):
        c = SC.error_label_case(ns, pattern)
        skp, skl = S.voxel_keypoints(c["s"], c["sl"])
        tkp, tkl = S.voxel_keypoints(c["t"], c["tl"])
        assert len(skp) == ns and np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"]) and 300 <= len(tkp) <= 500
        tree = R.cKDTree(tkp.astype(np.float64))
        for nr in (3, 8):
            a, b = SC.near_samples(skp, tkp, nr)
            assert a.shape == b.shape == (8, nr)
            wrong, right = 0, 0
            for i in range(len(a)):
                M = R.umeyama(skp[a[i]], tkp[b[i]])
                e_on, w = S.truncated_error(M, skp, skl, tree, tkp, tkl, 0.8, True)
                e_off, _ = S.truncated_error(M, skp, skl, tree, tkp, tkl, 0.8, False)
                wrong += w
                right += e_on < ns
                if pattern == "absent":
                    assert e_on == ns and e_off < ns
                if pattern == "one":
                    assert w == 0 and e_on == e_off == R.truncated_error(M, skp, tree, tkp, 0.8)
            if pattern in SC.ERROR_PATTERNS:
                if ns > 1:
                    assert wrong >= 1 and right >= 1, (pattern, nr, wrong, right)
                else:  # the one keypoint lands on its nearest target keypoint: an inlier, refused in "wrong" alone
                    assert (wrong, right) == ((8, 0) if pattern == "wrong" else (0, 8)), (pattern, nr, wrong, right)
            if pattern == "absent":
                assert wrong >= 8  # every hypothesis has an inlier to refuse
        if pattern in SC.ERROR_PATTERNS and ns > 1:
            # scattered in space: neither cloud's labels come in runs of the caller order
            assert (np.diff(tkl.astype(np.int64)) != 0).mean() > 0.4 and (np.diff(skl.astype(np.int64)) != 0).mean() > 0.4


# ---- D. the whole call ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr", SC.SAC_SAMPLES)
@pytest.mark.parametrize("k", SC.SAC_KS)
def test_the_relabelled_pair_has_ragged_rows_and_no_ambiguous_iteration(nr, k):
    c = SC.relabelled_pair()
    has_f = ~np.isnan(c["sf"][:, 0])
    for m, s in SC.FLAG_SETS:
        knn = S.feature_knn(c["sf"], c["tf"], k, c["skl"], c["tkl"]) if m else R.feature_knn(c["sf"], c["tf"], k)
        for seed in SC.SAC_SEEDS:
            st = {}
            S.sac_ia(c["skp"], c["sf"], c["skl"], c["tkp"], c["tf"], c["tkl"], match_same_label=bool(m), score_same_label=bool(s),
                     knn=knn, stats=st, max_iterations=SC.SAC_ITERATIONS, nr_samples=nr, k_correspondences=k, seed=seed)
            assert st["ambiguous"] == [], (nr, k, seed, m, s)
            drawn = np.array([x for smp, _ in st["samples"] for x in smp])
            if m:
                assert st["unsampleable"] == (has_f & (c["skl"] == SC.ABSENT)).sum() > 0
                assert st["short_rows"] > 0 or k <= 3
                assert (c["skl"][drawn] == SC.RARE).any() and not (c["skl"][drawn] == SC.ABSENT).any()
            else:
                assert st["unsampleable"] == 0 and (c["skl"][drawn] == SC.ABSENT).any()
            if s:
                assert max(st["label_rejects"]) > 0


def test_the_refused_pairs_cannot_be_sampled_though_they_have_features():
    for nr in (3, 6, 8):
        c = SC.unsampleable_pair(nr)
        skp, skl = S.voxel_keypoints(c["src"], c["sl"])
        tkp, tkl = S.voxel_keypoints(c["tgt"], c["tl"])
        assert np.array_equal(skl, c["skl"]) and np.array_equal(tkl, c["tkl"])
        has_f = ~np.isnan(c["sf"][:, 0])
        assert (has_f & (skl == SC.REST)).sum() == nr - 1 == (skl == SC.REST).sum() and has_f.sum() > 100
        with pytest.raises(ValueError, match=f"{nr - 1} source keypoints"):
            S.sac_ia(skp, c["sf"], skl, tkp, c["tf"], tkl, nr_samples=nr, max_iterations=1)
        # one keypoint more and it runs
        S.sac_ia(skp, c["sf"], skl, tkp, c["tf"], tkl, nr_samples=max(nr - 1, 3), max_iterations=1) if nr > 3 else None
    d = SC.disjoint_pair()
    skp, skl = S.voxel_keypoints(d["src"], d["sl"])
    tkp, tkl = S.voxel_keypoints(d["tgt"], d["tl"])
    assert (~np.isnan(d["tf"][:, 0])).sum() > 100 and not np.isin(skl, tkl).any()
    with pytest.raises(ValueError, match="0 source keypoints"):
        S.sac_ia(skp, d["sf"], skl, tkp, d["tf"], tkl, max_iterations=1)


def test_the_increasing_map_keeps_the_order_and_reaches_the_top():
    c = SC.relabelled_pair()
    sl, tl = SC.increasing_map(c["sl"], c["tl"])
    both, mapped = np.r_[c["sl"], c["tl"]], np.r_[sl, tl]
    u, first = np.unique(both, return_index=True)
    assert (np.diff(mapped[first].astype(np.int64)) > 0).all() and mapped.max() == SC.BIG and len(np.unique(mapped)) == len(u)
    skp, skl = S.voxel_keypoints(c["src"], sl)
    assert np.array_equal(skl, SC.increasing_map(c["skl"], np.r_[c["sl"], c["tl"]])[0]) and (skl == SC.BIG).any() == (c["skl"].max() == both.max())
