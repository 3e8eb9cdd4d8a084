"""CPU tests of the sicp_filter restatement (tests/filter_ref.py) and of the cases the GPU tests run (tests/filter_cases.py): the
fast form -- k-d tree candidates, decided by the float32 arithmetic -- agrees with the form that looks at every pair; the lists
agree with cKDTree's own neighbours recomputed by the float32 formula and with search_cases.np_knn; the tree sum agrees with one
Python add per node; and no case is degenerate in the wrong way."""
import importlib
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

import cluster_ref
import filter_cases
import filter_ref
import search_cases

ARRAYS = ("keep", "mean_dist", "neighbors", "xyz_kept")
FIELDS = ("n_points", "n_finite", "n_tested", "n_protected", "n_kept", "n_fail_stat", "n_fail_radius", "mean", "stddev", "threshold")


def _same(a, b):
    for k in ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["labels_kept"] is None) == (b["labels_kept"] is None)
    if a["labels_kept"] is not None:
        assert a["labels_kept"].tobytes() == b["labels_kept"].tobytes()
    for k in FIELDS:
        assert np.array(a[k]).tobytes() == np.array(b[k]).tobytes(), k


@pytest.mark.parametrize("name", filter_cases.NAMES)
def test_fast_form_equals_the_form_without_a_tree(name):
    """on every case (the large ones cut to their first 1500 points) the two statements of the rules give the same bytes"""
    c = filter_cases.small(name)
    fast = filter_ref.filter(c["xyz"], c["labels"], c["mask"], **c["params"])
    if c is filter_cases.case(name):
        _same(fast, filter_cases.reference(name))
    _same(fast, filter_ref.filter_slow(c["xyz"], c["labels"], c["mask"], **c["params"]))


@pytest.mark.parametrize("name", filter_cases.STREET[:1] + ["duplicates", "nan_mix", "interleaved", "mean_k_31"])
def test_lists_equal_the_tree_neighbours_in_float32(name):
    """cKDTree's own k nearest neighbours (double), their distances recomputed by the float32 formula, give the reference's
    mean distances wherever the double and the float32 order agree on the list's contents -- checked on 400 tested points per
    case against search_cases.np_knn, the search tests' statement of the same list, which decides every tie"""
    c, ref = filter_cases.case(name), filter_cases.reference(name)
    k = c["params"]["mean_k"]
    fin = np.flatnonzero(np.isfinite(c["xyz"]).all(axis=1))
    pts = c["xyz"][fin]
    tested = np.flatnonzero(~np.isnan(ref["mean_dist"]))
    pick = tested[:: max(1, len(tested) // 400)]
    q = c["xyz"][pick]
    _, d2 = search_cases.np_knn(q, pts, k + 1)
    want = filter_ref.mean_dist_of_lists(d2, k)
    assert want.tobytes() == ref["mean_dist"][pick].tobytes()
    _, idx = cKDTree(pts.astype(np.float64)).query(q.astype(np.float64), k=k + 1)
    near = np.sort(cluster_ref.d2_f32(q[:, None, :], pts[idx.reshape(len(q), k + 1)]), axis=1)
    agree = (near == d2).all(axis=1)
    assert agree.mean() > 0.9
    assert filter_ref.mean_dist_of_lists(near, k)[agree].tobytes() == ref["mean_dist"][pick][agree].tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13, 64, 100, 511, 512, 513])
def test_tree_sum_equals_one_add_per_node(n):
    rng = np.random.default_rng(n)
    v = rng.uniform(0, 3, n) ** 3
    present = rng.random(n) < 0.7
    got = filter_ref.tree_sum(v, present, n)
    assert got == filter_ref.tree_sum_slow(v, present, n)
    assert got == pytest.approx(math.fsum(v[present]), rel=1e-13)


def test_tree_shape_is_the_callers_index_range():
    """an entry's place in the tree is its caller index: moving the same values to other indices may change the sum's bits, and
    padding the range to the next power of two never does"""
    rng = np.random.default_rng(5)
    v = rng.uniform(0, 1, 700)
    all_ = np.ones(700, bool)
    a = filter_ref.tree_sum(v, all_, 700)
    assert a == filter_ref.tree_sum(np.concatenate([v, np.zeros(324)]), np.concatenate([all_, np.zeros(324, bool)]), 1024)
    sums = {filter_ref.tree_sum(v[rng.permutation(700)], all_, 700) for _ in range(20)}
    assert len(sums) > 1


def test_no_case_is_degenerate():
    for name in filter_cases.REALISTIC:
        c, r = filter_cases.case(name), filter_cases.reference(name)
        p = c["params"]
        assert r["n_tested"] > r["n_fail_stat"] + r["n_fail_radius"], name
        if p["mean_k"] > 0:
            assert 0 < r["n_fail_stat"] < r["n_tested"], name
        if p["radius"] > 0:
            assert 0 < r["n_fail_radius"] < r["n_tested"], name
        assert 0 < r["n_kept"] < r["n_points"], name
    # the planted points of the street scan are what the tests are for: each removes most of them and keeps most of the scene
    xyz, lab = filter_cases._street_scan()
    for name in filter_cases.STREET:
        r = filter_cases.reference(name)
        planted = (lab == 9) & (r["keep"] == 0)
        assert planted.sum() >= 40 and r["n_kept"] > 0.5 * len(xyz), name


def test_edge_cases_are_what_they_claim():
    r = filter_cases.reference("two_points")
    assert r["mean_dist"][0] == r["mean_dist"][1] == r["threshold"] and r["keep"].tolist() == [1, 1] and r["stddev"] == 0.0
    r = filter_cases.reference("clamped")
    assert r["raw_variance"] < 0.0 and r["stddev"] == 0.0 and r["threshold"] == r["mean"]
    assert filter_cases.search_clamped() == filter_cases.CLAMPED
    r = filter_cases.reference("duplicates")
    assert (r["mean_dist"] == 0.0).sum() >= 150 and (r["neighbors"] == 4).sum() >= 150
    r = filter_cases.reference("radius_edge")
    assert r["neighbors"].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    r = filter_cases.reference("dense")
    assert (r["neighbors"] == 7).sum() == 5000 and (r["neighbors"] == 0).sum() == 1
    c, r = filter_cases.case("faces"), filter_cases.reference("faces")  # nothing saturates, and the pairs fall on both sides of r
    joined = cluster_ref.d2_f32(c["xyz"][0::2], c["xyz"][1::2]) < cluster_ref.t2_of(filter_cases.R)
    assert 0 <= r["neighbors"].min() and r["neighbors"].max() < 12 and 10 < joined.sum() < len(joined) - 10
    c = filter_cases.case("interleaved")
    assert sorted(np.bincount(c["labels"])[1:].tolist()) == [5, 447, 448] and c["params"]["mean_k"] + 1 > 5
    for k in filter_cases.MEAN_KS:
        c = filter_cases.case(f"exact_count_{k}")
        assert np.isfinite(c["xyz"]).all(axis=1).sum() == k + 1 < len(c["xyz"])
        few = filter_cases.too_few(k)
        assert np.isfinite(few["xyz"]).all(axis=1).sum() == k
        with pytest.raises(filter_ref.TooFewPoints):
            filter_ref.filter(few["xyz"], few["labels"], few["mask"], **few["params"])
    for n in filter_cases.TREE_SIZES:
        c, r = filter_cases.case(f"tree_{n}"), filter_cases.reference(f"tree_{n}")
        assert len(c["xyz"]) == n and 0 < r["n_tested"] < r["n_finite"] < n and r["n_protected"] > 0


def test_refusals_of_the_restatement():
    c = filter_cases.case("select_mask")
    with pytest.raises(ValueError):
        filter_ref.filter(c["xyz"], c["labels"], drop=(1, 2), protect=(2,))
    with pytest.raises(ValueError):
        filter_ref.filter(c["xyz"], None, drop=(1,), mean_k=0)
    with pytest.raises(ValueError):
        filter_ref.filter(c["xyz"], c["labels"], mean_k=32)
    with pytest.raises(ValueError):
        filter_ref.filter(c["xyz"], c["labels"], mean_k=0, radius=0.5, min_neighbors=0)
    with pytest.raises(filter_ref.TooFewPoints):
        filter_ref.filter(c["xyz"], c["labels"], mean_k=4, mask=np.zeros(300, np.uint8))
    with pytest.raises(cluster_ref.GridOverflow):
        filter_ref.filter(filter_cases.cluster_cases.beyond_the_grid(), None, mean_k=0, radius=filter_cases.R, min_neighbors=1)


def test_binding_structs_match_the_header():
    """the ctypes structs of the binding have the sizes the C compiler gives the header's"""
    import os
    import subprocess
    import tempfile

    sicp = importlib.import_module("semantic-icp_amd")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = '#include <stdio.h>\n#include <stddef.h>\n#include "sicp.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", ' \
           "sizeof(sicp_filter_params), sizeof(sicp_filter_info), offsetof(sicp_filter_params, drop), offsetof(sicp_filter_info, mean)); return 0; }\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(code)
        subprocess.run(["gcc", "-I", os.path.join(root, "include"), src, "-o", exe], check=True)
        sizes = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    assert sizes == [sicp.C.sizeof(sicp.SicpFilterParams), sicp.C.sizeof(sicp.SicpFilterInfo), sicp.SicpFilterParams.drop.offset,
                     sicp.SicpFilterInfo.mean.offset]
    p = sicp.default_filter_params(drop=(3, 4), protect=(1,), radius=0.5)
    assert (p.mean_k, p.std_mul, p.radius, p.min_neighbors, p.n_drop, p.n_protect) == (20, 2.0, 0.5, 2, 2, 1)
    assert list(p.drop[:2]) == [3, 4] and p.protect[0] == 1
