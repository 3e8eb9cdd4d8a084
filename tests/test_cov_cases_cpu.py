"""CPU tests of what tests/test_gpu_covariances.py stands on (tests/cov_cases.py, tests/cov_ref.py): the restatement agrees
with np_ref.covariance_from_neighbors on the golden cloud; the oracle's normals pass every check on every case; GAMMA is
four times the oracle's largest ratio; a reference that picks the signed-smallest eigenvector fails at the stated share of
points of each rule case; and the clouds have the properties their families are named for."""
import os

import numpy as np
import pytest

import cov_cases as CC
import cov_ref as ref
import np_ref
import oracle_lib as O

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = CC.cases()


def test_longdouble_is_wider_than_float64():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_restatement_agrees_with_np_ref_on_the_golden_cloud():
    g = np.load(os.path.join(G, "cov.npz"))
    p, nn = g["p"], g["nn"]
    k = nn.shape[1]
    A, S = ref.moments(p, nn, k, 1)
    rows = np.arange(0, len(p), max(1, len(p) // 300))
    worst = 0.0
    for i in rows:
        _, normal, s, cov = np_ref.covariance_from_neighbors(p, nn[i], k, CC.EPS)
        # float64 sums of the same float32 products: within the cancellation's uncertainty u S (a few of it: k terms)
        assert np.abs(cov - A[i]).max() <= 4 * k * ref.U * S[i]
        worst = max(worst, np.abs(cov - A[i]).max() / (ref.U * S[i]))
        # LAPACK's last singular vector is an eigenvector of smallest |eigenvalue| of A to the same precision
        assert ref.ratio(A[i:i + 1], S[i:i + 1], normal[None])[0] <= 4 * k
    print(f"golden cloud: |A_np_ref - A| <= {worst:.2f} u S over {len(rows)} rows")
    # the golden normals pass the check itself, every row
    r = ref.ratio(A, S, g["normals"])
    print(f"golden cloud: largest ratio of the golden normals {r.max():.3f}")
    assert r.max() <= 4 * k
    # and the matrix of a normal is the golden matrix (computed as the sum of outer products) to rounding
    assert np.allclose(ref.matrix_of_normal(g["normals"], CC.EPS), g["cov"], atol=1e-14, rtol=0)


def test_ratio_sees_what_it_must():
    """on one cloud: a dropped neighbour, the live count as the divisor, a product of the other width, and a rotation of the
    normal by 1e-9 all land far above any GAMMA; the flag-0 matrices differ from the flag-1 ones"""
    p, k = CC.cloud("lidar+35"), 20
    nn = CC.oracle_lists("lidar+35", k)
    A, S = CC.reference("lidar+35", k, 1)
    n = CC.oracle_normals("lidar+35", k)
    cut = nn.copy()
    cut[:, -1] = -1
    A0, _ = ref.moments(p, nn, k, 0)
    Acnt, _ = ref.moments(p, cut, k - 1, 1)            # 19 neighbours divided by 19: what a kernel dividing by the live count sees
    for what, B in (("dropped neighbour", ref.moments(p, cut, k, 1)[0]), ("other width", A0), ("live count", Acnt)):
        r = ref.ratio(A[:200], S[:200], CC.jacobi_normals(B[:200]))
        print(f"{what}: median ratio {np.median(r):.3g}, share above 1000: {np.mean(r > 1000):.3f}")
        assert np.median(r) > 1000, what
    t = np.cross(n, np.roll(n, 1, axis=1))
    t /= np.linalg.norm(t, axis=1)[:, None]
    turned = n + 1e-9 * t
    turned /= np.linalg.norm(turned, axis=1)[:, None]
    assert np.median(ref.ratio(A, S, turned)) > 100


@pytest.fixture(scope="module")
def oracle_figures():
    """{case: figures} of the oracle's normals on every case, the semantic classes and the kept rows of `dropped` included"""
    out = {}
    for c in CASES:
        out[CC.case_id(c)] = (c.family, CC.figures(CC.cloud(c.cloud), CC.oracle_lists(c.cloud, c.k), c.k, c.flag,
                                                   CC.oracle_normals(c.cloud, c.k, c.flag)))
    p = CC.cloud("semantic")
    for k in CC.SEMANTIC_K:
        for label, rows in CC.semantic_classes():
            sub = np.ascontiguousarray(p[rows])
            nn = O.knn(sub, sub, k, kdtree=True)[0]
            nrm = O.covariances(sub, None, k, CC.EPS, 0, kdtree=True)[1]
            out[f"semantic-class{label}-n{len(rows)}-k{k}"] = ("semantic", CC.figures(sub, nn, k, 1, nrm))
    sub = np.ascontiguousarray(CC.cloud("dropped")[CC.kept_rows()])
    nn = O.knn(sub, sub, 20, kdtree=True)[0]
    out["dropped-k20"] = ("dropped", CC.figures(sub, nn, 20, 1, O.covariances(sub, None, 20, CC.EPS, 0, kdtree=True)[1]))
    return out


def test_the_oracles_normals_pass_every_check_on_every_case(oracle_figures):
    fam = {}
    for name, (family, f) in oracle_figures.items():
        assert f["unit"] <= ref.UNIT_BOUND, name
        assert f["ratio"] <= CC.GAMMA, (name, f["ratio"])
        a = fam.setdefault(family, [0.0, 0.0, 0])
        a[0], a[1], a[2] = max(a[0], f["ratio"]), max(a[1], f["unit"]), a[2] + f["rows"]
    for family, (r, u, rows) in fam.items():
        print(f"oracle: {family:9s} rows {rows:7d}  largest ratio {r:.3f}  largest | |n| - 1 | {u:.2e}")


def test_gamma_is_four_times_the_oracles_largest_ratio(oracle_figures):
    worst = max(oracle_figures, key=lambda name: oracle_figures[name][1]["ratio"])
    top = oracle_figures[worst][1]["ratio"]
    print(f"the oracle's largest ratio: {top:.4f} at {worst}; GAMMA = {CC.GAMMA}")
    assert abs(CC.ORACLE_MAX_RATIO - top) <= 0.005 * top
    assert CC.GAMMA == 4.0 * CC.ORACLE_MAX_RATIO


@pytest.mark.parametrize("name,k", sorted(CC.BITES), ids=lambda v: str(v))
def test_the_rule_cases_bite(name, k):
    """the eigenvector of the smallest SIGNED eigenvalue fails ratio <= BITE_THRESHOLD at no less than the stated share of
    points: on these inputs a column choice without |.| cannot pass"""
    A, S = CC.reference(name, k, 1)
    share = float(np.mean(ref.ratio(A, S, ref.signed_smallest_normal(A)) > CC.BITE_THRESHOLD))
    print(f"{name} k={k}: signed-smallest fails at {share:.3f} of {len(A)} points (floor {CC.BITES[(name, k)]})")
    assert share >= CC.BITES[(name, k)]
    above = float(np.mean(ref.ratio(A, S, ref.signed_smallest_normal(A)) > CC.GAMMA))
    assert above >= 0.9 * CC.BITES[(name, k)], (above, "the bite must survive the bar itself")


def test_exact_clouds_have_exact_matrices():
    """the axis-aligned grid and the coincident cloud have exactly representable products: A's z row is exactly zero (grid)
    or A is exactly zero (coincident), so the column choice is decided by the tie rule alone: e_z, the later column"""
    for k in CC.RULE_K:
        A, _ = CC.reference("coincident", k, 1)
        assert not A.any()
        n = CC.oracle_normals("coincident", k)
        assert np.array_equal(np.abs(n), np.tile([0.0, 0.0, 1.0], (len(n), 1)))
        A, _ = CC.reference("grid", k, 1)
        assert not A[:, 2, :].any() and not A[:, :, 2].any()
        n = CC.oracle_normals("grid", k)
        assert np.array_equal(np.abs(n), np.tile([0.0, 0.0, 1.0], (len(n), 1)))
    A, _ = CC.reference("grid", 3, 1)
    w = np.linalg.eigvalsh(A)
    assert np.mean(w[:, 1] == 0) >= 0.02    # k = 3 on a lattice: some triples are collinear: two zero eigenvalues, the tie goes to e_z


def test_full_clouds_leave_no_slack_and_lidar_clouds_do():
    for c in CASES:
        A, S = CC.reference(c.cloud, c.k, c.flag)
        with np.errstate(divide="ignore", invalid="ignore"):
            slack = S / np.abs(np.linalg.eigvalsh(A)).max(axis=1)
        if c.family == "full":
            assert len(A) == c.k == 20 and slack.max() < 4, CC.case_id(c)
        if c.family == "every_k" and c.k >= 5:
            assert np.median(slack) > 100


def test_lists_of_short_and_tied_clouds():
    for n, k in CC.SHORT:
        nn = CC.oracle_lists(f"first/{n}", k)
        assert (nn[:, n:] == -1).all() and (np.sort(nn[:, :n], axis=1) == np.arange(n)).all()
    # kd-tree and brute force (order: distance, lower caller index) give the same lists on the clouds full of ties
    for name in ("grid", "dup7", "coincident"):
        p = CC.cloud(name)
        for k in CC.RULE_K:
            assert np.array_equal(CC.oracle_lists(name, k), O.knn(p, p, k, kdtree=False)[0]), (name, k)


def test_semantic_and_dropped_inputs():
    lab = CC.semantic_labels()
    assert np.array_equal(np.bincount(lab)[1:], CC.SEMANTIC_SIZES) and len(lab) == len(CC.cloud("semantic"))
    for k in CC.SEMANTIC_K:
        assert {1, 2, k - 1, k, k + 1} <= set(CC.SEMANTIC_SIZES)
    assert (np.diff(lab.astype(int)) != 0).mean() > 0.5                 # scattered, not sorted by class
    p = CC.cloud("dropped")
    assert len(CC.kept_rows()) == len(p) - CC.N_DROPPED
    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
