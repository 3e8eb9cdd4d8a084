"""cov_body and cov9_caller_order_kernel (csrc/feature_kernels.hip) and sicp_covariances' two getter paths against a
restatement that shares nothing with the Jacobi code (tests/cov_ref.py), at every k, list layout, flag and degenerate
shape (cases and bar: tests/cov_cases.py, checked without a GPU by tests/test_cov_cases_cpu.py):

 1. every k = 1..32 under every nn_method (method 1 writes the lists rank-major), flag 1; flag 0 at the batch edges;
 2. the |eigenvalue| rule and degenerate spectra: lidar + 300 m, planar grids, a line, repeated points, one position;
 3. scale x 1e-3 and x 1e3; 4. clouds of n = k = 20 points, where the eigen-solve has no slack;
 5. short lists (n < k); 6. n around the workgroup; 7. SEMANTIC segments of 1 .. 400 points; 8. dropped points;
 then both getter paths in every state, recomputation after k_cov, the flag or the cloud change, a cloud shared by handles
 that differ in all three, and the jobs of one align_batch launch against lone engines.

Every case checks EVERY row: the lists are the oracle's k-NN; the normal is finite, of unit length within 540 u and an
eigenvector of smallest |eigenvalue| of the restated moment matrix within GAMMA u S; the matrix is I - (1 - eps) n n^T of
the returned normal bit for bit.  Each prints its figures (profiles/covariances/figures.txt)."""
import functools
import importlib

import numpy as np
import pytest

import cov_cases as CC
import cov_ref as ref
import oracle_lib as O

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
S_, T_ = sicp.SOURCE, sicp.TARGET
METHODS = pytest.mark.parametrize("method", [0, 1, 2], ids=["bruteforce", "boxtree", "boxtree_per_query"])
FIG = {}      # family -> [gpu ratio, oracle ratio, unit, rows with the oracle's bits, rows]


def params(k, method, flag, mode=sicp.MODE_GICP, **kw):
    p = sicp.default_params(mode)
    p.k_cov, p.nn_method, p.quirk_float_products = k, method, flag
    for name, v in kw.items():
        setattr(p, name, v)
    return p


def engine(k, method, flag, mode=sicp.MODE_GICP, **kw):
    return sicp.Engine(0, params(k, method, flag, mode, **kw))


def read(e, which=S_):
    cov, nrm, _, nn = e.covariances(which, want_nn=True)
    return cov, nrm, nn


def note(family, f, of):
    a = FIG.setdefault(family, [0.0, 0.0, 0.0, 0, 0])
    a[0], a[1], a[2] = max(a[0], f["ratio"]), max(a[1], of["ratio"] if of else 0.0), max(a[2], f["unit"])
    a[3] += f["same"] or 0
    a[4] += f["rows"]


def check(family, p, k, flag, got, want_nn, onrm, what, eps=CC.EPS):
    """every check of the module's docstring on one read (cov, nrm, nn) of the cloud p"""
    cov, nrm, nn = got
    assert nn.shape == want_nn.shape and np.array_equal(nn, want_nn), (what, "lists")
    f = CC.assert_normals(p, nn, k, flag, nrm, what, onrm)
    CC.assert_matrices(cov, nrm, eps, what)
    note(family, f, CC.figures(p, nn, k, flag, onrm) if onrm is not None else None)
    return f


def run_case(c, method, e=None):
    p = CC.cloud(c.cloud)
    own = e is None
    e = engine(c.k, method, c.flag) if own else e
    try:
        e.set_source(p)
        got = read(e)
        alone = e.covariance_matrices(S_)
    finally:
        if own:
            e.close()
    what = f"{CC.case_id(c)} method {method}"
    f = check(c.family, p, c.k, c.flag, got, CC.oracle_lists(c.cloud, c.k), CC.oracle_normals(c.cloud, c.k, c.flag), what)
    assert alone.tobytes() == got[0].tobytes(), (what, "cov9 alone")
    return got, f


def cases_of(family):
    return pytest.mark.parametrize("c", [c for c in CC.cases() if c.family == family], ids=CC.case_id)


# ---- 1 .. 6: one cloud, one handle ------------------------------------------------------------------------------------------------------
@METHODS
@cases_of("every_k")
def test_every_k(c, method):
    (cov, nrm, nn), _ = run_case(c, method)
    assert nn.shape == (3000, c.k) and (nn >= 0).all()


@METHODS
@cases_of("rule")
def test_the_eigenvalue_rule_and_degenerate_spectra(c, method):
    (cov, nrm, nn), f = run_case(c, method)
    if c.cloud in ("grid", "coincident"):
        # exact products: the matrix's z row is exactly zero, the tie rule alone decides: e_z, the later column
        assert np.array_equal(np.abs(nrm), np.tile([0.0, 0.0, 1.0], (len(nrm), 1))), CC.case_id(c)
        assert np.array_equal(np.abs(nrm), np.abs(CC.oracle_normals(c.cloud, c.k)))
    if c.cloud == "coincident":
        assert np.array_equal(nn, np.tile(np.arange(c.k, dtype=np.int32), (len(nn), 1)))   # the lowest indices, ascending
        ocov = O.covariances(CC.cloud(c.cloud), None, c.k, CC.EPS, 0)[0]
        assert np.allclose(cov, ocov, atol=1e-12)


@METHODS
@cases_of("scale")
def test_scale(c, method):
    run_case(c, method)


@METHODS
@pytest.mark.parametrize("flag", [1, 0])
def test_the_eigen_solve_at_full_precision(flag, method):
    """n = k = 20 about the origin: every neighbourhood is the whole cloud, S ~ |A|; the clouds one after another on one handle"""
    with engine(20, method, flag) as e:
        for c in CC.cases():
            if c.family == "full" and c.flag == flag:
                (cov, nrm, nn), _ = run_case(c, method, e)
                assert (np.sort(nn, axis=1) == np.arange(20)).all()


@METHODS
@cases_of("short")
def test_short_lists_divide_by_k(c, method):
    """the -1 tail is there, the divisor is k (the restatement divides by k), every output is finite"""
    (cov, nrm, nn), _ = run_case(c, method)
    n = len(nrm)
    assert n < c.k and (nn[:, n:] == -1).all() and (np.sort(nn[:, :n], axis=1) == np.arange(n)).all()
    assert np.isfinite(cov).all() and np.isfinite(nrm).all()


@METHODS
@cases_of("edge")
def test_workgroup_edge(c, method):
    run_case(c, method)


# ---- 7: SEMANTIC segments ---------------------------------------------------------------------------------------------------------------
@METHODS
@pytest.mark.parametrize("k", CC.SEMANTIC_K)
def test_semantic_segments(k, method):
    """every neighbourhood stays inside its class, and each class equals the reference on that class alone"""
    p, lab = CC.cloud("semantic"), CC.semantic_labels()
    with engine(k, method, 1, sicp.MODE_SEMANTIC, num_classes=len(CC.SEMANTIC_SIZES)) as e:
        e.set_source(p, lab)
        cov, nrm, nn = read(e)
        alone = e.covariance_matrices(S_)
    assert alone.tobytes() == cov.tobytes()
    for label, rows in CC.semantic_classes():
        sub = np.ascontiguousarray(p[rows])
        local = CC.local_lists(rows, nn[rows], len(p))
        onn = O.knn(sub, sub, k, kdtree=True)[0]
        onrm = O.covariances(sub, None, k, CC.EPS, 0, kdtree=True)[1]
        assert (local[:, len(rows):] == -1).all()
        check("semantic", sub, k, 1, (cov[rows], nrm[rows], local), onn, onrm, f"semantic class {label} n {len(rows)} k {k} method {method}")


# ---- 8: dropped points ------------------------------------------------------------------------------------------------------------------
@METHODS
def test_dropped_points(method):
    p, keep = CC.cloud("dropped"), CC.kept_rows()
    fin = np.zeros(len(p), dtype=bool)
    fin[keep] = True
    with engine(20, method, 1) as e:
        e.set_source(p)
        assert e.cloud_size(S_) == (len(p), len(keep))
        cov, nrm, nn = read(e)
        alone = e.covariance_matrices(S_)          # a cloud with dropped points goes through the host loop: the NaN rows are there
    assert np.isnan(cov[~fin]).all() and np.isnan(nrm[~fin]).all() and (nn[~fin] == -1).all()
    assert np.isnan(alone[~fin]).all() and alone[fin].tobytes() == cov[fin].tobytes()
    sub = np.ascontiguousarray(p[keep])
    onn = O.knn(sub, sub, 20, kdtree=True)[0]
    assert np.array_equal(nn[fin], keep[onn])                          # caller indices, none of a dropped point
    onrm = O.covariances(sub, None, 20, CC.EPS, 0, kdtree=True)[1]
    check("dropped", sub, 20, 1, (cov[fin], nrm[fin], CC.local_lists(keep, nn[fin], len(p))), onn, onrm, f"dropped method {method}")


# ---- both getter paths ------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


@pytest.mark.parametrize("which", [S_, T_], ids=["source", "target"])
@pytest.mark.parametrize("n", [257, 3000])
@pytest.mark.parametrize("eps", [1e-3, 0.25])
def test_both_getter_paths_return_the_same_bytes(n, which, eps):
    """sicp_covariances(h, which, cov9, NULL, NULL, NULL) forms the matrices on the device; the full call on the host"""
    p = CC.cloud("lidar+35")[:n]
    rng = np.random.default_rng(n)
    with engine(20, 1, 1, epsilon=eps) as e:
        e.set_cloud(which, p)
        # the engine's own normals
        cov, nrm, nn = read(e, which)
        assert e.covariance_matrices(which).tobytes() == cov.tobytes()
        CC.assert_matrices(cov, nrm, eps, "own normals")
        assert np.abs(cov - (np.eye(3) - (1 - eps) * nrm[:, :, None] * nrm[:, None, :])).max() < 1e-15
        # set_covariances of normal-form matrices: the normals are taken out of them, the matrices formed anew
        given = _unit(rng, n)
        e.set_covariances(which, ref.matrix_of_normal(given, eps))
        cov, nrm, _, _ = e.covariances(which)
        assert e.covariance_matrices(which).tobytes() == cov.tobytes()
        CC.assert_matrices(cov, nrm, eps, "normal form")
        assert np.abs(np.abs(np.einsum("na,na->n", nrm, given)) - 1).max() < 1e-12 and ref.unit_error(nrm).max() <= 8 * ref.U
        # set_covariances of general matrices (GICP): what is there is what comes back, and no normal belongs to it
        B = rng.normal(size=(n, 3, 3))
        general = B @ B.transpose(0, 2, 1) + 0.1 * np.eye(3)
        general = 0.5 * (general + general.transpose(0, 2, 1))
        e.set_covariances(which, general)
        cov, nrm, _, _ = e.covariances(which)
        assert np.array_equal(cov, general) and np.isnan(nrm).all()
        assert e.covariance_matrices(which).tobytes() == cov.tobytes()
        # and the engine's own again once the cloud is set anew
        e.set_cloud(which, p)
        assert e.covariance_matrices(which).tobytes() == lone("lidar+35", n, 20, 1, 1, eps)[0]


# ---- staleness --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lone(name, n, k, method, flag, eps=CC.EPS):
    """the bytes (cov, nrm, nn) a fresh engine returns for the first n points of that cloud"""
    with engine(k, method, flag, epsilon=eps) as e:
        e.set_source(CC.cloud(name)[:n])
        return tuple(a.tobytes() for a in read(e))


def bytes_of(e, which=S_):
    return tuple(a.tobytes() for a in read(e, which))


@METHODS
def test_features_are_recomputed_when_k_the_flag_or_the_cloud_change(method):
    with engine(20, method, 1) as e:
        held = None
        for k, flag, name in ((20, 1, "lidar+35"), (5, 1, "lidar+35"), (20, 1, "lidar+35"), (20, 0, "lidar+35"), (20, 1, "lidar+35"),
                              (20, 1, "lidar+300"), (7, 0, "lidar+300"), (7, 0, "lidar+35")):
            e.set_params(params(k, method, flag))
            if name != held:
                e.set_source(CC.cloud(name))
                held = name
            assert bytes_of(e) == lone(name, 3000, k, method, flag), (k, flag, name)
            assert e.covariance_matrices(S_).tobytes() == lone(name, 3000, k, method, flag)[0]
    assert lone("lidar+35", 3000, 20, method, 1) != lone("lidar+35", 3000, 20, method, 0)      # the flag changes the bytes
    assert lone("lidar+35", 3000, 20, method, 1)[1] != lone("lidar+300", 3000, 20, method, 1)[1]


def test_a_cloud_shared_by_handles_of_different_k_method_and_flag():
    """the cloud carries feat_k, feat_float_products and nn_stride: each handle's read is its lone bytes, in any order"""
    setups = ((20, 1, 1), (5, 0, 0), (32, 2, 1), (9, 1, 0))
    n = 2000
    es = [engine(*s) for s in setups]
    try:
        es[0].set_source(CC.cloud("lidar+35")[:n])
        es[0].set_target(CC.cloud("lidar+300")[:n])
        for e in es[1:]:
            e.share_cloud(S_, es[0], S_)
        es[1].share_cloud(T_, es[0], S_)            # the same cloud in both slots of one handle
        es[2].set_target(CC.cloud("lidar+300")[:n])
        for i in (0, 1, 2, 3, 1, 0, 3, 2, 2, 0):
            k, m, f = setups[i]
            assert bytes_of(es[i]) == lone("lidar+35", n, k, m, f), setups[i]
            assert es[i].covariance_matrices(S_).tobytes() == lone("lidar+35", n, k, m, f)[0], setups[i]
        assert bytes_of(es[1], T_) == lone("lidar+35", n, 5, 0, 0)
        assert bytes_of(es[0], T_) == lone("lidar+300", n, 20, 1, 1) == bytes_of(es[0], T_)
        assert bytes_of(es[2], T_) == lone("lidar+300", n, 32, 2, 1)
    finally:
        for e in es:
            e.close()


@METHODS
def test_the_jobs_of_one_batch_launch_equal_lone_engines(method):
    """align_batch computes the features of all its clouds in one launch whose grid is sized for the largest: the smaller
    jobs' rows, and each job's own flag, are those of lone engines"""
    sizes, flags = (40, 255, 257, 1000), (1, 0, 0, 1)
    es = [engine(20, method, f, max_outer=1, max_lm_iterations=2) for f in flags]
    try:
        for e, n in zip(es, sizes):
            e.set_source(CC.cloud("lidar+35")[:n])
            e.set_target(CC.cloud("lidar+35")[3000 - n:])
        sicp.align_batch(es)
        for e, n, f in zip(es, sizes, flags):
            assert bytes_of(e, S_) == lone("lidar+35", n, 20, method, f), (n, f)
            want = lone_tail(n, method, f)
            assert bytes_of(e, T_) == want, (n, f)
            assert e.covariance_matrices(T_).tobytes() == want[0]
    finally:
        for e in es:
            e.close()


@functools.lru_cache(maxsize=None)
def lone_tail(n, method, flag):
    with engine(20, method, flag) as e:
        e.set_source(CC.cloud("lidar+35")[3000 - n:])
        return tuple(a.tobytes() for a in read(e))


# ---- the figures ------------------------------------------------------------------------------------------------------------------------
def test_zz_figures():
    """(runs last) per case family: the GPU's and the oracle's largest ratio, the largest | |n| - 1 | and the rows whose
    normal has the oracle's bits up to sign -- reported, not asserted"""
    print(f"covariances: GAMMA {CC.GAMMA:.3f}  unit bound {ref.UNIT_BOUND:.3e}")
    for family, (g, o, u, same, rows) in FIG.items():
        print(f"covariances: family {family:9s} rows {rows:7d}  gpu ratio {g:.3f}  oracle ratio {o:.3f}  | |n| - 1 | {u:.2e}  oracle's bits {same}")
        assert g <= CC.GAMMA and u <= ref.UNIT_BOUND
