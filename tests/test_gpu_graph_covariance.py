"""GPU tests of sicp_graph_marginals / sicp_graph_relative_covariances through the C ABI: the blocks against sparse LU solves
(tests/graph_cov_ref.py) under the a-priori bound of the stopping rule, the independence of a query's bytes from its company,
the graph left as it was, the per-query statuses, the refusals, the memory limit, and one loop closure gated end to end.

Accuracy.  Per query the gap is max |got - ref| / max |ref|.  A column stops at |r| <= tolerance |b|, so an entry of J X is off by
at most |J|_2 tolerance max_row|J| / lambda_min(H) (graph_cov_ref.bound): a condition on the solver, not a measurement.  The
float64 restatement of the same method sits at 1e-6 to 1e-3 of it on these cases; the test prints the kernels' gap beside the
restatement's."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import graph_cov_ref as V
import pose_graph_cases as cases
import pose_graph_ref as R

sicp = importlib.import_module("semantic-icp_amd")
pytestmark = pytest.mark.gpu
TOLERANCE = 1e-10
CHI2_6_99 = 16.811893829770927  # the 99 % quantile of chi-square with 6 degrees of freedom


def build(g, params=None):
    pg = sicp.PoseGraph(0, params)
    assert pg.add_nodes(g["poses"], g["fixed"]) == 0
    if len(g["ei"]):
        assert pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"]) == 0
    return pg


def ask(pg, qa, qb, **kw):
    """relative covariances where qa >= 0, marginals where qa < 0, in the order asked"""
    qa, qb = np.asarray(qa, dtype=np.int32), np.asarray(qb, dtype=np.int32)
    p = sicp.default_graph_cov_params(**kw) if kw else None
    cov, st = np.empty((len(qb), 6, 6)), np.empty(len(qb), dtype=np.int32)
    infos = []
    for mask, call in ((qa >= 0, lambda m: pg.relative_covariances(qa[m], qb[m], p)), (qa < 0, lambda m: pg.marginals(qb[m], p))):
        if mask.any():
            cov[mask], st[mask], info = call(mask)
            infos.append(info)
    return cov, st, infos


@functools.lru_cache(maxsize=None)
def solved(name):
    g, kind, a, qa, qb = V.case(name)
    ref, st, H = V.reference(g, qa, qb, kind, a)
    rest, _, longest = V.restated(g, qa, qb, kind, a, TOLERANCE)
    for arr in (ref, st, rest):
        arr.setflags(write=False)
    return g, kind, a, qa, qb, ref, st, V.lambda_min(H), rest, longest


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_blocks_against_sparse_lu(name):
    g, kind, a, qa, qb, ref, st_ref, lam, rest, longest = solved(name)
    with build(g, sicp.default_graph_params(loss=kind, cauchy_a=a)) as pg:
        before = pg.poses().tobytes()
        got, st, (info,) = ask(pg, qa, qb)
        marg, mst, _ = ask(pg, -np.ones(len(qb), dtype=np.int32), qb)
        assert pg.poses().tobytes() == before
    assert np.array_equal(st, st_ref)
    assert info["n_ok"] == int((st == V.OK).sum()) and info["n_failed"] == int((st != V.OK).sum())
    assert info["worst_relative_residual"] <= TOLERANCE * (1 + 1e-12)  # (the device tests sqrt(rr) <= tolerance sqrt(bb), this is the quotient)
    J = V.jacobian(g, qa, qb)
    worst, worst_rest, worst_abs = 0.0, 0.0, 0.0
    for q in range(len(qb)):
        if st_ref[q] != V.OK:
            assert np.isnan(got[q]).all()
            continue
        assert np.array_equal(got[q], got[q].T)
        scale = np.abs(ref[q]).max()
        if scale == 0.0:
            assert not got[q].any()
            continue
        gap, limit = np.abs(got[q] - ref[q]).max() / scale, V.bound(J[q], TOLERANCE, lam) / scale
        worst, worst_abs = max(worst, gap / limit), max(worst_abs, gap * scale)
        worst_rest = max(worst_rest, np.abs(rest[q] - ref[q]).max() / scale / limit)
        assert gap <= limit, (q, gap, limit)
    # the marginals of the same nodes: against the reference's, and zeros at the fixed node
    mref, mst_ref, _ = V.reference(g, -np.ones(len(qb), dtype=np.int32), qb, kind, a)
    assert np.array_equal(mst, mst_ref)
    Jm = V.jacobian(g, -np.ones(len(qb), dtype=np.int32), qb)
    for q in range(len(qb)):
        if mst_ref[q] != V.OK:
            assert np.isnan(marg[q]).all()
        elif g["fixed"][qb[q]]:
            assert not marg[q].any() and not np.signbit(marg[q]).any()
        else:
            scale = np.abs(mref[q]).max()
            assert np.abs(marg[q] - mref[q]).max() <= V.bound(Jm[q], TOLERANCE, lam)
            assert np.linalg.eigvalsh(marg[q])[0] > 0
    print(f"graph_cov {name}: nodes {len(g['poses'])} lambda_min {lam:.3e} iterations {info['cg_iterations']} (restatement {longest}) "
          f"passes {info['passes']} worst gap/bound: kernels {worst:.3e} restatement {worst_rest:.3e}; worst absolute gap {worst_abs:.3e}")


# ---- rule 7: a query's bytes do not depend on its company ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring65_8_closures", "hub300"])
def test_a_querys_bytes_do_not_depend_on_its_company(name):
    g, kind, a, _, _ = V.case(name)
    qa, qb = V.queries(g, seed=7, pairs=7)
    with build(g) as pg, build(g) as twin:
        together, st, (info,) = ask(pg, qa, qb)
        assert not st.any() and info["passes"] == 2  # (8 queries at 24 columns)
        for q in range(8):
            alone, s1, _ = ask(pg, qa[q:q + 1], qb[q:q + 1])
            assert alone.tobytes() == together[q].tobytes() and s1[0] == st[q]
        back, sb, _ = ask(pg, qa[::-1], qb[::-1])
        assert back[::-1].tobytes() == together.tobytes() and np.array_equal(sb[::-1], st)
        for cols, passes in ((6, 8), (12, 4), (48, 1)):
            c, s, (i,) = ask(pg, qa, qb, max_columns=cols)
            assert c.tobytes() == together.tobytes() and np.array_equal(s, st) and i["passes"] == passes
        # check_every changes when the host looks, not what the device does
        c, s, _ = ask(pg, qa, qb, check_every=1)
        assert c.tobytes() == together.tobytes()
        # two graphs driven alike
        c, s, (i,) = ask(twin, qa, qb)
        assert c.tobytes() == together.tobytes() and np.array_equal(s, st) and i == info


# ---- rule 1: the graph is left as it was ----------------------------------------------------------------------------------------
def test_the_call_leaves_the_graph_and_a_later_optimize_unchanged():
    g = cases.ring(closures=8)
    qa, qb = V.queries(g, seed=3)
    p = sicp.default_graph_params(gradient_tolerance=1e-7, function_tolerance=0.0, parameter_tolerance=0.0)
    with build(g, p) as pg, build(g, p) as twin:
        before = pg.poses().tobytes()
        ask(pg, qa, qb)
        ask(pg, -np.ones(3, dtype=np.int32), [1, 2, 3], max_columns=6)
        assert pg.poses().tobytes() == before
        a, b = pg.optimize(), twin.optimize()
        assert a == b and a["accepted_steps"] >= 1
        assert pg.poses().tobytes() == twin.poses().tobytes()
        # and after the optimisation: the same answer on both, the one that asked before and the one that did not
        c1, s1, _ = ask(pg, qa, qb)
        c2, s2, _ = ask(twin, qa, qb)
        assert c1.tobytes() == c2.tobytes() and np.array_equal(s1, s2)
        assert pg.optimize() == twin.optimize() and pg.poses().tobytes() == twin.poses().tobytes()


# ---- statuses -------------------------------------------------------------------------------------------------------------------
def test_the_iteration_limit_gives_not_converged_with_the_last_iterate():
    g = cases.ring(closures=8)
    qa, qb = V.queries(g, seed=3)
    with build(g) as pg:
        cov, st, (info,) = ask(pg, qa, qb, max_cg_iterations=3)
        full, _, _ = ask(pg, qa, qb)
    assert np.all(st == sicp.GRAPH_COV_NOT_CONVERGED) and np.isfinite(cov).all()
    # (5 queries at 24 columns: two passes of three iterations each)
    assert info == dict(info, passes=2, cg_iterations=6, n_ok=0, n_failed=len(qb)) and info["worst_relative_residual"] > TOLERANCE
    rest, rst, _ = V.restated(g, qa, qb, tolerance=TOLERANCE, max_iterations=3)
    assert np.all(rst == V.NOT_CONVERGED)
    # three steps of the same recurrence in another summation order: rounding level, relative to the converged block
    assert np.abs(cov - rest).max() <= 1e-9 * np.abs(full).max()


def test_a_graph_without_a_fixed_node_answers_unanchored():
    g = cases.ring(closures=2)
    g["fixed"][:] = False
    with build(g) as pg:
        cov, st, infos = ask(pg, [1, 5, -1], [2, 9, 4])
        assert np.all(st == sicp.GRAPH_COV_UNANCHORED) and np.isnan(cov).all()
        assert infos == [dict(passes=0, cg_iterations=0, n_ok=0, n_failed=k, worst_relative_residual=0.0) for k in (2, 1)]


def test_statuses_split_by_component():
    """a ring with node 0 fixed and a chain without a fixed node, side by side in one graph"""
    a, b = cases.ring(n=12, closures=2, seed=21), cases.chain(6, seed=22, fixed_at=2, isolated=0)
    b["fixed"][:] = False
    n = len(a["poses"])
    g = dict(poses=np.concatenate([a["poses"], b["poses"]]), fixed=np.concatenate([a["fixed"], b["fixed"]]),
             ei=np.concatenate([a["ei"], b["ei"] + n]).astype(np.int32), ej=np.concatenate([a["ej"], b["ej"] + n]).astype(np.int32),
             z=np.concatenate([a["z"], b["z"]]), omega=np.concatenate([a["omega"], b["omega"]]))
    qa = np.array([1, 3, n + 1, 4, 0], dtype=np.int32)
    qb = np.array([7, n + 2, n + 4, 0, n + 3], dtype=np.int32)
    want = np.array([0, 2, 2, 0, 2], dtype=np.int32)
    ref, st_ref, H = V.reference(g, qa, qb)
    assert np.array_equal(st_ref, want)
    with build(g) as pg:
        cov, st, (info,) = ask(pg, qa, qb)
        marg, mst, _ = ask(pg, -np.ones(2, dtype=np.int32), [n + 1, 5])
    assert np.array_equal(st, want) and np.array_equal(mst, [2, 0])
    assert (info["n_ok"], info["n_failed"]) == (2, 3)
    keep = np.repeat(V.anchored(g), 6)
    lam = V.lambda_min(H[keep][:, keep])
    J = V.jacobian(g, qa, qb)
    for q in np.flatnonzero(want == 0):
        assert np.abs(cov[q] - ref[q]).max() <= V.bound(J[q], TOLERANCE, lam)
    assert np.isnan(cov[want == 2]).all() and np.isnan(marg[0]).all() and np.isfinite(marg[1]).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_and_leave_the_graph_alone():
    L = sicp.lib()
    g = cases.ring(n=12, closures=2, seed=21)
    ip, dp = sicp._ip, sicp._dp
    ptr = sicp._ptr
    with build(g) as pg, build(g) as twin:
        G = pg._g
        before = pg.poses().tobytes()
        a, b = np.array([1, 2], np.int32), np.array([5, 7], np.int32)
        cov, st = np.full((2, 6, 6), 7.0), np.full(2, 7, np.int32)
        info = sicp.SicpGraphCovInfo(passes=7)

        def refused(status, *words):
            assert status == sicp.ERR_INVALID_ARGUMENT
            text = L.sicp_graph_last_error(G).decode()
            assert all(w in text for w in words) and text.endswith("nothing was written"), text
            assert np.all(cov == 7.0) and np.all(st == 7) and info.passes == 7
            assert pg.poses().tobytes() == before

        def rel(p=None, n=2, aa=a, bb=b, out=cov):
            return L.sicp_graph_relative_covariances(G, None if p is None else C.byref(p), n, ptr(aa, ip), ptr(bb, ip), ptr(out, dp),
                                                     ptr(st, ip), C.byref(info))

        def marg(p=None, n=2, bb=b, out=cov):
            return L.sicp_graph_marginals(G, None if p is None else C.byref(p), n, ptr(bb, ip), ptr(out, dp), ptr(st, ip), C.byref(info))

        refused(rel(aa=None), "relative_covariances", "NULL")
        refused(rel(bb=None), "NULL")
        refused(rel(out=None), "NULL")
        refused(marg(bb=None), "sicp_graph_marginals", "NULL")
        refused(marg(out=None), "NULL")
        refused(rel(n=0), "n must be >= 1")
        refused(marg(n=-1), "n must be >= 1")
        refused(rel(bb=np.array([5, 12], np.int32)), "query 1", "outside")
        refused(rel(aa=np.array([-1, 2], np.int32)), "query 0", "outside")
        refused(marg(bb=np.array([5, -1], np.int32)), "query 1", "outside")
        refused(rel(aa=np.array([1, 7], np.int32)), "query 1", "itself")
        for bad in (dict(tolerance=0.0), dict(tolerance=1.0), dict(tolerance=float("nan")), dict(max_cg_iterations=-1), dict(check_every=0),
                    dict(max_columns=7), dict(max_columns=-6)):
            p = sicp.default_graph_cov_params()
            for k, v in bad.items():
                setattr(p, k, v)
            refused(rel(p), "parameters")
            refused(marg(p), "parameters")
        # what follows is what the twin answers
        c1, s1, (i1,) = ask(pg, a, b)
        c2, s2, (i2,) = ask(twin, a, b)
        assert c1.tobytes() == c2.tobytes() and np.array_equal(s1, s2) and i1 == i2 and not s1.any()
        # status and info are optional
        assert L.sicp_graph_marginals(G, None, 2, ptr(b, ip), ptr(cov, dp), None, None) == sicp.OK
        assert np.isfinite(cov).all() and not np.any(cov == 7.0)


# ---- the arena's limit ------------------------------------------------------------------------------------------------------------
def _padded_ring(extra):
    """ring(closures=8) followed by `extra` free nodes without edges: identity blocks that make every work buffer large"""
    g = cases.ring(closures=8)
    lone = np.tile(np.array([0, 0, 0, 1, 0, 0, 0.0]), (extra, 1))
    g["poses"] = np.concatenate([g["poses"], lone])
    g["fixed"] = np.concatenate([g["fixed"], np.zeros(extra, dtype=bool)])
    return g


def _arena_bytes(count, size=8):
    """what a device buffer of `count` elements takes of the arena (the size classes of csrc/engine.hpp)"""
    b = (count + count // 8 + 64) * size
    if b <= 256:
        return 256
    p2 = 256
    while p2 < b:
        p2 <<= 1
    step = max(p2 >> 4, 256)
    return (b + step - 1) // step * step


def test_a_limit_that_fits_6_columns_but_not_24_gives_the_same_bytes():
    g = _padded_ring(20000)
    n = len(g["poses"])
    qa, qb = V.queries(cases.ring(closures=8), seed=3, pairs=3)
    with build(g) as pg, build(g) as free:
        want, st, (info,) = ask(free, qa, qb)
        assert info["passes"] == 1 and not st.any()
        pg.linearize()  # (the optimiser's buffers exist before the limit is set)
        vec6, vec12 = _arena_bytes(6 * n * 6), _arena_bytes(6 * n * 12)
        try:
            # room for the five vectors of 6 columns and the small buffers, not for those of 12
            sicp.set_memory_limit(0, sicp.memory_reserved(0) + 5 * vec6 + vec6 // 2)
            assert 5 * vec12 > 5 * vec6 + vec6 // 2
            got, s, (i,) = ask(pg, qa, qb)
        finally:
            sicp.set_memory_limit(0, 0)
        assert got.tobytes() == want.tobytes() and np.array_equal(s, st)
        assert i["passes"] == len(qb)  # (one query per pass)


def test_a_limit_too_small_for_six_columns_is_out_of_memory():
    """With the limit at one byte the arena takes no new slab.  Filler graphs ask for the blocks the call will ask for until the
    arena's free blocks and slab space of that size are used up and one is refused; from there the graph's own call must be
    refused, nothing written, and the graph must optimise as its twin."""
    L = sicp.lib()
    g = _padded_ring(100000)
    qb = np.array([5], np.int32)
    cov, st = np.full((1, 6, 6), 7.0), np.full(1, 7, np.int32)
    quick = sicp.default_graph_cov_params(max_cg_iterations=1)
    args = (C.byref(quick), 1, sicp._ptr(qb, sicp._ip), sicp._ptr(cov, sicp._dp), sicp._ptr(st, sicp._ip), None)
    p = sicp.default_graph_params(gradient_tolerance=1e-7, function_tolerance=0.0, parameter_tolerance=0.0)
    fillers = []
    with build(g, p) as pg, build(g, p) as twin:
        pg.linearize()
        before = pg.poses().tobytes()
        try:
            fillers = [build(g) for _ in range(48)]
            for f in fillers:
                f.linearize()  # (as the graph under test: the call's first request is for its own buffers)
            sicp.set_memory_limit(0, 1)
            hit = False
            for f in fillers:
                status = L.sicp_graph_marginals(f._g, *args)
                if status == sicp.ERR_OUT_OF_MEMORY:
                    hit = True
                    break
                assert status == sicp.OK
            assert hit, "48 fillers of 160 MB found room: the arena holds more free space than this test allows for"
            cov[:], st[:] = 7.0, 7
            status = L.sicp_graph_marginals(pg._g, *args)
            text = L.sicp_graph_last_error(pg._g).decode()
        finally:
            sicp.set_memory_limit(0, 0)
            for f in fillers:
                f.close()
        assert status == sicp.ERR_OUT_OF_MEMORY, text
        assert text.startswith("sicp_graph_marginals: ") and "out of memory" in text and "unchanged" in text
        assert np.all(cov == 7.0) and np.all(st == 7) and pg.poses().tobytes() == before
        a, b = pg.optimize(), twin.optimize()
        assert a == b and pg.poses().tobytes() == twin.poses().tobytes() and a["accepted_steps"] >= 1


# ---- end to end: gating a loop closure ----------------------------------------------------------------------------------------
# the seed chosen on the CPU restatement for wide margins on both sides: chi2 6.7 for the true closure, 715 for the false one
GATE_SEED, GATE_A, GATE_B = 7, 12, 47


def gate_candidates(g, seed=GATE_SEED, a=GATE_A, b=GATE_B):
    """a true closure between nodes a and b (the truth plus measurement noise) and a false one (the same, off by the transform of
    pose_graph_cases' outliers), with the measurement's covariance"""
    rng = np.random.default_rng(seed)
    sigma = np.array([cases.SIGMA_T] * 3 + [cases.SIGMA_R] * 3)
    z_true = R.mul(R.mul(R.inverse(g["truth"][a]), g["truth"][b]), R.exp(rng.normal(size=6) * sigma))
    z_false = R.mul(z_true, R.exp(np.array([3.0, -2.0, 1.0, 0.3, -0.5, 0.8])))
    return z_true, z_false, np.diag(sigma ** 2)


def gate_chi2(poses, cov_rel, Sigma_z, z, a=GATE_A, b=GATE_B):
    r = R.log(R.mul(R.inverse(R.mul(R.inverse(poses[a]), poses[b])), z))
    return float(r @ np.linalg.solve(cov_rel + Sigma_z, r))


def test_gating_a_loop_closure_before_it_enters_the_graph():
    g = cases.ring(closures=1)
    z_true, z_false, Sigma_z = gate_candidates(g)
    p = sicp.default_graph_params(gradient_tolerance=1e-7, function_tolerance=0.0, parameter_tolerance=0.0)
    with build(g, p) as pg:
        assert pg.optimize()["termination_name"] == "gradient"
        poses = pg.poses()
        cov, st, _ = pg.relative_covariances([GATE_A], [GATE_B])
        assert st[0] == sicp.GRAPH_COV_OK
        good, bad = gate_chi2(poses, cov[0], Sigma_z, z_true), gate_chi2(poses, cov[0], Sigma_z, z_false)
        print(f"graph_cov gating: chi2 of the true closure {good:.3f}, of the false one {bad:.3e}; the 99 % gate (6 dof) {CHI2_6_99:.2f}")
        assert good < CHI2_6_99 < bad
        # the reference at the optimised poses agrees on both
        ref, _, _ = V.reference(g, [GATE_A], [GATE_B], poses=poses)
        assert abs(gate_chi2(poses, ref[0], Sigma_z, z_true) - good) <= 1e-6 * good
        # the closure that passed goes in, and the trajectory tightens around it
        first = pg.add_edges([GATE_A], [GATE_B], z_true[None], np.linalg.inv(Sigma_z)[None])
        assert first == len(g["ei"])
        pg.optimize()
        after, st2, _ = pg.relative_covariances([GATE_A], [GATE_B])
        assert st2[0] == 0 and np.trace(after[0]) < np.trace(cov[0])
