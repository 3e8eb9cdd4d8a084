"""GPU tests of sicp_graph_* through the C ABI: the linearisation against the restatement (tests/pose_graph_ref.py), the
optimisation against the reference minimiser, the robust loss, determinism, the step control, the refusals and one loop closure
end to end.

Tolerances.  The kernels are compared at the tolerance of the header's host build (tests/pose_graph_cases.py, header_tolerance: 32 x the
restatement's own float64 rounding noise, relative to a block's largest magnitude or to the size of what it is formed from).  A
node's sums add `deg` such blocks: their error is that of the blocks plus deg * eps of the summation, relative to the sum of the
blocks' magnitudes."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as R
from pose_graph_cases import floors, header_tolerance

sicp = importlib.import_module("semantic-icp_amd")
pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
GTOL = 1e-7  # the gradient tolerance of the optimisation tests: far above the reference minimiser's own (1e-12 of the initial)


@functools.lru_cache(maxsize=1)
def tolerance():
    return header_tolerance()[1]


def build(g, params=None, calls=1):
    pg = sicp.PoseGraph(0, params)
    assert pg.add_nodes(g["poses"], g["fixed"]) == 0
    m = len(g["ei"])
    cuts = np.linspace(0, m, calls + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            assert pg.add_edges(g["ei"][a:b], g["ej"][a:b], g["z"][a:b], g["omega"][a:b]) == a
    return pg


def block_scale(A, floor):
    return np.maximum(np.abs(A).reshape(len(A), -1).max(axis=1), floor)


def check_linearisation(g, kind=R.LOSS_NONE, a=1.0):
    tol = tolerance()
    with build(g, sicp.default_graph_params(loss=kind, cauchy_a=a)) as pg:
        err, lin = pg.errors(), pg.linearize()
    n, m = len(g["poses"]), len(g["ei"])
    E = R.edges(g["poses"], g["ei"], g["ej"], g["z"], g["omega"], kind, a)
    F = floors(g["poses"][g["ei"]], g["poses"][g["ej"]], g["z"], g["omega"])
    worst = {}
    for name, got, want in (("r", err["residual"], E["r"]), ("s", err["chi2"], E["s"]), ("w", err["weight"], E["w"])):
        gap = np.abs(got - want).reshape(m, -1).max(axis=1) / block_scale(want, F[name])
        worst[name] = gap.max()
        assert np.all(gap <= tol), (name, gap.max(), tol)
    g_ref, H_ref = R.node_sums(n, g["fixed"], g["ei"], g["ej"], E)
    # per node: the sum of the incident blocks' scales and the degree
    gs, Hs, deg = np.zeros(n), np.zeros(n), np.zeros(n)
    for ends, gk, Hk in ((g["ei"], "gi", "Hi"), (g["ej"], "gj", "Hj")):
        np.add.at(gs, ends, block_scale(E[gk], F[gk]))
        np.add.at(Hs, ends, block_scale(E[Hk], 0.0))
        np.add.at(deg, ends, 1)
    free = ~np.asarray(g["fixed"], dtype=bool)
    bound = tol + deg * EPS
    ggap = np.abs(lin["gradient"] - g_ref).max(axis=1)
    Hgap = np.abs(lin["diag_blocks"] - H_ref).reshape(n, -1).max(axis=1)
    assert np.all(ggap[free] <= (bound * gs)[free]), (ggap[free] / np.maximum(gs[free], 1e-300)).max()
    assert np.all(Hgap[free] <= (bound * Hs)[free]), (Hgap[free] / np.maximum(Hs[free], 1e-300)).max()
    # a fixed node: the identity and zero, exactly; a node without edges: zeros, exactly
    assert np.array_equal(lin["diag_blocks"][~free], np.tile(np.eye(6), (int((~free).sum()), 1, 1)))
    assert not lin["gradient"][~free].any()
    lone = free & (deg == 0)
    assert not lin["diag_blocks"][lone].any() and not lin["gradient"][lone].any()
    cost_ref = 0.5 * float(E["rho"].sum())
    cost_scale = 0.5 * float(block_scale(E["rho"], F["rho"]).sum())
    for c in (err["cost"], lin["cost"]):
        assert abs(c - cost_ref) <= (tol + m * EPS) * cost_scale
    assert err["cost"] == lin["cost"]
    print("linearisation: worst relative gaps", {k: f"{v:.2e}" for k, v in worst.items()}, "tolerance", f"{tol:.2e}")


LINEAR_CASES = {
    "two_nodes": lambda: cases.two_nodes(),
    "triangle": lambda: cases.triangle(),
    "ring65": lambda: cases.ring(65, 1),
    "hub300": lambda: cases.hub(),
    "edges1": lambda: cases.counted(1),
    "edges255": lambda: cases.counted(255),
    "edges256": lambda: cases.counted(256),
    "edges257": lambda: cases.counted(257),
    "edges1025": lambda: cases.counted(1025),
    "residual_angles": lambda: cases.edge_case_graph(),
    "fixed_in_chain_and_lone_node": lambda: cases.chain(),
}


@pytest.mark.parametrize("name", list(LINEAR_CASES))
@pytest.mark.parametrize("kind", [R.LOSS_NONE, R.LOSS_CAUCHY], ids=["none", "cauchy"])
def test_linearisation_against_the_restatement(name, kind):
    check_linearisation(LINEAR_CASES[name](), kind, 1.5)


# ---- optimisation ------------------------------------------------------------------------------------------------------------
def opt_params(**kw):
    base = dict(gradient_tolerance=GTOL, function_tolerance=0.0, parameter_tolerance=0.0, max_iterations=200)
    base.update(kw)
    return sicp.default_graph_params(**base)


@functools.lru_cache(maxsize=None)
def reference(name, kind=R.LOSS_NONE, a=1.0):
    g = OPT_CASES[name]()
    x, info = R.minimise(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"], kind, a)
    assert info["converged"], name
    x.setflags(write=False)
    return g, x, info


def check_against_reference(g, x_ref, ref_info, got, info, kind=R.LOSS_NONE, a=1.0, dense=True):
    """the criteria of the issue, all computed by the restatement at the returned poses"""
    cost, grad, H = R.assemble(got, g["fixed"], g["ei"], g["ej"], g["z"], g["omega"], kind, a)
    gmax = float(np.abs(grad).max())
    print(f"info {info}\nrestated at the result: cost {cost:.12e} (reference {ref_info['cost']:.12e}), max |g| {gmax:.3e}")
    if info["termination_name"] == "gradient":
        assert gmax <= 10 * GTOL
    assert cost <= ref_info["cost"] * (1 + 1e-9)
    fixed = np.asarray(g["fixed"], dtype=bool)
    deg = np.bincount(np.concatenate([g["ei"], g["ej"]]), minlength=len(got))
    assert np.array_equal(got[fixed], g["poses"][fixed])
    assert np.array_equal(got[deg == 0], g["poses"][deg == 0])
    keep = np.repeat(~fixed & (deg > 0), 6)
    Href = ref_info["H"][keep][:, keep]
    if dense:
        lam = float(np.linalg.eigvalsh(Href.toarray())[0])
    else:
        import scipy.sparse.linalg as spla
        lam = float(spla.eigsh(Href, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])
    dist = R.tangent_distance(x_ref, got)
    print(f"distance to the reference minimiser {dist:.3e}, bound 2 |g| / lambda_min = {2 * np.linalg.norm(grad) / lam:.3e} (lambda_min {lam:.3e})")
    assert lam > 0 and dist < 2 * np.linalg.norm(grad) / lam


OPT_CASES = {
    "ring": lambda: cases.ring(65, 1),
    "hub": lambda: cases.hub(),
    "grid": lambda: cases.grid_world(),
    "ring_outliers": lambda: cases.ring(65, 20, seed=21, outliers=3),
}


@pytest.mark.parametrize("name", ["ring", "hub", "grid"])
def test_optimisation_against_the_reference_minimiser(name):
    g, x_ref, ref_info = reference(name)
    with build(g, opt_params()) as pg:
        info = pg.optimize()
        got = pg.poses()
    check_against_reference(g, x_ref, ref_info, got, info, dense=name != "grid")


def test_lone_and_fixed_nodes_keep_their_bytes_through_optimize():
    g = cases.chain(n=9, fixed_at=4, isolated=2)
    with build(g, opt_params()) as pg:
        info = pg.optimize()
        got = pg.poses()
    assert info["accepted_steps"] >= 1
    assert np.array_equal(got[[4, 9, 10]], g["poses"][[4, 9, 10]])
    assert not np.array_equal(got[0], g["poses"][0])


def test_robust_loss():
    a = 3.0
    g, x_c, ref_c = reference("ring_outliers", R.LOSS_CAUCHY, a)
    _, x_n, ref_n = reference("ring_outliers", R.LOSS_NONE, 1.0)
    with build(g, opt_params(loss=sicp.GRAPH_LOSS_CAUCHY, cauchy_a=a)) as pg:
        info_c = pg.optimize()
        got_c = pg.poses()
        chi2 = pg.errors()["chi2"]
    check_against_reference(g, x_c, ref_c, got_c, info_c, R.LOSS_CAUCHY, a)
    m = len(g["ei"])
    assert set(np.argsort(chi2)[-3:]) == {m - 3, m - 2, m - 1}
    with build(g, opt_params()) as pg:
        info_n = pg.optimize()
        got_n = pg.poses()
    check_against_reference(g, x_n, ref_n, got_n, info_n)
    assert R.tangent_distance(got_c, got_n) > 1e-2


# ---- determinism ---------------------------------------------------------------------------------------------------------------
def _info_bytes(info):
    return tuple((k, np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in sorted(info.items()))


def test_determinism():
    g = cases.ring(65, 6, seed=31)
    runs = []
    for calls in (1, 1, 5):
        with build(g, opt_params(), calls=calls) as pg:
            info = pg.optimize()
            first = pg.poses()
            again = pg.optimize()
            second = pg.poses()
        runs.append((first.tobytes(), _info_bytes(info)))
        assert info["accepted_steps"] >= 1
        assert again["accepted_steps"] == 0 and second.tobytes() == first.tobytes()
    assert runs[0] == runs[1], "the same graph built twice"
    assert runs[0] == runs[2], "the edges added in one call or in five"


# ---- step control --------------------------------------------------------------------------------------------------------------
def test_a_rejected_first_step_and_convergence_after_it():
    g = cases.step_control()
    r0 = R.residual(g["poses"][g["ei"]], g["poses"][g["ej"]], g["z"])
    assert 2.8 < np.linalg.norm(r0[-1, 3:]) < 3.1
    _, ref = R.minimise(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"], initial_radius=1e16, max_iterations=1)
    assert ref["first_step_rejected"], "the reference accepts the first full step: the case does not exercise the step control"
    # The closure is an outlier of 3 rad under a quadratic loss: the cost at the minimum is large and Gauss-Newton converges
    # linearly.  "Converges": the run ends on one of its tolerances with the gradient down by 1e-6 from the start.
    _, g0, _ = R.assemble(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"])
    with build(g, opt_params(initial_radius=1e16, gradient_tolerance=1e-7 * np.abs(g0).max(), function_tolerance=1e-14, max_iterations=1000)) as pg:
        info = pg.optimize()
        got = pg.poses()
    print(info)
    assert info["rejected_steps"] >= 1 and info["termination_name"] in ("gradient", "function")
    _, grad, _ = R.assemble(got, g["fixed"], g["ei"], g["ej"], g["z"], g["omega"])
    assert np.abs(grad).max() <= 1e-6 * np.abs(g0).max() and info["final_cost"] < info["initial_cost"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _snapshot(pg):
    n, m = pg.size()
    e = pg.errors() if m else {"chi2": np.zeros(0), "residual": np.zeros(0), "weight": np.zeros(0), "cost": 0.0}
    return (n, m, pg.poses().tobytes() if n else b"", e["chi2"].tobytes(), e["residual"].tobytes(), e["weight"].tobytes(), e["cost"])


def test_create_refuses_bad_parameters():
    L = sicp.lib()
    h = C.c_void_p()
    assert L.sicp_graph_create(0, None, C.byref(h)) == sicp.ERR_INVALID_ARGUMENT
    assert L.sicp_graph_create(0, C.byref(sicp.default_graph_params()), None) == sicp.ERR_INVALID_ARGUMENT
    assert L.sicp_graph_create(-1, C.byref(sicp.default_graph_params()), C.byref(h)) == sicp.ERR_INVALID_ARGUMENT
    assert L.sicp_default_graph_params(None) == sicp.ERR_INVALID_ARGUMENT
    bad = [dict(loss=2), dict(cauchy_a=0.0), dict(cauchy_a=float("nan")), dict(max_iterations=-1), dict(gradient_tolerance=-1.0),
           dict(function_tolerance=float("nan")), dict(parameter_tolerance=-1e-3), dict(initial_radius=0.0), dict(min_radius=0.0),
           dict(initial_radius=1e20), dict(max_radius=float("inf")), dict(min_relative_decrease=1.0), dict(min_relative_decrease=-0.1),
           dict(min_lm_diagonal=0.0), dict(max_lm_diagonal=1e-9), dict(max_consecutive_invalid_steps=0), dict(max_cg_iterations=0),
           dict(cg_eta=0.0), dict(cg_eta=1.0), dict(cg_check_every=0)]
    for kw in bad:
        assert L.sicp_graph_create(0, C.byref(sicp.default_graph_params(**kw)), C.byref(h)) == sicp.ERR_INVALID_ARGUMENT, kw
        assert not h.value


def test_refusals_leave_the_graph_as_it_was():
    L = sicp.lib()
    g = cases.triangle()
    dp, ip, bp = sicp._dp, sicp._ip, sicp._bp
    ptr = sicp._ptr
    with build(g) as pg:
        before = _snapshot(pg)
        G = pg._g
        first = C.c_int32(-7)
        ok_pose = np.array([[0, 0, 0, 1, 1, 2, 3.0]])
        ok_om = np.eye(6)[None].copy()
        i01, j01 = np.array([0], np.int32), np.array([1], np.int32)

        def refused(st, *needles):
            text = L.sicp_graph_last_error(G).decode()
            assert st == sicp.ERR_INVALID_ARGUMENT, (st, text)
            for n in needles:
                assert n in text, text
            assert _snapshot(pg) == before and first.value == -7

        def nodes(q, n=None, fixed=None):
            q = np.ascontiguousarray(q, dtype=np.float64)
            return L.sicp_graph_add_nodes(G, len(q) if n is None else n, ptr(q, dp), fixed, C.byref(first))

        def edges(i, j, z, om, m=None):
            z, om = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(om, dtype=np.float64)
            i, j = np.asarray(i, np.int32), np.asarray(j, np.int32)
            return L.sicp_graph_add_edges(G, len(i) if m is None else m, ptr(i, ip), ptr(j, ip), ptr(z, dp), ptr(om, dp), C.byref(first))

        # nodes
        refused(L.sicp_graph_add_nodes(G, 1, None, None, C.byref(first)), "NULL")
        refused(nodes(ok_pose, n=0), "n must be >= 1")
        for col, v in ((4, np.nan), (0, np.inf)):
            q = np.repeat(ok_pose, 3, axis=0); q[2, col] = v
            refused(nodes(q), "pose 2", "not finite")
        q = np.repeat(ok_pose, 2, axis=0); q[1, 3] = 1 + 3e-6
        refused(nodes(q), "pose 1", "quaternion")
        # edges
        refused(L.sicp_graph_add_edges(G, 1, None, ptr(j01, ip), ptr(ok_pose, dp), ptr(ok_om, dp), C.byref(first)), "NULL")
        refused(L.sicp_graph_add_edges(G, 1, ptr(i01, ip), ptr(j01, ip), None, ptr(ok_om, dp), C.byref(first)), "NULL")
        refused(L.sicp_graph_add_edges(G, 1, ptr(i01, ip), ptr(j01, ip), ptr(ok_pose, dp), None, C.byref(first)), "NULL")
        refused(edges(i01, j01, ok_pose, ok_om, m=0), "m must be >= 1")
        refused(edges([0, 1], [1, 3], np.repeat(ok_pose, 2, 0), np.repeat(ok_om, 2, 0)), "edge 1", "outside")
        refused(edges([-1], [1], ok_pose, ok_om), "edge 0", "outside")
        refused(edges([0, 2], [1, 2], np.repeat(ok_pose, 2, 0), np.repeat(ok_om, 2, 0)), "edge 1", "itself")
        z = ok_pose.copy(); z[0, 5] = np.nan
        refused(edges(i01, j01, z, ok_om), "edge 0", "not finite")
        z = ok_pose.copy(); z[0, 3] = 0.99
        refused(edges(i01, j01, z, ok_om), "edge 0", "quaternion")
        om = ok_om.copy(); om[0, 2, 3] = np.inf
        refused(edges(i01, j01, ok_pose, om), "edge 0", "not finite")
        om = ok_om.copy(); om[0, 2, 3] = 1e-6
        refused(edges(i01, j01, ok_pose, om), "edge 0", "not symmetric")
        om = ok_om.copy(); om[0, 4, 4] = -1.0
        refused(edges(i01, j01, ok_pose, om), "edge 0", "positive definite")
        om2 = np.repeat(ok_om, 2, 0); om2[1] = np.ones((6, 6))  # singular
        refused(edges([0, 1], [1, 2], np.repeat(ok_pose, 2, 0), om2), "edge 1", "positive definite")
        # ranges
        buf = np.zeros((4, 7))
        refused(L.sicp_graph_get_poses(G, 2, 2, ptr(buf, dp)), "beyond")
        refused(L.sicp_graph_get_poses(G, -1, 1, ptr(buf, dp)), "first")
        refused(L.sicp_graph_get_poses(G, 0, 0, ptr(buf, dp)), "count")
        refused(L.sicp_graph_get_poses(G, 0, 1, None), "NULL")
        assert not buf.any()
        refused(L.sicp_graph_set_poses(G, 2, 2, ptr(np.repeat(ok_pose, 2, 0), dp)), "beyond")
        refused(L.sicp_graph_set_poses(G, 0, 1, None), "NULL")
        q = ok_pose.copy(); q[0, 0] = 0.5
        refused(L.sicp_graph_set_poses(G, 0, 1, ptr(q, dp)), "quaternion")
        flags = np.ones(4, np.uint8)
        refused(L.sicp_graph_set_fixed(G, 1, 3, ptr(flags, bp)), "beyond")
        refused(L.sicp_graph_set_fixed(G, 0, 1, None), "NULL")
        refused(L.sicp_graph_errors(G, None, None, None, None), "NULL")
        refused(L.sicp_graph_linearize(G, None, None, None), "NULL")
        refused(L.sicp_graph_optimize(G, None), "NULL")
        refused(L.sicp_graph_size(G, None, None), "NULL")
        # an asymmetry below 1e-9 of the largest entry is accepted and the mean of the two halves stored; a quaternion within
        # 1e-6 of unit norm is stored normalised
        om = ok_om.copy() * 100.0; om[0, 1, 2] = 2e-8
        zq = ok_pose.copy(); zq[0, 3] = 1 + 5e-7
        first.value = -1
        assert edges([2], [0], zq, om) == sicp.OK and first.value == 3
        om_sym = om[0].copy(); om_sym[1, 2] = om_sym[2, 1] = 1e-8
        zn = zq.copy(); zn[0, :4] /= np.linalg.norm(zn[0, :4])
        e = pg.errors()
        r = R.residual(g["poses"][[2]], g["poses"][[0]], zn)[0]
        assert abs(e["chi2"][3] - r @ om_sym @ r) <= 1e-12 * e["chi2"][3]
        assert pg.size() == (3, 4)


def test_optimize_needs_a_fixed_node_and_an_edge():
    L = sicp.lib()
    g = cases.triangle()
    info = sicp.SicpGraphInfo()
    with sicp.PoseGraph(0) as pg:
        pg.add_nodes(g["poses"], g["fixed"])
        assert L.sicp_graph_optimize(pg._g, C.byref(info)) == sicp.ERR_NOT_READY
        assert "no edge" in L.sicp_graph_last_error(pg._g).decode()
        pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
        pg.set_fixed([False], first=1)
        before = _snapshot(pg)
        assert L.sicp_graph_optimize(pg._g, C.byref(info)) == sicp.ERR_NOT_READY
        assert "no fixed node" in L.sicp_graph_last_error(pg._g).decode()
        assert _snapshot(pg) == before
        pg.set_fixed([True], first=1)
        assert pg.optimize()["accepted_steps"] >= 1
        pg.clear()
        assert pg.size() == (0, 0)


def test_a_memory_limit_refuses_add_edges_and_the_graph_optimises_as_its_twin():
    """With the limit at one byte the arena takes no new slab.  Filler graphs ask for the blocks the large add_edges will ask for
    until the arena's free blocks and slab space of that size are used up and one is refused; from there the graph's own call
    must be refused, the graph unchanged, and its optimisation the twin's byte for byte."""
    L = sicp.lib()
    g = cases.ring(65, 4, seed=41)
    m = 200_001
    ei, ej = np.zeros(m, np.int32), np.ones(m, np.int32)
    z = np.tile(np.array([0, 0, 0, 1, 0, 0, 0.0]), (m, 1))
    om = np.tile(np.eye(6), (m, 1, 1))
    args = (m, sicp._ptr(ei, sicp._ip), sicp._ptr(ej, sicp._ip), sicp._ptr(z, sicp._dp), sicp._ptr(om, sicp._dp), None)
    fillers = []
    with build(g, opt_params()) as pg, build(g, opt_params()) as twin:
        before = _snapshot(pg)
        try:
            fillers = [sicp.PoseGraph(0) for _ in range(64)]
            for f in fillers:
                f.add_nodes(g["poses"][:2])
            sicp.set_memory_limit(0, 1)
            hit = False
            for f in fillers:
                st = L.sicp_graph_add_edges(f._g, *args)
                if st == sicp.ERR_OUT_OF_MEMORY:
                    hit = True
                    assert f.size() == (2, 0)
                    break
                assert st == sicp.OK
            assert hit, "64 fillers of 70 MB found room: the arena holds more free space than this test allows for"
            st = L.sicp_graph_add_edges(pg._g, *args)
            text = L.sicp_graph_last_error(pg._g).decode()
        finally:
            sicp.set_memory_limit(0, 0)
            for f in fillers:
                f.close()
        assert st == sicp.ERR_OUT_OF_MEMORY
        assert text.startswith("sicp_graph_add_edges: ") and "out of memory" in text and text.endswith("the graph is unchanged")
        assert _snapshot(pg) == before
        a, b = pg.optimize(), twin.optimize()
        assert _info_bytes(a) == _info_bytes(b) and pg.poses().tobytes() == twin.poses().tobytes()
        assert a["accepted_steps"] >= 1


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def test_a_loop_closure_moves_the_trajectory():
    """The street of tests/place_cases.py: 17 keyframes and the first revisit as node 17.  Odometry from the true poses with a
    seeded drift, one closure from sicp_align started at place_init_qt(yaw), weighted by the inverse of its pose covariance."""
    import np_ref
    import place_cases as PC
    import synth

    sc = PC.scene()
    entry, _, yaw_deg = sc["revisits"][0]
    truth_mats = list(sc["entry_poses"]) + [sc["query_poses"][0]]
    truth = np.array([np_ref.mat_to_qt(M) for M in truth_mats])
    n = len(truth)
    rng = np.random.default_rng(5)
    ei, ej = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    sig = np.array([0.05] * 3 + [np.deg2rad(0.5)] * 3)
    z_odo = R.mul(R.mul(R.inverse(truth[ei]), truth[ej]), R.exp(rng.normal(size=(n - 1, 6)) * sig))
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = PC.SCENE_CLASSES
    with sicp.Engine(0, p) as e:
        e.set_confusion(synth.confusion_matrix(PC.SCENE_CLASSES))
        e.set_source(*sc["queries"][0])      # node j: the revisit
        e.set_target(*sc["entries"][entry])  # node i: the keyframe it sees again
        z_loop, _ = e.align(sicp.place_init_qt(np.deg2rad(yaw_deg)))
        cov = e.pose_covariance(z_loop)
    assert cov["positive_definite"]
    omega_loop = np.linalg.inv(cov["covariance"])
    g = dict(poses=cases._integrate(truth, z_odo), fixed=np.arange(n) == 0,
             ei=np.append(ei, entry).astype(np.int32), ej=np.append(ej, n - 1).astype(np.int32),
             z=np.concatenate([z_odo, np.asarray(z_loop)[None]]),
             omega=np.concatenate([np.tile(np.diag(1 / sig ** 2), (n - 1, 1, 1)), 0.5 * (omega_loop + omega_loop.T)[None]]))
    x_ref, ref_info = R.minimise(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"])
    assert ref_info["converged"]
    with build(g, opt_params()) as pg:
        info = pg.optimize()
        got = pg.poses()
    check_against_reference(g, x_ref, ref_info, got, info)
    before = np.linalg.norm(g["poses"][:, 4:] - truth[:, 4:], axis=1).mean()
    after = np.linalg.norm(got[:, 4:] - truth[:, 4:], axis=1).mean()
    print(f"mean translation error {before:.3f} m -> {after:.3f} m")
    assert after < before
