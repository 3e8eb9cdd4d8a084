"""GPU tests of the pose graph's priors and enabled flags through the C ABI (include/sicp.h, "pose graph", rules 5 - 12): the
linearisation against the restatement (tests/pose_graph_prior_ref.py), the exact statements, the optimisation against the
reference minimisers (the restatement's and, for pose priors, the unchanged pose_graph_ref on the identity-twin), the
covariances with priors and cut-off components, readiness and refusals, and the bytes of a graph without priors against those
recorded from the build before priors existed (tests/golden/graph_parent_bytes.json).

Tolerances are those of tests/test_gpu_pose_graph.py: header_tolerance() per block, tol + deg * eps on a node's sums with the
node's enabled priors counted in deg; the optimisation criteria of check_against_reference; graph_cov_ref.bound for covariances."""
import ctypes as C
import functools
import hashlib
import importlib
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import scipy.sparse.linalg as spla

import graph_cov_ref as V
import pose_graph_cases as cases
import pose_graph_prior_ref as P
import pose_graph_ref as R
import test_gpu_pose_graph as base
from pose_graph_cases import floors, header_tolerance

sicp = importlib.import_module("semantic-icp_amd")
pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
GTOL = base.GTOL
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph_parent_bytes.json")
COV_TOLERANCE = 1e-10


@functools.lru_cache(maxsize=1)
def tolerance():
    return header_tolerance()[1]


def build(g, pri=None, params=None, e_on=None, p_on=None, calls=1):
    pg = base.build(g, params, calls)
    if pri is not None and len(pri["node"]):
        assert P.add_to(pg, pri) == 0
    if e_on is not None:
        pg.set_edges_enabled(e_on)
    if p_on is not None:
        pg.set_priors_enabled(p_on)
    return pg


def make_priors(g, nodes, kinds, seed=0, noise=0.05):
    """priors near the truth: a pose prior z = truth exp(noise) with a random information matrix, a position prior the true
    position plus noise with the leading 3x3 of one"""
    rng = np.random.default_rng(seed)
    z, om = [], []
    for k, kind in zip(nodes, kinds):
        T = g["truth"][k]
        spd = cases.random_spd(rng, 1)[0]
        if kind == P.POSE:
            z.append(R.mul(T, R.exp(rng.normal(size=6) * noise))); om.append(spd)
        else:
            z.append(T[4:] + rng.normal(size=3) * noise); om.append(spd[:3, :3])
    return P.make(nodes, kinds, z, om)


def mixed(g, count, seed):
    """`count` priors of mixed kinds on random nodes, the first three (where there are three) on one node"""
    rng = np.random.default_rng(seed)
    nodes = rng.integers(0, len(g["poses"]), size=count)
    nodes[:3] = 5
    return make_priors(g, nodes, rng.integers(0, 2, size=count), seed + 1)


def block_scale(A, floor):
    return np.maximum(np.abs(A).reshape(len(A), -1).max(axis=1), floor)


# ---- 1. linearisation -----------------------------------------------------------------------------------------------------------
def check_linearisation(g, pri, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0):
    tol = tolerance()
    n, m, np_ = len(g["poses"]), len(g["ei"]), len(pri["node"])
    e_on, p_on = P._masks(m, np_, e_on, p_on)
    with build(g, pri, sicp.default_graph_params(loss=kind, cauchy_a=a), e_on, p_on) as pg:
        err, perr, lin = pg.errors(), pg.prior_errors(), pg.linearize()
        assert pg.counts() == dict(nodes=n, edges=m, edges_enabled=int(e_on.sum()), priors=np_, priors_enabled=int(p_on.sum()))
        assert np.array_equal(pg.edges_enabled(), e_on) and np.array_equal(pg.priors_enabled(), p_on)
    E = R.edges(g["poses"], g["ei"], g["ej"], g["z"], g["omega"], kind, a)
    F = floors(g["poses"][g["ei"]], g["poses"][g["ej"]], g["z"], g["omega"])
    PE = P.priors(g["poses"], pri, kind, a)
    PF = P.floors(g["poses"][pri["node"]], pri)
    # every entry at the current poses, a disabled one too
    for name, got, want in (("r", err["residual"], E["r"]), ("s", err["chi2"], E["s"]), ("w", err["weight"], E["w"])):
        gap = np.abs(got - want).reshape(m, -1).max(axis=1) / block_scale(want, F[name])
        assert np.all(gap <= tol), ("edge", name, gap.max(), tol)
    for name, got, want in (("r", perr["residual"], PE["r"]), ("s", perr["chi2"], PE["s"]), ("w", perr["weight"], PE["w"])):
        gap = np.abs(got - want).reshape(np_, -1).max(axis=1) / block_scale(want, PF[name])
        assert np.all(gap <= tol), ("prior", name, gap.max(), tol)
    assert not perr["residual"][pri["kind"] == P.POSITION, 3:].any()
    g_ref, H_ref = P.node_sums(g, pri, E, PE, e_on, p_on)
    gs, Hs, deg = np.zeros(n), np.zeros(n), np.zeros(n)
    for ends, gk, Hk in ((g["ei"], "gi", "Hi"), (g["ej"], "gj", "Hj")):
        np.add.at(gs, ends[e_on], block_scale(E[gk], F[gk])[e_on])
        np.add.at(Hs, ends[e_on], block_scale(E[Hk], 0.0)[e_on])
        np.add.at(deg, ends[e_on], 1)
    np.add.at(gs, pri["node"][p_on], block_scale(PE["g"], PF["g"])[p_on])
    np.add.at(Hs, pri["node"][p_on], block_scale(PE["H"], 0.0)[p_on])
    np.add.at(deg, pri["node"][p_on], 1)
    free = ~np.asarray(g["fixed"], dtype=bool)
    bound = tol + deg * EPS
    ggap = np.abs(lin["gradient"] - g_ref).max(axis=1)
    Hgap = np.abs(lin["diag_blocks"] - H_ref).reshape(n, -1).max(axis=1)
    assert np.all(ggap[free] <= (bound * gs)[free]), (ggap[free] / np.maximum(gs[free], 1e-300)).max()
    assert np.all(Hgap[free] <= (bound * Hs)[free]), (Hgap[free] / np.maximum(Hs[free], 1e-300)).max()
    # a fixed node, with or without priors: the identity and zero, exactly; a node without enabled entries: zeros, exactly
    assert np.array_equal(lin["diag_blocks"][~free], np.tile(np.eye(6), (int((~free).sum()), 1, 1)))
    assert not lin["gradient"][~free].any()
    lone = free & (deg == 0)
    assert not lin["diag_blocks"][lone].any() and not lin["gradient"][lone].any()
    cost_ref = 0.5 * float(E["rho"][e_on].sum() + PE["rho"][p_on].sum())
    cost_scale = 0.5 * float(block_scale(E["rho"], F["rho"])[e_on].sum() + block_scale(PE["rho"], PF["rho"])[p_on].sum())
    assert abs(lin["cost"] - cost_ref) <= (tol + (m + np_) * EPS) * cost_scale
    assert err["cost"] == lin["cost"] == perr["cost"]


def _two_nodes():
    g = cases.two_nodes()
    return g, make_priors(g, [1, 1], [P.POSE, P.POSITION], 60), None, None


def _chain():
    g = cases.chain()  # node 4 fixed, node 9 without edges, node 2 free
    return g, make_priors(g, [4, 9, 2, 4, 9, 2], [P.POSE] * 3 + [P.POSITION] * 3, 61), None, None


def _ring(count):
    g = cases.ring(65, 1)
    return g, mixed(g, count, 62 + count), None, None


def _counted(which):
    g = cases.counted(257)
    m = len(g["ei"])
    off = {"none": np.zeros(m, dtype=bool), "all": np.ones(m, dtype=bool), "every_second": np.arange(m) % 2 == 1,
           "first": np.arange(m) == 0, "last": np.arange(m) == m - 1, "one_nodes": (g["ei"] == 11) | (g["ej"] == 11)}[which]
    assert which == "none" or off.any()
    pri = make_priors(g, [11, 11, 40], [P.POSE, P.POSITION, P.POSITION], 63)
    return g, pri, ~off, np.array([True, False, True])  # (a disabled prior is still reported)


LINEAR_CASES = {"two_nodes": _two_nodes, "chain_fixed_lone_free": _chain}
LINEAR_CASES.update({f"ring65_priors{c}": functools.partial(_ring, c) for c in (1, 63, 64, 65, 257)})
LINEAR_CASES.update({f"edges257_off_{w}": functools.partial(_counted, w) for w in ("none", "all", "every_second", "first", "last", "one_nodes")})


@pytest.mark.parametrize("name", list(LINEAR_CASES))
@pytest.mark.parametrize("kind", [R.LOSS_NONE, R.LOSS_CAUCHY], ids=["none", "cauchy"])
def test_linearisation_against_the_restatement(name, kind):
    g, pri, e_on, p_on = LINEAR_CASES[name]()
    check_linearisation(g, pri, e_on, p_on, kind, 1.5)


# ---- 2. exact statements ----------------------------------------------------------------------------------------------------------
def test_a_node_with_everything_disabled_is_a_node_without_edges():
    g = cases.chain(n=9, fixed_at=4, isolated=1)
    pri = make_priors(g, [0, 0, 6], [P.POSE, P.POSITION, P.POSITION], 70)
    e_on = np.ones(8, dtype=bool)
    e_on[0] = False  # node 0's only edge
    with build(g, pri, base.opt_params(), e_on, [False, False, True]) as pg:
        lin = pg.linearize()
        assert not lin["diag_blocks"][0].any() and not lin["gradient"][0].any() and lin["diag_blocks"][1].any()
        info = pg.optimize()
        got = pg.poses()
    assert info["accepted_steps"] >= 1
    assert np.array_equal(got[[0, 4, 9]], g["poses"][[0, 4, 9]])
    assert not np.array_equal(got[1], g["poses"][1]) and not np.array_equal(got[6], g["poses"][6])


def test_a_prior_on_a_fixed_node_counts_in_the_cost_and_nowhere_else():
    g = cases.triangle()  # node 1 fixed
    pri = make_priors(g, [1, 1], [P.POSE, P.POSITION], 71)
    with build(g) as plain, build(g, pri) as pg:
        a, b = plain.linearize(), pg.linearize()
        assert np.array_equal(b["diag_blocks"][1], np.eye(6)) and not b["gradient"][1].any()
        assert a["gradient"].tobytes() == b["gradient"].tobytes() and a["diag_blocks"].tobytes() == b["diag_blocks"].tobytes()
        want = 0.5 * float(P.priors(g["poses"], pri)["rho"].sum())
        assert want > 0 and abs((b["cost"] - a["cost"]) - want) <= 1e-12 * b["cost"]


def _outputs(pg):
    lin = pg.linearize()
    info = pg.optimize()
    return (lin["gradient"].tobytes(), lin["diag_blocks"].tobytes(), np.float64(lin["cost"]).tobytes(), base._info_bytes(info), pg.poses().tobytes())


def test_disabling_and_enabling_again_is_byte_equal_to_never_touching_the_flags():
    g = cases.ring(65, 6, seed=31)
    pri = mixed(g, 9, 72)
    with build(g, pri, base.opt_params()) as pg, build(g, pri, base.opt_params()) as twin:
        e_off = np.ones(len(g["ei"]), dtype=bool)
        e_off[[0, 17, 66]] = False
        pg.set_edges_enabled(e_off)
        pg.set_priors_enabled([False, True, False])
        assert pg.linearize()["gradient"].tobytes() != twin.linearize()["gradient"].tobytes()
        pg.set_edges_enabled(np.ones(len(g["ei"]), dtype=bool))
        pg.set_priors_enabled([True] * 9)
        assert pg.counts() == twin.counts()
        # setting the flags to the values they have is a no-op
        pg.set_edges_enabled([True, True], first=3)
        assert _outputs(pg) == _outputs(twin)


def test_determinism_with_priors_and_flags():
    g = cases.ring(65, 6, seed=31)
    g["fixed"][:] = False
    pri = mixed(g, 70, 73)
    e_on = np.arange(len(g["ei"])) % 7 != 3
    p_on = np.arange(70) % 5 != 2
    runs = []
    for calls in (1, 1, 5):
        with build(g, pri, base.opt_params(), e_on, p_on, calls=calls) as pg:
            out = _outputs(pg)
            again = pg.optimize()
            assert again["accepted_steps"] == 0 and pg.poses().tobytes() == out[-1]
        runs.append(out)
    assert dict(runs[0][3])["accepted_steps"] >= 1
    assert runs[0] == runs[1], "the same graph built twice"
    assert runs[0] == runs[2], "the edges added in one call or in five"


# ---- 3. optimisation ----------------------------------------------------------------------------------------------------------
def check_against_reference(g, pri, e_on, p_on, x_ref, ref_info, got, info, kind=R.LOSS_NONE, a=1.0):
    """test_gpu_pose_graph.check_against_reference with priors and flags: every criterion computed by the restatement at the
    returned poses"""
    e_on, p_on = P._masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    cost, grad, _ = P.assemble(got, g, pri, e_on, p_on, kind, a)
    gmax = float(np.abs(grad).max())
    print(f"info {info}\nrestated at the result: cost {cost:.12e} (reference {ref_info['cost']:.12e}), max |g| {gmax:.3e}")
    if info["termination_name"] == "gradient":
        assert gmax <= 10 * GTOL
    assert cost <= ref_info["cost"] * (1 + 1e-9)
    fixed = np.asarray(g["fixed"], dtype=bool)
    deg = np.bincount(np.concatenate([g["ei"][e_on], g["ej"][e_on], pri["node"][p_on]]), minlength=len(got))
    assert np.array_equal(got[fixed], g["poses"][fixed])
    assert np.array_equal(got[deg == 0], g["poses"][deg == 0])
    keep = np.repeat(~fixed & (deg > 0), 6)
    lam = float(np.linalg.eigvalsh(ref_info["H"][keep][:, keep].toarray())[0])
    dist = R.tangent_distance(x_ref, got)
    print(f"distance to the reference minimiser {dist:.3e}, bound 2 |g| / lambda_min = {2 * np.linalg.norm(grad) / lam:.3e} (lambda_min {lam:.3e})")
    assert lam > 0 and dist < 2 * np.linalg.norm(grad) / lam


def test_a_pose_prior_in_place_of_the_fixed_node_against_both_oracles():
    g = cases.ring(65, 1)
    g["fixed"][:] = False
    pri = P.make([0], [P.POSE], [g["poses"][0]], [np.diag([1e4] * 3 + [1e3] * 3)])
    x_ref, ref_info = P.minimise(g, pri)
    assert ref_info["converged"]
    with build(g, pri, base.opt_params()) as pg:
        info = pg.optimize()
        got = pg.poses()
    assert info["accepted_steps"] >= 1
    check_against_reference(g, pri, None, None, x_ref, ref_info, got, info)
    # the identity-twin through the unchanged pose_graph_ref and the unchanged criteria
    t = P.identity_twin(g, pri)
    xt, t_info = R.minimise(t["poses"], t["fixed"], t["ei"], t["ej"], t["z"], t["omega"])
    assert t_info["converged"]
    base.check_against_reference(t, xt, t_info, np.concatenate([got, P.IDENTITY[None]]), info)


def test_disabled_outliers_meet_the_minimiser_of_the_graph_without_them():
    g = cases.ring(65, 20, seed=21, outliers=3)
    m = len(g["ei"])
    e_on = np.arange(m) < m - 3
    without = dict(g, ei=g["ei"][e_on], ej=g["ej"][e_on], z=g["z"][e_on], omega=g["omega"][e_on])
    x_ref, ref_info = R.minimise(without["poses"], without["fixed"], without["ei"], without["ej"], without["z"], without["omega"])
    assert ref_info["converged"]
    with build(g, None, base.opt_params(), e_on) as pg:
        info = pg.optimize()
        got = pg.poses()
        chi2 = pg.errors()["chi2"]
    base.check_against_reference(without, x_ref, ref_info, got, info)
    assert set(np.argsort(chi2)[-3:]) == {m - 3, m - 2, m - 1}  # still reported, and still the worst


def test_position_priors_and_gps_outliers_under_cauchy():
    a = 3.0
    g = cases.ring(65, 1)
    g["fixed"][:] = False
    nodes = list(range(0, 65, 8))
    om = np.eye(3) / 0.05 ** 2
    z = [g["truth"][k, 4:] for k in nodes] + [g["truth"][3, 4:] + np.array([5.0, -4.0, 3.0]), g["truth"][30, 4:] + np.array([-6.0, 2.0, 4.0])]
    pri = P.make(nodes + [3, 30], [P.POSITION] * (len(nodes) + 2), z, [om] * (len(nodes) + 2))
    x_ref, ref_info = P.minimise(g, pri, kind=R.LOSS_CAUCHY, a=a)
    assert ref_info["converged"]
    with build(g, pri, base.opt_params(loss=sicp.GRAPH_LOSS_CAUCHY, cauchy_a=a)) as pg:
        info = pg.optimize()
        got = pg.poses()
        chi2 = pg.prior_errors()["chi2"]
    check_against_reference(g, pri, None, None, x_ref, ref_info, got, info, R.LOSS_CAUCHY, a)
    assert set(np.argsort(chi2)[-2:]) == {len(nodes), len(nodes) + 1}
    assert np.linalg.norm(got[:, 4:] - g["truth"][:, 4:], axis=1).max() < 0.5  # the two gross fixes did not drag the ring


# ---- 4. covariances ------------------------------------------------------------------------------------------------------------
def cov_anchored(g, pri, e_on, p_on):
    """per node: its component over the enabled edges holds a fixed node or an enabled pose prior"""
    n = len(g["poses"])
    A = sp.coo_matrix((np.ones(int(e_on.sum())), (g["ei"][e_on], g["ej"][e_on])), shape=(n, n))
    _, comp = csgraph.connected_components(A, directed=False)
    has = np.zeros(comp.max() + 1, dtype=bool)
    has[comp[np.asarray(g["fixed"], dtype=bool)]] = True
    has[comp[pri["node"][p_on & (pri["kind"] == P.POSE)]]] = True
    return has[comp]


def cov_reference(g, pri, qa, qb, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0):
    """graph_cov_ref.reference with the priors' blocks in H and the anchoring of rule 11: (cov, status, lambda_min of the
    anchored part of H, J).  The nodes outside the anchored components are left out: no query reaches them and no enabled edge
    joins them to the rest."""
    e_on, p_on = P._masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    _, _, H = P.assemble(g["poses"], g, pri, e_on, p_on, kind, a)
    fixed, anch = np.asarray(g["fixed"], dtype=bool), cov_anchored(g, pri, e_on, p_on)
    keep = np.repeat(anch, 6)
    Hk = H[keep][:, keep].tocsc()
    lu = spla.splu(Hk)
    J = V.jacobian(g, qa, qb)
    st = np.zeros(len(qb), dtype=np.int32)
    cov = np.full((len(qb), 6, 6), np.nan)
    for q, (ka, kb) in enumerate(zip(qa, qb)):
        ends = [kb] + ([ka] if ka >= 0 else [])
        if any(not fixed[k] and not anch[k] for k in ends):
            st[q] = V.UNANCHORED
            continue
        Jk = J[q][:, keep]
        cov[q] = V.symmetrise(Jk @ lu.solve(np.ascontiguousarray(Jk.T)))
    return cov, st, V.lambda_min(Hk), J


def check_covariances(pg, g, pri, qa, qb, e_on=None, p_on=None):
    ref, st_ref, lam, J = cov_reference(g, pri, qa, qb, e_on, p_on)
    got, st, _ = base_ask(pg, qa, qb)
    assert np.array_equal(st, st_ref), (st, st_ref)
    for q in range(len(qb)):
        if st_ref[q] != V.OK:
            assert np.isnan(got[q]).all()
            continue
        scale = np.abs(ref[q]).max()
        if scale == 0.0:
            assert not got[q].any()
            continue
        assert np.array_equal(got[q], got[q].T)
        gap, limit = np.abs(got[q] - ref[q]).max(), V.bound(J[q], COV_TOLERANCE, lam)
        assert gap <= limit, (q, gap, limit)
    return got, st


def base_ask(pg, qa, qb):
    """test_gpu_graph_covariance.ask: relative covariances where qa >= 0, marginals where qa < 0, in the order asked"""
    qa, qb = np.asarray(qa, dtype=np.int32), np.asarray(qb, dtype=np.int32)
    cov, st = np.empty((len(qb), 6, 6)), np.empty(len(qb), dtype=np.int32)
    infos = []
    for mask, call in ((qa >= 0, lambda m: pg.relative_covariances(qa[m], qb[m])), (qa < 0, lambda m: pg.marginals(qb[m]))):
        if mask.any():
            cov[mask], st[mask], info = call(mask)
            infos.append(info)
    return cov, st, infos


@pytest.mark.parametrize("name", ["two_nodes", "triangle", "chain_and_lone_node", "ring65_8_closures"])
def test_covariances_with_a_pose_prior_in_place_of_the_fixed_node(name):
    g, kind, a, qa, qb = V.case(name)
    held = int(np.flatnonzero(g["fixed"])[0])
    g["fixed"][:] = False
    pri = P.make([held], [P.POSE], [g["poses"][held]], [cases.random_spd(np.random.default_rng(80), 1, 1e2, 1e5)[0]])
    qa, qb = np.append(qa, [-1, -1]).astype(np.int32), np.append(qb, [held, qb[0]]).astype(np.int32)
    with build(g, pri) as pg:
        before = pg.poses().tobytes()
        got, st = check_covariances(pg, g, pri, qa, qb)
        assert pg.poses().tobytes() == before
    # the held node's marginal is no longer zero: it is what the prior and the graph know of it
    assert st[-2] == V.OK and np.linalg.eigvalsh(got[-2])[0] > 0


def test_a_component_cut_off_by_its_bridge_is_unanchored_until_the_edge_is_back():
    g = cases.chain(n=9, fixed_at=4, isolated=1)  # edge k joins k and k + 1; node 9 has no edges
    pri = make_priors(g, [7, 8, 8, 9], [P.POSITION] * 4, 81)
    qa = np.array([-1, -1, 2, 7, -1, 6], dtype=np.int32)
    qb = np.array([2, 7, 8, 8, 9, 3], dtype=np.int32)
    e_on = np.ones(8, dtype=bool)
    e_on[6] = False  # the bridge 6 - 7: nodes 7 and 8 keep edge 7 and three position priors, node 9 one position prior
    with build(g, pri, None, e_on) as pg:
        got, st = check_covariances(pg, g, pri, qa, qb, e_on)
        assert list(st) == [V.OK, V.UNANCHORED, V.UNANCHORED, V.UNANCHORED, V.UNANCHORED, V.OK]
        assert np.isnan(got[[1, 2, 3, 4]]).all() and np.isfinite(got[[0, 5]]).all()
        alone, s1, _ = base_ask(pg, qa[:1], qb[:1])
        assert alone.tobytes() == got[:1].tobytes() and s1[0] == V.OK  # rule 7, in the company of unanchored queries
        pg.set_edges_enabled([True], first=6)
        got2, st2 = check_covariances(pg, g, pri, qa, qb)
        assert list(st2) == [V.OK] * 4 + [V.UNANCHORED, V.OK]
        # a weak pose prior anchors what the position priors could not
        weak = P.make([9], [P.POSE], [g["poses"][9]], [np.eye(6) * 1e-2])
        assert pg.add_priors(weak["node"], weak["z"], weak["omega"]) == 4
        both = {k: np.concatenate([pri[k], weak[k]]) for k in pri}
        _, st3 = check_covariances(pg, g, both, qa, qb)
        assert not st3.any()


def test_a_querys_bytes_do_not_depend_on_its_company_with_priors():
    g = cases.ring(closures=8)
    g["fixed"][:] = False
    rng = np.random.default_rng(82)
    kinds = rng.integers(0, 2, size=12)
    kinds[0] = P.POSE  # at least one anchor
    pri = make_priors(g, rng.integers(0, 65, size=12), kinds, 83)
    qa, qb = V.queries(dict(g, fixed=np.arange(65) == 0), seed=7, pairs=7)
    e_on = np.arange(len(g["ei"])) != 10
    with build(g, pri, None, e_on) as pg, build(g, pri, None, e_on) as twin:
        together, st, _ = base_ask(pg, qa, qb)
        assert not st.any()
        for q in range(len(qb)):
            alone, s1, _ = base_ask(pg, qa[q:q + 1], qb[q:q + 1])
            assert alone.tobytes() == together[q].tobytes() and s1[0] == st[q]
        again, _, _ = base_ask(twin, qa[::-1], qb[::-1])
        assert again[::-1].tobytes() == together.tobytes()


# ---- 5. readiness and refusals ---------------------------------------------------------------------------------------------------
def _snapshot(pg):
    c = pg.counts()
    e = pg.errors() if c["edges"] else {"chi2": np.zeros(0), "residual": np.zeros(0), "weight": np.zeros(0), "cost": 0.0}
    p = pg.prior_errors() if c["priors"] else {"chi2": np.zeros(0), "residual": np.zeros(0), "weight": np.zeros(0), "cost": 0.0}
    return (tuple(sorted(c.items())), pg.poses().tobytes() if c["nodes"] else b"", pg.edges_enabled().tobytes(), pg.priors_enabled().tobytes(),
            e["chi2"].tobytes(), e["residual"].tobytes(), e["weight"].tobytes(), e["cost"],
            p["chi2"].tobytes(), p["residual"].tobytes(), p["weight"].tobytes(), p["cost"])


def test_optimize_readiness_with_flags_and_priors():
    L = sicp.lib()
    g = cases.triangle()
    info = sicp.SicpGraphInfo()
    pri = make_priors(g, [0, 2], [P.POSE, P.POSITION], 90)
    with build(g, pri, base.opt_params()) as pg:
        pg.set_edges_enabled([False] * 3)
        pg.set_priors_enabled([False] * 2)
        before = _snapshot(pg)
        assert L.sicp_graph_optimize(pg._g, C.byref(info)) == sicp.ERR_NOT_READY
        assert "no edge or prior that is enabled" in L.sicp_graph_last_error(pg._g).decode()
        assert _snapshot(pg) == before
        pg.set_edges_enabled([True] * 3)
        pg.set_fixed([False], first=1)
        before = _snapshot(pg)
        assert L.sicp_graph_optimize(pg._g, C.byref(info)) == sicp.ERR_NOT_READY  # edges, no fixed node, no enabled prior
        assert "no fixed node" in L.sicp_graph_last_error(pg._g).decode()
        assert _snapshot(pg) == before
        pg.set_priors_enabled([True], first=1)  # a position prior alone is enough for optimize
        assert pg.optimize()["accepted_steps"] >= 1
    with sicp.PoseGraph(0, base.opt_params()) as pg:  # priors only
        pg.add_nodes(g["poses"])
        assert L.sicp_graph_optimize(pg._g, C.byref(info)) == sicp.ERR_NOT_READY
        P.add_to(pg, make_priors(g, [0, 1, 1], [P.POSE, P.POSE, P.POSITION], 91))
        start = pg.poses()
        out = pg.optimize()
        got = pg.poses()
        assert out["accepted_steps"] >= 1 and out["final_cost"] < out["initial_cost"]
        assert np.array_equal(got[2], start[2]) and not np.array_equal(got[0], start[0])  # node 2 has nothing: its bytes stay
        assert pg.counts() == dict(nodes=3, edges=0, edges_enabled=0, priors=3, priors_enabled=3)
        assert pg.errors()["cost"] == pg.prior_errors()["cost"] == pg.linearize()["cost"]
        pg.clear()
        assert pg.counts() == dict(nodes=0, edges=0, edges_enabled=0, priors=0, priors_enabled=0) and pg.size() == (0, 0)


def test_refusals_leave_the_graph_as_it_was():
    L = sicp.lib()
    g = cases.triangle()
    pri = make_priors(g, [0, 2], [P.POSE, P.POSITION], 92)
    dp, ip, bp, ptr = sicp._dp, sicp._ip, sicp._bp, sicp._ptr
    with build(g, pri, None, [True, False, True], [True, False]) as pg:
        before = _snapshot(pg)
        G = pg._g
        first = C.c_int32(-7)
        node0 = np.array([0], np.int32)
        ok_z, ok_om = np.array([[0, 0, 0, 1, 1, 2, 3.0]]), np.eye(6)[None].copy()
        ok_p, ok_om3 = np.array([[1, 2, 3.0]]), np.eye(3)[None].copy()

        def refused(st, *needles):
            text = L.sicp_graph_last_error(G).decode()
            assert st == sicp.ERR_INVALID_ARGUMENT, (st, text)
            for n in needles:
                assert n in text, text
            assert _snapshot(pg) == before and first.value == -7

        def priors(kind, node, z, om, m=None):
            node = np.asarray(node, np.int32)
            z, om = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(om, dtype=np.float64)
            return L.sicp_graph_add_priors(G, kind, len(node) if m is None else m, ptr(node, ip), ptr(z, dp), ptr(om, dp), C.byref(first))

        refused(priors(2, node0, ok_z, ok_om), "kind")
        refused(priors(-1, node0, ok_z, ok_om), "kind")
        refused(priors(P.POSE, node0, ok_z, ok_om, m=0), "m must be >= 1")
        refused(L.sicp_graph_add_priors(G, P.POSE, 1, None, ptr(ok_z, dp), ptr(ok_om, dp), C.byref(first)), "NULL")
        refused(L.sicp_graph_add_priors(G, P.POSE, 1, ptr(node0, ip), None, ptr(ok_om, dp), C.byref(first)), "NULL")
        refused(L.sicp_graph_add_priors(G, P.POSITION, 1, ptr(node0, ip), ptr(ok_p, dp), None, C.byref(first)), "NULL")
        refused(priors(P.POSE, [0, 3], np.repeat(ok_z, 2, 0), np.repeat(ok_om, 2, 0)), "prior 1", "outside")
        refused(priors(P.POSITION, [-1], ok_p, ok_om3), "prior 0", "outside")
        z = ok_z.copy(); z[0, 5] = np.nan
        refused(priors(P.POSE, node0, z, ok_om), "prior 0", "not finite")
        z = ok_z.copy(); z[0, 3] = 0.99
        refused(priors(P.POSE, node0, z, ok_om), "prior 0", "quaternion")
        p = np.repeat(ok_p, 2, 0); p[1, 2] = np.inf
        refused(priors(P.POSITION, [0, 1], p, np.repeat(ok_om3, 2, 0)), "prior 1", "not finite")
        for kind, zz, om in ((P.POSE, ok_z, ok_om), (P.POSITION, ok_p, ok_om3)):
            bad = om.copy(); bad[0, 1, 2] = np.inf
            refused(priors(kind, node0, zz, bad), "prior 0", "not finite")
            bad = om.copy(); bad[0, 1, 2] = 1e-6
            refused(priors(kind, node0, zz, bad), "prior 0", "not symmetric")
            bad = om.copy(); bad[0, 2, 2] = -1.0
            refused(priors(kind, node0, zz, bad), "prior 0", "positive definite")
            bad = np.ones_like(om)  # singular
            refused(priors(kind, node0, zz, bad), "prior 0", "positive definite")
        # flags: ranges and NULLs
        flags, out = np.ones(4, np.uint8), np.full(4, 9, np.uint8)
        for setter, getter, have in ((L.sicp_graph_set_edges_enabled, L.sicp_graph_get_edges_enabled, 3),
                                     (L.sicp_graph_set_priors_enabled, L.sicp_graph_get_priors_enabled, 2)):
            refused(setter(G, have - 1, 2, ptr(flags, bp)), "beyond")
            refused(setter(G, -1, 1, ptr(flags, bp)), "first")
            refused(setter(G, 0, 0, ptr(flags, bp)), "count")
            refused(setter(G, 0, 1, None), "NULL")
            refused(getter(G, have - 1, 2, ptr(out, bp)), "beyond")
            refused(getter(G, 0, 0, ptr(out, bp)), "count")
            refused(getter(G, 0, 1, None), "NULL")
        assert np.all(out == 9)
        refused(L.sicp_graph_prior_errors(G, None, None, None, None), "NULL")
        # sicp_graph_counts: every output is nullable
        n_pri = C.c_int64(-1)
        assert L.sicp_graph_counts(G, None, None, None, C.byref(n_pri), None) == sicp.OK and n_pri.value == 2
        assert L.sicp_graph_counts(G, None, None, None, None, None) == sicp.OK
        # accepted: an asymmetry below 1e-9 of the largest entry (the mean of the halves is stored), a quaternion within 1e-6
        om = ok_om3.copy() * 100.0; om[0, 0, 1] = 2e-8
        first.value = -1
        assert priors(P.POSITION, [1], ok_p, om) == sicp.OK and first.value == 2
        om_sym = om[0].copy(); om_sym[0, 1] = om_sym[1, 0] = 1e-8
        r = g["poses"][1, 4:] - ok_p[0]
        e = pg.prior_errors()
        assert abs(e["chi2"][2] - r @ om_sym @ r) <= 1e-12 * e["chi2"][2] and not e["residual"][2, 3:].any()
        zq = ok_z.copy(); zq[0, 3] = 1 + 5e-7
        assert priors(P.POSE, [1], zq, ok_om) == sicp.OK and first.value == 3
        zn = zq.copy(); zn[0, :4] /= np.linalg.norm(zn[0, :4])
        r = P.pose_residual(g["poses"][[1]], zn)[0]
        e = pg.prior_errors()
        assert abs(e["chi2"][3] - r @ r) <= 1e-12 * e["chi2"][3]
        assert pg.counts() == dict(nodes=3, edges=3, edges_enabled=2, priors=4, priors_enabled=3)


def test_a_memory_limit_refuses_add_priors_and_the_graph_optimises_as_its_twin():
    """test_gpu_pose_graph's arena-limit test for sicp_graph_add_priors: with the limit at one byte the arena takes no new slab;
    filler graphs ask for the blocks the large add_priors will ask for until one is refused; from there the graph's own call must
    be refused, the graph unchanged, and its optimisation the twin's byte for byte."""
    L = sicp.lib()
    g = cases.ring(65, 4, seed=41)
    pri = mixed(g, 5, 93)
    m = 200_001
    node = np.zeros(m, np.int32)
    z = np.tile(np.array([0, 0, 0, 1, 0, 0, 0.0]), (m, 1))
    om = np.tile(np.eye(6), (m, 1, 1))
    args = (P.POSE, m, sicp._ptr(node, sicp._ip), sicp._ptr(z, sicp._dp), sicp._ptr(om, sicp._dp), None)
    fillers = []
    with build(g, pri, base.opt_params()) as pg, build(g, pri, base.opt_params()) as twin:
        before = _snapshot(pg)
        try:
            fillers = [sicp.PoseGraph(0) for _ in range(64)]
            for f in fillers:
                f.add_nodes(g["poses"][:2])
            sicp.set_memory_limit(0, 1)
            hit = False
            for f in fillers:
                st = L.sicp_graph_add_priors(f._g, *args)
                if st == sicp.ERR_OUT_OF_MEMORY:
                    hit = True
                    assert f.counts()["priors"] == 0
                    break
                assert st == sicp.OK
            assert hit, "64 fillers of 70 MB found room: the arena holds more free space than this test allows for"
            st = L.sicp_graph_add_priors(pg._g, *args)
            text = L.sicp_graph_last_error(pg._g).decode()
        finally:
            sicp.set_memory_limit(0, 0)
            for f in fillers:
                f.close()
        assert st == sicp.ERR_OUT_OF_MEMORY
        assert text.startswith("sicp_graph_add_priors: ") and "out of memory" in text and text.endswith("the graph is unchanged")
        assert _snapshot(pg) == before
        a, b = pg.optimize(), twin.optimize()
        assert base._info_bytes(a) == base._info_bytes(b) and pg.poses().tobytes() == twin.poses().tobytes()
        assert a["accepted_steps"] >= 1


# ---- 6. the bytes of a graph without priors ---------------------------------------------------------------------------------------
PARENT_CASES = {"ring65": lambda: cases.ring(65, 1), "hub": lambda: cases.hub()}


def parent_byte_hashes(name):
    """sha256 of what a graph without priors and with every edge enabled returns, through calls that the build before priors had:
    linearize() and marginals at the initial poses, then optimize()'s info and poses"""
    g = PARENT_CASES[name]()
    sha = lambda b: hashlib.sha256(b).hexdigest()
    nodes = np.arange(len(g["poses"]), dtype=np.int32)[:: max(1, len(g["poses"]) // 8)]
    with base.build(g, base.opt_params()) as pg:
        lin = pg.linearize()
        cov, st, _ = pg.marginals(nodes)
        info = pg.optimize()
        poses = pg.poses()
    return {"linearize": sha(lin["gradient"].tobytes() + lin["diag_blocks"].tobytes() + np.float64(lin["cost"]).tobytes()),
            "marginals": sha(cov.tobytes() + st.tobytes()), "info": sha(repr(base._info_bytes(info)).encode()), "poses": sha(poses.tobytes())}


@pytest.mark.parametrize("name", list(PARENT_CASES))
def test_a_graph_without_priors_returns_the_bytes_of_the_build_before_priors(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    assert parent_byte_hashes(name) == want


# ---- 7. ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_constants_of_the_binding_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sicp.h")).read()
    assert f"SICP_GRAPH_PRIOR_POSE = {sicp.PRIOR_POSE}" in text and f"SICP_GRAPH_PRIOR_POSITION = {sicp.PRIOR_POSITION}" in text
    assert (sicp.PRIOR_POSE, sicp.PRIOR_POSITION) == (P.POSE, P.POSITION)
