"""The conditions that tests/test_gpu_pose_graph_steps.py relies on, asserted from the restatement alone
(tests/pose_graph_step_ref.py on the cases of tests/pose_graph_step_cases.py).  No GPU.  A case that misses its condition is
replaced in pose_graph_step_cases.py, never excused here."""
import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_prior_ref as P
import pose_graph_ref as R
import pose_graph_step_cases as SC
import pose_graph_step_ref as S

TOL = cases.header_tolerance()[1]
ZERO_TOL = dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)


# ---- the restatement against the two references it stands on -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain", "hub", "prior_ring"])
@pytest.mark.parametrize("loss", list(SC.LOSSES))
def test_linearise_is_the_prior_references_assemble(name, loss):
    c, l = SC.get(name, loss), SC.lin(name, loss)
    cost, g, H = P.assemble(c["g"]["poses"], c["g"], c["pri"], c["e_on"], c["p_on"], c["kind"], c["a"])
    assert abs(cost - l["cost"]) <= 1e-13 * cost
    assert np.abs(g - l["g"]).max() <= 1e-12 * np.abs(g).max()
    assert abs(H - l["H"]).max() <= 1e-12 * abs(H).max()
    assert S.cost(c, c["g"]["poses"]) == pytest.approx(cost, rel=1e-13)


def test_fixed_and_lone_nodes_follow_the_header():
    l = SC.lin("chain")  # node 4 fixed, node 9 without edges
    H = l["H"].toarray()
    assert np.array_equal(H[24:30], np.eye(60)[24:30]) and np.array_equal(H[:, 24:30], np.eye(60)[:, 24:30])
    assert not H[54:].any() and not H[:, 54:].any() and not l["g"][24:30].any() and not l["g"][54:].any()
    A, _, _ = S.damped_system(l, 1e4, 1e-6, 1e32)
    assert np.array_equal(A.toarray()[54:, 54:], np.eye(6) * (1e-6 / 1e4))  # the clip's lower end carries a lone node
    assert np.allclose(A.diagonal()[:54], l["H"].diagonal()[:54] * (1 + 1e-4), rtol=1e-15)


def test_longdouble_and_float64_linearisations_agree():
    c = SC.get("step_control")
    a, b = S.linearise(c), S.linearise(c, dtype=np.longdouble)
    assert b["H"].dtype == np.longdouble and np.abs(a["H"].toarray() - b["H"]).max() <= 1e-12 * np.abs(b["H"]).max()
    assert abs(a["cost"] - b["cost"]) <= 1e-13 * a["cost"]


def test_pcg_converges_to_the_direct_solve():
    for name, loss, radius in (("ring65", "none", 1e4), ("hub", "cauchy", 1.0), ("prior_ring", "none", 1e16)):
        A, run = SC.solve(name, loss, radius)
        direct = S.lm_step(SC.get(name, loss), SC.lin(name, loss), radius)["delta"]
        assert run["state"] == "converged" and np.linalg.norm(run["x"] - direct) <= 1e-6 * np.linalg.norm(direct)


def test_the_default_eta_hides_the_step():
    """the reason for TIGHT_ETA: at cg_eta = 0.1 the conjugate gradients stop far from the direct solve's step"""
    direct = S.lm_step(SC.get("ring65"), SC.lin("ring65"), 1e4)["delta"]
    _, run = SC.solve("ring65", "none", 1e4, eta=0.1)
    assert run["iterations"] < 20 and np.linalg.norm(run["x"] - direct) > 0.5 * np.linalg.norm(direct)


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loss,radius", SC.step_cases(), ids=lambda v: str(v))
def test_a_the_restated_pcg_meets_the_bound_with_factor_one(name, loss, radius):
    A, run = SC.solve(name, loss, radius)
    res, bound = SC.residual_bound(A, SC.lin(name, loss)["g"], run["x"], SC.TIGHT_ETA, TOL, factor=1.0)
    assert run["state"] == "converged" and 2 * run["iterations"] <= 5000
    assert SC.cg_budget(name, loss, radius) >= 2 * run["iterations"]
    assert res <= bound, (res, bound)
    if not name.startswith("banded"):  # the step survives being applied to the poses and read off them again
        l = SC.lin(name, loss)
        seen = S.step_of(l["poses"], R.retract(l["poses"], l["fixed"], run["x"]))
        res, bound = SC.residual_bound(A, l["g"], seen, SC.TIGHT_ETA, TOL)
        assert res <= 0.8 * bound, (res, bound)
    outcome, rho = SC.first_step(name, loss, radius)
    assert abs(rho - 1e-3) >= 0.05  # the library's own step, 1e-10 away, is accepted or rejected as this one
    assert outcome == "accepted" or name == "step_control"


def test_a_the_cases_reach_the_paths_they_are_for():
    g = SC.get("hub")["g"]
    assert (g["ei"] > g["ej"]).sum() >= 100 and (g["ei"] < g["ej"]).sum() >= 100  # both B and B^T from node 0's side
    assert np.bincount(np.concatenate([g["ei"], g["ej"]]))[0] == 300
    blocks = lambda n: (n + 255) // 256
    assert blocks(6 * 42) == 1 and blocks(6 * 43) == 2 and blocks(255) == blocks(256) == 1 and blocks(257) == 2
    for n, rows, nodes, cost in ((10923, 257, 43, 86), (65537, 1537, 257, 512)):
        m = len(SC.get(f"banded_{n}")["g"]["ei"])
        assert (blocks(6 * n), blocks(n), blocks(m)) == (rows, nodes, cost)
    c = SC.get("prior_ring")
    assert set(c["pri"]["kind"][c["p_on"]]) == {P.POSE, P.POSITION} and not c["e_on"].all() and not c["p_on"].all()
    lone = SC.lin("chain")["H"].diagonal() == 0
    assert lone.sum() == 6 and SC.get("chain")["g"]["fixed"].sum() == 1


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clip", SC.CLIP_CASES)
def test_b_the_clip_is_engaged_and_changes_the_step(name, clip):
    l, p = SC.lin(name), SC.CLIPS[clip]
    lo, hi = p.get("min_lm_diagonal", 1e-6), p.get("max_lm_diagonal", 1e32)
    d = l["H"].diagonal()
    assert (lo > d.max()) if clip == "lo_above" else (hi < d[d > 0].min() and lo < hi)
    A, run = SC.solve(name, "none", SC.CLIP_RADIUS, lo, hi)
    res, bound = SC.residual_bound(A, l["g"], run["x"], SC.TIGHT_ETA, TOL, factor=1.0)
    assert run["state"] == "converged" and res <= bound
    unclipped = S.lm_step(SC.get(name), l, SC.CLIP_RADIUS)["delta"]
    res, bound = SC.residual_bound(A, l["g"], unclipped, SC.TIGHT_ETA, TOL)
    assert res > 100 * bound
    if (name, clip) == ("ring65", "lo_above"):
        clipped = S.lm_step(SC.get(name), l, SC.CLIP_RADIUS, lo, hi)["delta"]
        assert np.linalg.norm(clipped) == pytest.approx(4.68, abs=0.01) and np.linalg.norm(unclipped) == pytest.approx(12.2, abs=0.1)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def test_c_enough_stop_cases_meet_the_condition():
    found = SC.stop_cases()
    assert len(found) >= 6 and max(k for *_, k in found) >= 8 and {e for _, _, e, _ in found} == {0.1, 1e-3, 1e-6}
    for name, radius, eta, k in found:
        ratios = SC.solve(name, "none", radius, eta=eta)[1]["ratios"]
        assert len(ratios) == k and ratios[k - 1] <= eta / 2 and (k == 1 or ratios[k - 2] >= 2 * eta)


def test_c_the_iterates_are_known_to_a_noise_far_below_their_differences():
    for name, radius, eta, k_ref in SC.stop_cases():
        for k, noise, x in SC.truncated(name, radius, eta, k_ref):
            assert noise < 1e-9, (name, radius, k, noise)
            nxt = SC.solve(name, "none", radius, eta=1e-300, keep=(k + 1,))[1]["iterates"][k + 1]
            assert np.linalg.norm(nxt - x) > 1e3 * 32 * noise * np.linalg.norm(x)  # one iteration more or less is seen


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
def test_d_the_gain_ratios_of_step_control():
    c, l = SC.get("step_control"), SC.lin("step_control")
    for radius, rho in SC.GAIN_TABLE.items():
        assert float(S.lm_step(c, l, radius)["rho"]) == pytest.approx(rho, abs=0.02)
    assert float(S.lm_step(c, l, SC.TRIPLE_RADIUS)["rho"]) >= 0.95
    assert S.new_radius(SC.TRIPLE_RADIUS, 0.937) == 3 * SC.TRIPLE_RADIUS  # the factor is exactly 1/3 from there on
    for radius in list(SC.GAIN_TABLE)[:3]:
        s = S.lm_step(c, l, radius)
        assert SC.radius_noise(c, radius, s["delta"])[1] < 1e-10


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SC.LOOPS))
def test_e_the_reference_trace(which):
    records, K = SC.loop_trace(which)
    mrd = SC.LOOPS[which].get("min_relative_decrease", 1e-3)
    assert len(records) == K and all(abs(r["rho"] - mrd) >= 0.05 for r in records)
    o = "".join(r["outcome"][0] for r in records)
    j = len(o) - len(o.lstrip("r"))
    assert j >= 3 and [r["radius_after"] for r in records[:j]] == [1e16 / 2.0 ** (i * (i + 1) // 2) for i in range(1, j + 1)]
    if which == "rejections_then_three_accepted":
        assert o == "r" * j + "aaa"
    else:
        assert o.endswith("ar") and "ar" not in o[:-2] and records[-1]["radius_after"] == records[-1]["radius"] / 2


# ---- (f) ------------------------------------------------------------------------------------------------------------------------
def test_f_the_terminations_of_the_reference():
    c = SC.get("step_control")
    _, end = S.trace(c, dict(ZERO_TOL, initial_radius=123.0), 0)
    assert (end["termination"], end["iterations"], end["radius"]) == ("max_iterations", 0, 123.0)
    g = SC.at_truth()
    assert np.abs(S.linearise(S.case(g))["g"]).max() <= 1e-9
    assert S.trace(S.case(g), dict(gradient_tolerance=1e-8))[1]["termination"] == "gradient"
    _, end = S.trace(SC.get("ring65"), dict(ZERO_TOL, function_tolerance=1.0))
    assert (end["termination"], end["accepted_steps"], end["iterations"]) == ("function", 1, 1)
    _, end = S.trace(SC.get("ring65"), dict(ZERO_TOL, parameter_tolerance=1e3))
    assert (end["termination"], end["accepted_steps"], end["iterations"]) == ("parameter", 0, 1)
    _, end = S.trace(c, dict(ZERO_TOL, initial_radius=1000.0, min_radius=1000.0))
    assert (end["termination"], end["iterations"], end["rejected_steps"], end["radius"]) == ("min_radius", 1, 1, 500.0)


def test_f_the_invalid_graph_is_accepted_by_rule_4_and_overflows():
    g = SC.invalid_graph()
    assert np.isfinite(g["poses"]).all() and np.isfinite(g["z"]).all() and np.isfinite(g["omega"]).all()
    for q in (g["poses"], g["z"]):
        assert np.abs(np.linalg.norm(q[:, :4], axis=1) - 1).max() <= 1e-6
    assert np.array_equal(g["omega"], np.swapaxes(g["omega"], 1, 2)) and np.linalg.eigvalsh(g["omega"]).min() > 0
    assert (g["ei"] != g["ej"]).all() and g["fixed"].any()
    with np.errstate(all="ignore"):
        assert not np.isfinite(S.cost(S.case(g), g["poses"]))
        for limit, radius in ((5, 1e4 / 1024), (2, 1e4 / 2)):
            _, end = S.trace(S.case(g), dict(ZERO_TOL, max_consecutive_invalid_steps=limit))
            assert (end["termination"], end["invalid_steps"], end["iterations"], end["accepted_steps"]) == ("invalid_steps", limit, limit, 0)
            assert end["radius"] == radius
