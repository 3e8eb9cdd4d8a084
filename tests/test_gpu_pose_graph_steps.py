"""GPU tests of what sicp_graph_optimize does after the linearisation, step by step: the linear solve (the matrix-vector
products with their off-diagonal blocks, the preconditioner, the damping and its clip, the sums over more than 256 partials),
the stopping rule and the iteration counts, the model decrease, the radius update, the loop's bookkeeping and every
termination.  The reference is tests/pose_graph_step_ref.py on the cases of tests/pose_graph_step_cases.py; every condition
these tests rely on is asserted from the reference alone in tests/test_pose_graph_step_cpu.py.

The step a call has taken is read off the poses: delta = log(T_before^-1 T_after) per node.

Tolerances.  (a), (b): |-g - A_ref delta| <= 2 eta |g| + tol | |A_ref| |delta| |, tol = header_tolerance() (the kernels' own
stopping rule evaluated by the reference's matrix; 2 for the drift of the recursive residual).  (c), (d): 32 x the distance of
the restatement in float64 from the restatement in np.longdouble.  Everything else is exact.  Each test prints its figures
(profiles/graph_steps/figures.txt)."""
import functools
import importlib
import time

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_prior_ref as P
import pose_graph_ref as R
import pose_graph_step_cases as SC
import pose_graph_step_ref as S
import test_gpu_pose_graph as base

sicp = importlib.import_module("semantic-icp_amd")
pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
ZERO = dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)
FIELDS = ("iterations", "accepted_steps", "rejected_steps", "invalid_steps", "cg_iterations", "termination_name", "initial_cost",
          "final_cost", "gradient_max_norm", "radius")


@functools.lru_cache(maxsize=1)
def tolerance():
    return cases.header_tolerance()[1]


def build(c, **params):
    g, pri = c["g"], c["pri"]
    pg = base.build(g, sicp.default_graph_params(loss=c["kind"], cauchy_a=c["a"], **params))
    if len(pri["node"]):
        assert P.add_to(pg, pri) == 0
    if c["e_on"] is not None:
        pg.set_edges_enabled(c["e_on"])
    if c["p_on"] is not None:
        pg.set_priors_enabled(c["p_on"])
    return pg


def run(c, **params):
    """(poses after, info, max |g| of linearize() at the poses after, poses before) of one optimize() on a fresh graph.  "Before"
    is what the graph stored (quaternions normalised: an ulp off the input here and there)."""
    with build(c, **params) as pg:
        before = pg.poses()
        info = pg.optimize()
        got = pg.poses()
        gmax = np.abs(pg.linearize()["gradient"]).max()
    assert set(FIELDS) <= set(info)
    return got, info, gmax, before


def one_step(c, radius, eta=SC.TIGHT_ETA, max_cg=500, **more):
    return run(c, **dict(ZERO, max_iterations=1, initial_radius=radius, cg_eta=eta, max_cg_iterations=max_cg, **more))


def expect(info, **fields):
    """every field of the info, exactly"""
    assert set(fields) == set(FIELDS), set(FIELDS) ^ set(fields)
    for k, v in fields.items():
        if callable(v):
            assert v(info[k]), (k, info[k], info)
        else:
            assert info[k] == v, (k, info[k], v, info)


def check_step(name, loss, radius, before, got, info, lo=1e-6, hi=1e32, eta=SC.TIGHT_ETA):
    """(a): the step that was taken solves the reference's damped system"""
    c, l = SC.get(name, loss), SC.lin(name, loss)
    delta = S.step_of(before, got)
    res, bound = SC.residual_bound(SC.system(name, loss, radius, lo, hi), l["g"], delta, eta, tolerance())
    print(f"(a) {name} {loss} r={radius:g} lo={lo:g} hi={hi:g}: |-g - A delta| = {res:.3e}, bound {bound:.3e}, ratio {res / bound:.3f}; "
          f"cg_iterations {info['cg_iterations']}, |delta| {np.linalg.norm(delta):.3e}")
    assert np.linalg.norm(delta) > 0 and res <= bound, (res, bound)
    still = l["fixed"] | (l["H"].diagonal().reshape(-1, 6) == 0).all(axis=1)
    assert got[still].tobytes() == before[still].tobytes()  # fixed and lone nodes keep their bytes
    return delta


# ---- (a) the step solves the reference system -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,loss,radius", SC.step_cases(), ids=lambda v: str(v))
def test_a_the_step_solves_the_reference_system(name, loss, radius):
    start = time.perf_counter()
    c = SC.get(name, loss)
    SC.system(name, loss, radius)  # (the reference's share of the time: the graph, its linearisation and the damped matrix)
    built = time.perf_counter()
    got, info, _, before = one_step(c, radius, max_cg=SC.cg_budget(name, loss, radius))
    ran = time.perf_counter()
    assert info["iterations"] == 1 and info["accepted_steps"] + info["rejected_steps"] == 1 and info["invalid_steps"] == 0
    assert 1 <= info["cg_iterations"] < SC.cg_budget(name, loss, radius)
    outcome = "accepted" if name.startswith("banded") else SC.first_step(name, loss, radius)[0]
    if outcome == "rejected":  # (step_control at the large radii: the step cannot be seen, its rejection can)
        print(f"(a) {name} {loss} r={radius:g}: rejected, as the reference's (rho {SC.first_step(name, loss, radius)[1]:.3f})")
        assert info["rejected_steps"] == 1 and got.tobytes() == before.tobytes()
        return
    assert info["accepted_steps"] == 1
    check_step(name, loss, radius, before, got, info)
    end = time.perf_counter()
    print(f"(a) {name} {loss} r={radius:g}: {end - start:.2f} s, of which the CPU reference {built - start + end - ran:.2f} s "
          f"(shared with the other radii of the case) and the library with its upload {ran - built:.2f} s")


# ---- (b) the clip of the damping diagonal ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,clip", SC.CLIP_CASES)
def test_b_clipped_damping(name, clip):
    p = SC.CLIPS[clip]
    lo, hi = p.get("min_lm_diagonal", 1e-6), p.get("max_lm_diagonal", 1e32)
    got, info, _, before = one_step(SC.get(name), SC.CLIP_RADIUS, max_cg=SC.cg_budget(name, "none", SC.CLIP_RADIUS, lo, hi), **p)
    assert info["iterations"] == 1 and info["accepted_steps"] == 1
    check_step(name, "none", SC.CLIP_RADIUS, before, got, info, lo, hi)


# ---- (c) iteration counts and the stopping rule ---------------------------------------------------------------------------------
def _bytes(got, info):
    return got.tobytes(), base._info_bytes(info)


@pytest.mark.parametrize("case", SC.stop_cases(), ids=lambda v: f"{v[0]}-r{v[1]:g}-eta{v[2]:g}-k{v[3]}")
def test_c_iteration_counts_and_the_stopping_rule(case):
    name, radius, eta, k_ref = case
    c, l = SC.get(name), SC.lin(name)
    ended = [one_step(c, radius, eta, cg_check_every=every, min_relative_decrease=0.0) for every in (1, 8, 64)]
    print(f"(c) {name} r={radius:g} eta={eta:g}: k_ref {k_ref}, cg_iterations {[i['cg_iterations'] for _, i, _, _ in ended]}")
    for got, info, _, _ in ended:
        assert info["cg_iterations"] == k_ref
        assert _bytes(got, info) == _bytes(*ended[0][:2]), "a solve that ends on eta must not depend on cg_check_every"
    for k, noise, x_k in SC.truncated(name, radius, eta, k_ref):
        cut = [one_step(c, radius, eta, max_cg=k, cg_check_every=every, min_relative_decrease=0.0) for every in (1, 8, k + 3)]
        for got, info, _, _ in cut:
            assert info["cg_iterations"] == k and _bytes(got, info) == _bytes(*cut[0][:2])
        assert cut[0][1]["accepted_steps"] == 1, "the truncated step was not accepted: it cannot be read off the poses"
        delta = S.step_of(cut[0][3], cut[0][0])
        gap = np.linalg.norm(delta - x_k) / np.linalg.norm(x_k)
        print(f"(c) {name} r={radius:g} eta={eta:g} max_cg_iterations={k}: |delta - x_k| / |x_k| = {gap:.3e}, noise {noise:.3e}, "
              f"tolerance {32 * noise:.3e}")
        assert gap <= 32 * noise


# ---- (d) the model decrease and the radius update -------------------------------------------------------------------------------
def _restated_cost_gap(c, got):
    """|cost - restated cost| bound of check_linearisation at the poses `got` (a graph without priors)"""
    g = c["g"]
    E = R.edges(got, g["ei"], g["ej"], g["z"], g["omega"], c["kind"], c["a"])
    F = cases.floors(got[g["ei"]], got[g["ej"]], g["z"], g["omega"])
    scale = 0.5 * float(base.block_scale(E["rho"], F["rho"]).sum())
    return 0.5 * float(E["rho"].sum()), (tolerance() + len(g["ei"]) * EPS) * scale


@pytest.mark.parametrize("radius", [r for r, rho in SC.GAIN_TABLE.items() if rho > 0])
def test_d_an_accepted_step_and_its_radius(radius):
    c, l = SC.get("step_control"), SC.lin("step_control")
    got, info, gmax, before = one_step(c, radius)
    cost0, bound0 = _restated_cost_gap(c, l["poses"])
    delta = S.step_of(before, got)
    want, noise, rho = SC.radius_noise(c, radius, delta)
    cost, bound = _restated_cost_gap(c, got)
    print(f"(d) step_control r={radius:g}: rho of the library's step {rho:.6f} (table {SC.GAIN_TABLE[radius]}), radius {info['radius']!r}, "
          f"restated {want!r}, relative gap {abs(info['radius'] - want) / want:.3e}, noise {noise:.3e}, tolerance {32 * noise:.3e}; "
          f"final_cost {info['final_cost']!r}, restated {cost!r}, bound {bound:.3e}")
    assert abs(rho - SC.GAIN_TABLE[radius]) <= 0.02
    assert abs(info["final_cost"] - cost) <= bound
    assert abs(info["radius"] - want) <= 32 * noise * want
    expect(info, iterations=1, accepted_steps=1, rejected_steps=0, invalid_steps=0, cg_iterations=lambda k: 1 <= k < 500,
           termination_name="max_iterations", initial_cost=lambda v: abs(v - cost0) <= bound0, final_cost=lambda v: v < info["initial_cost"],
           gradient_max_norm=gmax, radius=lambda v: v > 0)


def test_d_a_rejected_step():
    c, l = SC.get("step_control"), SC.lin("step_control")
    got, info, gmax, before = one_step(c, 1000.0)
    cost0, bound0 = _restated_cost_gap(c, l["poses"])
    assert got.tobytes() == before.tobytes()
    assert np.float64(info["final_cost"]).tobytes() == np.float64(info["initial_cost"]).tobytes()
    expect(info, iterations=1, accepted_steps=0, rejected_steps=1, invalid_steps=0, cg_iterations=lambda k: 1 <= k < 500,
           termination_name="max_iterations", initial_cost=lambda v: abs(v - cost0) <= bound0, final_cost=info["initial_cost"],
           gradient_max_norm=gmax, radius=500.0)


def test_d_a_gain_ratio_above_095_triples_the_radius():
    got, info, _, before = one_step(SC.get("step_control"), SC.TRIPLE_RADIUS)
    rho = SC.radius_noise(SC.get("step_control"), SC.TRIPLE_RADIUS, S.step_of(before, got))[2]
    print(f"(d) step_control r={SC.TRIPLE_RADIUS:g}: rho {rho:.6f}, radius {info['radius']!r}")
    assert rho >= 0.95 and info["accepted_steps"] == 1 and info["radius"] == 3 * SC.TRIPLE_RADIUS


# ---- (e) the loop's bookkeeping over several iterations -------------------------------------------------------------------------
@pytest.mark.parametrize("which", list(SC.LOOPS))
def test_e_the_loops_bookkeeping(which):
    c = SC.get("step_control")
    records, K = SC.loop_trace(which)
    params = dict(ZERO, cg_eta=SC.TIGHT_ETA, **SC.LOOPS[which])
    prev_poses, prev_radius = None, params["initial_radius"]
    rejections = 0
    for k in range(K + 1):
        got, info, gmax, before = run(c, max_iterations=k, **params)
        done = records[:k]
        count = lambda what: sum(r["outcome"] == what for r in done)
        print(f"(e) {which} max_iterations={k}: {info['accepted_steps']} accepted, {info['rejected_steps']} rejected, radius {info['radius']!r}"
              + (f", the trace's rho {done[-1]['rho']:.4f}" if done else ""))
        expect(info, iterations=k, accepted_steps=count("accepted"), rejected_steps=count("rejected"), invalid_steps=0,
               cg_iterations=lambda v: v >= k, termination_name="max_iterations", initial_cost=lambda v: v > 0,
               final_cost=lambda v: v <= info["initial_cost"], gradient_max_norm=gmax, radius=lambda v: v > 0)
        if k == 0:
            assert info["radius"] == prev_radius and got.tobytes() == before.tobytes()
            prev_poses = got
            continue
        rec = done[-1]
        if rec["outcome"] == "rejected":
            rejections += 1
            assert got.tobytes() == prev_poses.tobytes()
            # j rejections in a row divide by 2^(j (j + 1) / 2); after an acceptance the count starts again
            assert info["radius"] == prev_radius / 2.0 ** rejections, (info["radius"], prev_radius, rejections)
            if k == rejections:
                assert info["radius"] == 1e16 / 2.0 ** (rejections * (rejections + 1) // 2)
        else:
            rejections = 0
            want, noise, rho = SC.radius_noise(c, prev_radius, S.step_of(prev_poses, got), poses=prev_poses)
            # the same path as the trace's: its rho is 0.05 from the threshold, the library's step 1e-10 |g| from the direct solve
            assert abs(rho - rec["rho"]) <= 1e-3, (rho, rec["rho"])
            if rho >= 0.95:
                assert info["radius"] == 3 * prev_radius
            else:
                assert abs(info["radius"] - want) <= 32 * noise * want, (info["radius"], want, noise)
        prev_poses, prev_radius = got, info["radius"]


# ---- (f) every termination once -------------------------------------------------------------------------------------------------
def test_f_max_iterations_zero():
    c = SC.get("ring65")
    with build(c, **dict(ZERO, max_iterations=0, initial_radius=123.0)) as pg:
        cost = pg.linearize()["cost"]
    got, info, gmax, before = run(c, **dict(ZERO, max_iterations=0, initial_radius=123.0))
    assert got.tobytes() == before.tobytes()
    expect(info, iterations=0, accepted_steps=0, rejected_steps=0, invalid_steps=0, cg_iterations=0, termination_name="max_iterations",
           initial_cost=cost, final_cost=cost, gradient_max_norm=gmax, radius=123.0)


def test_f_gradient_at_the_truth():
    g = SC.at_truth()
    got, info, gmax, before = run(S.case(g), gradient_tolerance=1e-8)
    assert got.tobytes() == before.tobytes()
    expect(info, iterations=0, accepted_steps=0, rejected_steps=0, invalid_steps=0, cg_iterations=0, termination_name="gradient",
           initial_cost=lambda v: 0 <= v <= 1e-20, final_cost=info["initial_cost"], gradient_max_norm=lambda v: v == gmax and v <= 1e-8, radius=1e4)


def test_f_function_tolerance():
    c = SC.get("ring65")
    first, one, _, _ = one_step(c, 1e4, max_cg=SC.cg_budget("ring65", "none", 1e4))
    params = dict(initial_radius=1e4, cg_eta=SC.TIGHT_ETA, max_cg_iterations=SC.cg_budget("ring65", "none", 1e4))
    got, info, gmax, before = run(c, **dict(ZERO, function_tolerance=1.0, **params))
    assert got.tobytes() == first.tobytes(), "the poses are the candidate of the one step"
    check_step("ring65", "none", 1e4, before, got, info)
    expect(info, iterations=1, accepted_steps=1, rejected_steps=0, invalid_steps=0, cg_iterations=one["cg_iterations"], termination_name="function",
           initial_cost=one["initial_cost"], final_cost=one["final_cost"], gradient_max_norm=gmax, radius=one["radius"])
    assert info["final_cost"] < info["initial_cost"] and one["termination_name"] == "max_iterations"


def test_f_parameter_tolerance():
    c = SC.get("ring65")
    got, info, gmax, before = run(c, **dict(ZERO, parameter_tolerance=1e3))
    assert got.tobytes() == before.tobytes()
    expect(info, iterations=1, accepted_steps=0, rejected_steps=0, invalid_steps=0, cg_iterations=lambda k: k >= 1, termination_name="parameter",
           initial_cost=lambda v: v > 0, final_cost=info["initial_cost"], gradient_max_norm=gmax, radius=1e4)


def test_f_min_radius():
    c = SC.get("step_control")
    got, info, gmax, before = run(c, **dict(ZERO, initial_radius=1000.0, min_radius=1000.0, cg_eta=SC.TIGHT_ETA))
    assert got.tobytes() == before.tobytes()
    expect(info, iterations=1, accepted_steps=0, rejected_steps=1, invalid_steps=0, cg_iterations=lambda k: k >= 1, termination_name="min_radius",
           initial_cost=lambda v: v > 0, final_cost=info["initial_cost"], gradient_max_norm=gmax, radius=500.0)


@pytest.mark.parametrize("limit,divisor", [(5, 1024.0), (2, 2.0)])
def test_f_invalid_steps(limit, divisor):
    """chi2 overflows to +inf at finite poses: every step is invalid (NaN arithmetic in a bounded loop)"""
    g = SC.invalid_graph()
    with build(S.case(g), **dict(ZERO, max_consecutive_invalid_steps=limit)) as pg:
        before = pg.poses()
        info = pg.optimize()
        got = pg.poses()
    print(f"(f) invalid steps, limit {limit}: {info}")
    assert got.tobytes() == before.tobytes()
    expect(info, iterations=limit, accepted_steps=0, rejected_steps=0, invalid_steps=limit, cg_iterations=0, termination_name="invalid_steps",
           initial_cost=np.inf, final_cost=np.inf, gradient_max_norm=lambda v: not v <= 1e100, radius=1e4 / divisor)
