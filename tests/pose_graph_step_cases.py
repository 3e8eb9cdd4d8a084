"""Cases for the per-step tests of sicp_graph_optimize (tests/test_pose_graph_step_cpu.py, tests/test_gpu_pose_graph_steps.py):
the smallest graphs that reach each path of the linear solve and of the step control.  A case is pose_graph_step_ref.case();
every reference is computed once and shared (functools.lru_cache) and must be left unchanged."""
import functools

import numpy as np

import pose_graph_cases as cases
import pose_graph_prior_ref as P
import pose_graph_ref as R
import pose_graph_step_ref as S

CAUCHY_A = 10.0  # weights from 0.003 to 1 on these graphs
LOSSES = {"none": (R.LOSS_NONE, 1.0), "cauchy": (R.LOSS_CAUCHY, CAUCHY_A)}
# Under the Cauchy loss the smallest radius is 1e-2, not 1e-4.  The rings start from integrated odometry: only the down-weighted
# closure has a residual, |g| is small, and at 1e-4 the step (1e-8) drowns in the rounding of the poses it is read off
# (eps |t|): the float64 restatement, observed the same way, misses the bound of test (a) by a factor of 23 there (with
# cauchy_a = 1.5: by 1400).  tests/test_pose_graph_step_cpu.py asserts that every case below is observable.
SMALL_RADII = {"none": (1e16, 1e4, 1.0, 1e-4), "cauchy": (1e16, 1e4, 1.0, 1e-2)}
TIGHT_ETA = 1e-10


def _priors(g, nodes, kinds, seed, noise=0.05):
    """priors near the truth: a pose prior z = truth exp(noise), a position prior the true position plus noise"""
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


def prior_ring():
    """ring(65, 6) with pose and position priors (three on node 5, one on the fixed node 0, one of them disabled) and two of
    the closures switched off; the odometry keeps every node joined to the fixed one"""
    g = cases.ring(65, 6, seed=31)
    nodes = [5, 5, 5, 0, 17, 33, 40, 52, 64]
    kinds = [P.POSE, P.POSITION, P.POSITION, P.POSE, P.POSITION, P.POSE, P.POSITION, P.POSE, P.POSITION]
    e_on = np.ones(len(g["ei"]), dtype=bool)
    e_on[[66, 68]] = False
    p_on = np.ones(len(nodes), dtype=bool)
    p_on[2] = False
    return g, _priors(g, nodes, kinds, 71), e_on, p_on


def lanes(n, seed=9):
    """counted()-style: random poses, anisotropic information, node 7 fixed; a chain k -> k + 1 keeps the graph in one piece
    and 2 n random edges (either order) give every node its own degree"""
    rng = np.random.default_rng(seed + n)
    truth = cases.random_pose(rng, n)
    a = rng.integers(0, n, size=2 * n)
    b = (a + rng.integers(1, n, size=2 * n)) % n
    ei = np.concatenate([np.arange(n - 1), a]).astype(np.int32)
    ej = np.concatenate([np.arange(1, n), b]).astype(np.int32)
    z = cases._measure(rng, truth, ei, ej)
    fixed = np.zeros(n, dtype=bool)
    fixed[7] = True
    return dict(poses=R.mul(truth, R.exp(rng.normal(size=(n, 6)) * 0.1)), fixed=fixed, ei=ei, ej=ej, z=z,
                omega=cases.random_spd(rng, len(ei)), truth=truth)


def banded(n, seed=10):
    """a helix of n poses with edges k -> k + 1 and k -> k + 2 (M = 2 n - 3), noise-free measurements, the poses a small seeded
    perturbation off the truth; node 0 fixed.  The bandwidth keeps a sparse direct solve cheap at any n."""
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.float64)
    xi = np.zeros((n, 6))
    xi[:, 5] = 0.05 * k % (2 * np.pi) - np.pi
    xi[:, 3] = 0.3 * np.sin(0.01 * k)
    truth = R.exp(xi)
    truth[:, 4], truth[:, 5], truth[:, 6] = 10 * np.cos(0.05 * k), 10 * np.sin(0.05 * k), 0.01 * k
    ei = np.concatenate([np.arange(n - 1), np.arange(n - 2)]).astype(np.int32)
    ej = np.concatenate([np.arange(1, n), np.arange(2, n)]).astype(np.int32)
    z = cases._measure(rng, truth, ei, ej, noise=False)
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    poses = R.mul(truth, R.exp(rng.normal(size=(n, 6)) * np.array([0.02] * 3 + [0.01] * 3)))
    poses[0] = truth[0]
    return dict(poses=poses, fixed=fixed, ei=ei, ej=ej, z=z, omega=cases.default_omega(len(ei)), truth=truth)


SMALL = {"ring65": lambda: (cases.ring(65, 1), None, None, None), "hub": lambda: (cases.hub(), None, None, None),
         "chain": lambda: (cases.chain(), None, None, None), "step_control": lambda: (cases.step_control(), None, None, None),
         "prior_ring": prior_ring}
LANE_NODES = (42, 43, 255, 256, 257)
LANE_RADII = (1e4, 1.0)
BANDED_NODES = (10923, 65537)


@functools.lru_cache(maxsize=None)
def graph(name):
    if name in SMALL:
        return SMALL[name]()
    kind, n = name.split("_")
    return ({"lanes": lanes, "banded": banded}[kind](int(n)), None, None, None)


@functools.lru_cache(maxsize=None)
def get(name, loss="none"):
    g, pri, e_on, p_on = graph(name)
    kind, a = LOSSES[loss]
    return S.case(g, pri, e_on, p_on, kind, a)


@functools.lru_cache(maxsize=None)
def lin(name, loss="none"):
    out = S.linearise(get(name, loss))
    for v in (out["g"], out["poses"]):
        v.setflags(write=False)
    return out


def step_cases():
    """(name, loss, radius) of test (a)"""
    out = [(n, l, r) for n in SMALL for l in LOSSES for r in SMALL_RADII[l]]
    out += [(f"lanes_{n}", "none", r) for n in LANE_NODES for r in LANE_RADII]
    out += [(f"banded_{n}", "none", 1.0) for n in BANDED_NODES]
    return out


@functools.lru_cache(maxsize=None)
def system(name, loss, radius, lo=1e-6, hi=1e32):
    """the damped matrix of a case at a radius"""
    return S.damped_system(lin(name, loss), radius, lo, hi)[0]


@functools.lru_cache(maxsize=None)
def solve(name, loss, radius, lo=1e-6, hi=1e32, eta=TIGHT_ETA, keep=()):
    """the damped system of a case and the restated conjugate gradients on it, run to `eta`"""
    A = system(name, loss, radius, lo, hi)
    return A, S.pcg(A, -lin(name, loss)["g"], eta, 5000, keep)


BANDED_CG_BUDGET = 40  # twice what the restatement takes on the banded graphs at radius 1 (asserted on the CPU)


def cg_budget(name, loss, radius, lo=1e-6, hi=1e32):
    """max_cg_iterations of a one-step test: twice the restatement's iterations to TIGHT_ETA"""
    if name.startswith("banded"):
        return BANDED_CG_BUDGET
    return 2 * solve(name, loss, radius, lo, hi)[1]["iterations"]


@functools.lru_cache(maxsize=None)
def first_step(name, loss, radius):
    """(outcome, rho) of the reference's first step: "accepted" / "rejected" under min_relative_decrease = 1e-3"""
    rho = float(S.lm_step(get(name, loss), lin(name, loss), radius)["rho"])
    return ("accepted" if rho > 1e-3 else "rejected"), rho


def residual_bound(A, g, delta, eta, tol, factor=2.0):
    """|-g - A delta| and the bound of test (a): factor * eta |g| + tol | |A| |delta| |"""
    res = float(np.linalg.norm(-g - A @ delta))
    return res, factor * eta * float(np.linalg.norm(g)) + tol * float(np.linalg.norm(abs(A) @ np.abs(delta)))


# (b) the two clips: above every diagonal entry of H, and below every nonzero one
CLIPS = {"lo_above": dict(min_lm_diagonal=1e6), "hi_below": dict(min_lm_diagonal=1e-9, max_lm_diagonal=1e-3)}
CLIP_CASES = [(n, c) for n in ("ring65", "prior_ring") for c in CLIPS]
CLIP_RADIUS = 1e4

# (c) the stopping rule: (name, radius, eta) whose restated residual falls from >= 2 eta to <= eta / 2 in iteration k_ref.  The
# radii are searched; per (name, eta) the case with the most iterations is kept.
STOP_NAMES = ("ring65", "hub", "prior_ring", "lanes_43")
STOP_ETAS = (0.1, 1e-3, 1e-6)
STOP_RADII = tuple(10.0 ** (k / 2) for k in range(-4, 9))


@functools.lru_cache(maxsize=1)
def stop_cases():
    """[(name, radius, eta, k_ref)]"""
    out = []
    for name in STOP_NAMES:
        for eta in STOP_ETAS:
            best = None
            for radius in STOP_RADII:
                _, run = solve(name, "none", radius, eta=eta)
                k, ratios = run["iterations"], run["ratios"]
                before = ratios[k - 2] if k >= 2 else 1.0
                if run["state"] == "converged" and k >= 1 and before >= 2 * eta and ratios[k - 1] <= eta / 2 and (best is None or k > best[3]):
                    best = (name, radius, eta, k)
            if best:
                out.append(best)
    return out


@functools.lru_cache(maxsize=None)
def truncated(name, radius, eta, k_ref):
    """[(k, noise, x_k)] for the k < k_ref a test stops the solve at.  x_k is the restatement's iterate in float64 as a test
    can observe it: applied to the poses and read off them again (pose_graph_step_ref.step_of).  noise is its distance, relative
    to |x_k|, from the iterate of the same chain -- linearisation, damped system, recurrences -- in np.longdouble."""
    ks = tuple(sorted({k for k in (1, k_ref // 2, k_ref - 1) if 1 <= k < k_ref}))
    if not ks:
        return []
    l = lin(name)
    A, g, _ = S.damped_system(l, radius)
    x64 = S.pcg(A, -g, eta, k_ref, ks)["iterates"]
    A80, g80, _ = S.damped_system(S.linearise(get(name), dtype=np.longdouble), radius)
    x80 = S.pcg(A80, -g80, eta, k_ref, ks)["iterates"]
    out = []
    for k in ks:
        seen = S.step_of(l["poses"], R.retract(l["poses"], l["fixed"], x64[k]))
        out.append((k, float(np.linalg.norm(seen - x80[k]) / np.linalg.norm(x80[k])), seen))
    return out


# (d) the gain ratio of step_control()'s first step by radius (the reference alone, to +-0.02), and a radius whose rho >= 0.95
GAIN_TABLE = {50.0: 0.906, 100.0: 0.750, 300.0: 0.305, 1000.0: -0.38}
TRIPLE_RADIUS = 20.0


def radius_noise(c, radius, delta, max_radius=1e16, poses=None):
    """the radius after an accepted step `delta` from `poses` (default: the case's own), its gain ratio, and the relative
    distance of the radius' float64 evaluation from np.longdouble's at the same step"""
    rho = float(S.gain(c, S.linearise(c, poses), delta)["rho"])
    r64 = S.new_radius(radius, rho, max_radius)
    r80 = S.new_radius(radius, S.gain(c, S.linearise(c, poses, dtype=np.longdouble), delta)["rho"], max_radius)
    return float(r64), float(abs(r64 - r80) / r80), rho


# (e) the loops whose bookkeeping is followed iteration by iteration, both on step_control() from initial_radius = 1e16
LOOPS = {"rejections_then_three_accepted": dict(initial_radius=1e16),
         "a_rejection_after_acceptances": dict(initial_radius=1e16, min_relative_decrease=0.92)}
ZERO_TOLERANCES = dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0)


@functools.lru_cache(maxsize=None)
def loop_trace(which):
    """(records[:K], K): K is the first iteration count at which the trace has made three accepted steps after its rejections,
    or its first rejection after an acceptance"""
    records, _ = S.trace(get("step_control"), dict(ZERO_TOLERANCES, **LOOPS[which]), 40)
    o = "".join(r["outcome"][0] for r in records)
    K = o.index("aaa") + 3 if which == "rejections_then_three_accepted" else o.index("ar") + 2
    return records[:K], K


def invalid_graph():
    """finite poses whose chi2 overflows: two nodes 1e160 apart under an information of 1e4"""
    poses = np.array([[0, 0, 0, 1, 0, 0, 0.0], [0, 0, 0, 1, 1e160, -2e160, 5e159], [0, 0, 0, 1, 1.0, 2.0, 3.0]])
    ei, ej = np.array([0, 1], dtype=np.int32), np.array([1, 2], dtype=np.int32)
    z = np.tile(np.array([0, 0, 0, 1, 1.0, 0, 0]), (2, 1))
    return dict(poses=poses, fixed=np.array([True, False, False]), ei=ei, ej=ej, z=z, omega=np.tile(np.eye(6) * 1e4, (2, 1, 1)))


def at_truth():
    """a noise-free ring at its truth: the gradient is zero to rounding"""
    g = cases.ring(12, 1, seed=12, noise=False)
    g["poses"] = g["truth"].copy()
    return g
