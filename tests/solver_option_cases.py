"""Cases for the registration solve at every solver option and termination (tests/test_solver_options_cpu.py and
tests/test_gpu_solver_options.py): the twelve trust-region options of sicp_params, outer_tol / max_outer, lm_batch and
lm_on_device, each moved off its default so far that the branch it guards is taken.

Data: synth.config1_pair(), 2100 x 2100 points, labels {1, 2, 4}; GICP (K = 1), EM (K = 4, C = 11) and SEMANTIC (K = 1).
Two starts: NEAR (the identity) and FAR (25 degrees about (1, 2, 3) and (2, -1, 0.5) m off: mostly wrong matches, so the
default solve rejects steps in runs).

The reference is always the oracle (oracle_lib.solve_trace / align).  sicp_solve does not return the termination
status, so a test reads it off lm_iters, evals (1 + the attempts of the trace that are not invalid) and whether the
pose is still the start; `expectation()` derives the three from the oracle's trace.

No figure in this file is an expected value of a GPU run: the tests compute their expectations from the oracle on the
engine's own correspondences at run time.  What is fixed here is which option each case moves and the rule it must end on
(the CPU module asserts that the oracle shows it).
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
import synth
from np_ref import mat_to_qt

C_EM = 11
MODES = (O.MODE_GICP, O.MODE_EM, O.MODE_SEMANTIC)
MODE_NAMES = {O.MODE_GICP: "gicp", O.MODE_EM: "em", O.MODE_SEMANTIC: "semantic"}
KNN = {O.MODE_GICP: 1, O.MODE_EM: 4, O.MODE_SEMANTIC: 1}

NEAR = np.array([0, 0, 0, 1, 0, 0, 0.0])
FAR = mat_to_qt(synth.pose_matrix(25.0, (1, 2, 3), (2.0, -1.0, 0.5)))
STARTS = {"NEAR": NEAR, "FAR": FAR}
for _a in (NEAR, FAR):
    _a.setflags(write=False)

OPTION_FIELDS = ("max_lm_iterations", "gradient_tolerance", "function_tolerance", "parameter_tolerance", "initial_radius", "max_radius",
                 "min_radius", "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal", "max_consecutive_invalid_steps",
                 "jacobi_scaling")
OPTION_DEFAULTS = dict(max_lm_iterations=400, gradient_tolerance=1e-11, function_tolerance=1e-11, parameter_tolerance=1e-8,
                       initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_lm_diagonal=1e-6,
                       max_lm_diagonal=1e32, max_consecutive_invalid_steps=5, jacobi_scaling=1)

# ---- (A) stop rules: name -> (start, options, how the oracle must end) -------------------------------------------------------------
# "cap": status 1 after exactly max_lm_iterations; "stops_before": status 0, and the same solve with the named options back at
# their defaults runs on from the same trace (so the named option is what stopped it); "at_start": 0 iterations, 1 evaluation,
# the pose untouched, under the same condition; "runs_past": status 0 later than the default solve.
STOP_CASES = {
    "cap0": ("FAR", dict(max_lm_iterations=0), ("cap",)),
    "cap1": ("FAR", dict(max_lm_iterations=1), ("cap",)),
    "cap7": ("FAR", dict(max_lm_iterations=7), ("cap",)),
    "grad_stop_at_start": ("FAR", dict(gradient_tolerance=1e30), ("at_start", ("gradient_tolerance",))),
    # (at 1e3 the rotational part of the gradient is far beyond the range of lm.hpp's cheap bound gradient_clearly_above: the exact
    # norm decides every time.  Both sides of the bound are taken by near_gradient_bound below.)
    "grad_stop_midway": ("NEAR", dict(gradient_tolerance=1e3), ("stops_before", ("gradient_tolerance",))),
    "function": ("FAR", dict(function_tolerance=1e-3), ("stops_before", ("function_tolerance",))),
    "parameter": ("FAR", dict(parameter_tolerance=1e-3), ("stops_before", ("parameter_tolerance",))),
    "min_radius": ("FAR", dict(min_radius=1e3), ("stops_before", ("min_radius",))),
    "min_radius_at_start": ("FAR", dict(min_radius=1e4, initial_radius=1e4), ("at_start", ("min_radius",))),
    # All tolerances 0.  Left alone the oracle runs 99 / 78 / 122 iterations and ends on cost_change == 0, but from about attempt 46
    # / 40 / 59 on the cost changes by less than 1e-9 of itself and accept / reject follows the last bits of the sums: no two
    # float64 evaluations agree there (measured with the sums scaled by 1 + 1e-10 xi and 1 + 1e-9 xi, 8 seeds each).  So the case
    # is cut where every decision still has a margin of 100 over that noise -- it shows that no stop rule fires with a zero
    # tolerance, not where such a solve would end.
    "zero_tolerances": ("FAR", dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0, max_lm_iterations=30), ("cap",)),
    # The default tolerances from NEAR, cut before the noise: iterates with a large rotational gradient (the cheap bound cannot
    # tell, the exact norm is evaluated) and, from the 9th / 8th / 11th iterate on, ones the bound settles.
    "near_gradient_bound": ("NEAR", dict(max_lm_iterations={O.MODE_GICP: 10, O.MODE_EM: 9, O.MODE_SEMANTIC: 12}), ("cap",)),
}

# ---- (B) options that change the path: all from FAR under a cap of 25 iterations; name -> (options, the case to differ from) -----------
PATH_CAP = 25
PATH_CASES = {
    "default25": (dict(), None),
    "max_radius_1e4": (dict(max_radius=1e4), "default25"),
    "min_rel_decrease_0p5": (dict(min_relative_decrease=0.5), "default25"),
    "min_rel_decrease_0p9": (dict(min_relative_decrease=0.9), "default25"),
    "initial_radius_1": (dict(initial_radius=1.0), "default25"),
    "initial_radius_1e16": (dict(initial_radius=1e16), "default25"),
    "min_lm_diagonal_1e3": (dict(min_lm_diagonal=1e3), "default25"),
    "max_lm_diagonal_1em9": (dict(max_lm_diagonal=1e-9, min_lm_diagonal=1e-12), "default25"),
    # with a Jacobi-scaled LM diagonal the scaling cancels unless a clamp acts: scaling off is compared at the same clamp
    "no_scaling_min_lm_diagonal_1e3": (dict(jacobi_scaling=0, min_lm_diagonal=1e3), "min_lm_diagonal_1e3"),
}

# ---- (C) invalid steps in any mode: diag / radius overflows to +inf, the factorisation returns a zero step, model_change = 0 ----------
DENORMAL = dict(initial_radius=1e-320, min_radius=5e-324)
INVALID_CASES = {  # name -> (options, the oracle's sequence, status, iterations)
    "den_inv5": (dict(DENORMAL), "iiiii", 2, 5),
    "den_inv1": (dict(DENORMAL, max_consecutive_invalid_steps=1), "i", 2, 1),
    "den_cap3": (dict(DENORMAL, max_lm_iterations=3), "iii", 1, 3),
    "den_min_radius": (dict(DENORMAL, initial_radius=2e-323, max_consecutive_invalid_steps=50), "ii", 0, 2),
}

# ---- (D) a solve longer than one persistent launch (kSoloMaxEvals = 1024 evaluations) --------------------------------------------------
LONG_ITERATIONS = 1100
LONG_CASE = dict(initial_radius=1e-4, max_radius=1e-4, max_lm_iterations=LONG_ITERATIONS)
SOLO_MAX_EVALS = 1024

# ---- (E) outer loop, from NEAR: name -> (options, outer_iters of oracle_lib.align per mode GICP / EM / SEMANTIC) ----------------------
# (the last row: the reference's `outer > max_outer` against SEMANTIC's `count > max_outer`)
OUTER_CASES = {
    "outer_defaults": (dict(), (3, 2, 2)),
    "outer_tol_1e30": (dict(outer_tol=1e30), (1, 1, 1)),
    "max_outer_0": (dict(max_outer=0), (2, 2, 1)),
    "outer_tol_0_max_outer_4": (dict(outer_tol=0.0, max_outer=4), (6, 6, 5)),
}


def _cases():
    out = {}
    for name, (start, opts, _) in STOP_CASES.items():
        out[name] = (start, dict(opts))
    for name, (opts, _) in PATH_CASES.items():
        out[name] = ("FAR", dict(opts, max_lm_iterations=PATH_CAP))
    for name, (opts, _, _, _) in INVALID_CASES.items():
        out[name] = ("FAR", dict(opts))
    out["long"] = ("NEAR", dict(LONG_CASE))
    return out


CASES = _cases()              # name -> (start name, options): every inner-solve case of (A)-(D); a dict as a value: per mode


def case(name, mode):
    """(start name, options) of a case in a mode"""
    start, opts = CASES[name]
    return start, {k: (v[mode] if isinstance(v, dict) else v) for k, v in opts.items()}

# Options sicp_set_params refuses (one broken condition each, on top of the defaults) -- never handed to a call that reaches the GPU.
REFUSED = {
    "nan_initial_radius": dict(initial_radius=float("nan")),
    "inf_max_radius": dict(max_radius=float("inf")),
    "nan_min_radius": dict(min_radius=float("nan")),
    "nan_gradient_tolerance": dict(gradient_tolerance=float("nan")),
    "inf_function_tolerance": dict(function_tolerance=float("inf")),
    "nan_parameter_tolerance": dict(parameter_tolerance=float("nan")),
    "nan_min_relative_decrease": dict(min_relative_decrease=float("nan")),
    "nan_min_lm_diagonal": dict(min_lm_diagonal=float("nan")),
    "inf_max_lm_diagonal": dict(max_lm_diagonal=float("inf")),
    "negative_gradient_tolerance": dict(gradient_tolerance=-1e-11),
    "negative_function_tolerance": dict(function_tolerance=-1e-11),
    "negative_parameter_tolerance": dict(parameter_tolerance=-1e-8),
    "negative_min_radius": dict(min_radius=-1e-32),
    "zero_initial_radius": dict(initial_radius=0.0, min_radius=0.0),
    "min_radius_above_initial": dict(min_radius=1e5),
    "initial_radius_above_max": dict(initial_radius=1e17),
    "min_relative_decrease_1": dict(min_relative_decrease=1.0),
    "negative_min_relative_decrease": dict(min_relative_decrease=-1e-3),
    "negative_min_lm_diagonal": dict(min_lm_diagonal=-1e-6),
    "min_lm_diagonal_above_max": dict(min_lm_diagonal=1e33),
    "negative_max_lm_iterations": dict(max_lm_iterations=-1),
    "zero_max_consecutive_invalid_steps": dict(max_consecutive_invalid_steps=0),
    "negative_max_consecutive_invalid_steps": dict(max_consecutive_invalid_steps=-3),
}
REFUSED_FIELD = {  # the field sicp_last_error must name
    "min_radius_above_initial": "min_radius", "initial_radius_above_max": "initial_radius", "zero_initial_radius": "initial_radius",
    "min_lm_diagonal_above_max": "min_lm_diagonal",
}
# Legal by the same rule, at its edges: caps near INT_MAX where only the radius ends the retry loop, denormal radii
LEGAL_EXTREMES = {
    "int_max_caps_denormal_radius": dict(DENORMAL, max_lm_iterations=2**31 - 1, max_consecutive_invalid_steps=2**31 - 1),
    "int_max_caps_zero_min_radius": dict(min_radius=0.0, initial_radius=1e-300, max_radius=1e-300, max_lm_iterations=2**31 - 1,
                                         max_consecutive_invalid_steps=2**31 - 1, min_lm_diagonal=1e31, max_lm_diagonal=1e32),
    "all_bounds_equal": dict(min_radius=1.0, initial_radius=1.0, max_radius=1.0, min_lm_diagonal=1.0, max_lm_diagonal=1.0),
    "zero_everything_legal": dict(gradient_tolerance=0.0, function_tolerance=0.0, parameter_tolerance=0.0, min_radius=0.0,
                                  min_relative_decrease=0.0, min_lm_diagonal=0.0, max_lm_iterations=0),
}


def refused_field(name):
    if name in REFUSED_FIELD:
        return REFUSED_FIELD[name]
    (field,) = [f for f in REFUSED[name] if f in OPTION_FIELDS]
    return field


# ---- parameters ------------------------------------------------------------------------------------------------------------------------
def oracle_params(mode, C=None, **kw):
    p = O.default_params(mode)
    p.num_classes = (C_EM if mode == O.MODE_EM else 0) if C is None else C
    p.use_kdtree = 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def apply(p, opts):
    """the options of a case onto a parameter struct of the product or of the oracle (same field names)"""
    for k, v in opts.items():
        setattr(p, k, v)
    return p


# ---- the data, and the oracle's own slots for the CPU module -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair():
    src, sl, tgt, tl, _ = synth.config1_pair()
    for a in (src, sl, tgt, tl):
        a.setflags(write=False)
    return src, sl, tgt, tl


@functools.lru_cache(maxsize=None)
def oracle_features(mode):
    """covariances as the oracle's align() computes them: over the whole cloud, or per label segment in SEMANTIC"""
    src, sl, tgt, tl = pair()
    if mode != O.MODE_SEMANTIC:
        return O.covariances(src, None, 20, 1e-3, kdtree=True)[0], O.covariances(tgt, None, 20, 1e-3, kdtree=True)[0]
    cs, ct = np.empty((len(src), 3, 3)), np.empty((len(tgt), 3, 3))
    for cloud, lab, out in ((src, sl, cs), (tgt, tl, ct)):
        for L in np.unique(lab):
            m = np.nonzero(lab == L)[0]
            out[m] = O.covariances(np.ascontiguousarray(cloud[m]), None, 20, 1e-3, kdtree=True)[0]
    return cs, ct


@functools.lru_cache(maxsize=None)
def oracle_slots(mode, start_name):
    """(idx, w) at a start pose from the oracle's own k-NN: gate 250, EM weights drawn from U(0.2, 1) (any positive weights
    make a well-posed solve; the label path has its own tests), SEMANTIC searched label by label"""
    src, sl, tgt, tl = pair()
    K = KNN[mode]
    moved = O.transform_points(O.se3_matrix(STARTS[start_name]), src)
    if mode == O.MODE_SEMANTIC:
        idx = np.full((len(src), K), -1, dtype=np.int32)
        d2 = np.full((len(src), K), np.inf, dtype=np.float32)
        for L in np.unique(sl):
            ms, mt = np.nonzero(sl == L)[0], np.nonzero(tl == L)[0]
            i, d = O.knn(np.ascontiguousarray(moved[ms]), np.ascontiguousarray(tgt[mt]), K, kdtree=True)
            idx[ms], d2[ms] = mt[i], d
    else:
        idx, d2 = O.knn(moved, tgt, K, kdtree=True)
    idx = np.where(d2 < np.float32(250), idx, -1).astype(np.int32)
    w = np.random.default_rng(7).uniform(0.2, 1.0, idx.shape) if mode == O.MODE_EM else None
    idx.setflags(write=False)
    if w is not None:
        w.setflags(write=False)
    return idx, w


# ---- reading the oracle ----------------------------------------------------------------------------------------------------------------
SEQ = {1: "a", 0: "r", -1: "i"}
MAX_TRACE = 4000


def expectation(op, src, cs, tgt, ct, idx, w, start):
    """What a solve must report, from the oracle's trace: status, lm_iters (one per attempt), evals as the product counts them
    (one evaluation gives cost, gradient and H together: 1 + the attempts that are not invalid), the accept / reject / invalid
    sequence, the pose, whether it is still the start, and the cost at the pose."""
    q, tr = O.solve_trace(op, src, cs, tgt, ct, idx, w, start, max_trace=MAX_TRACE)
    acc = tr["accepted"]
    assert len(acc) < MAX_TRACE
    cost = O.accumulate(op, q, src, cs, tgt, ct, idx, w)[27]
    return dict(status=tr["status"], lm_iters=len(acc), evals=1 + int((acc != -1).sum()), seq="".join(SEQ[int(a)] for a in acc),
                pose=q, unchanged=bool(np.array_equal(q, np.asarray(start, dtype=np.float64))), cost=cost, trace=tr)


def first_difference(ta, tb, rel=1e-6):
    """the first attempt at which two traces part (decision, radius or candidate cost beyond `rel`), or None"""
    n = min(len(ta["accepted"]), len(tb["accepted"]))
    for k in range(n):
        if ta["accepted"][k] != tb["accepted"][k]:
            return k
        for key in ("radius", "cand_cost"):
            a, b = ta[key][k], tb[key][k]
            if abs(a - b) > rel * max(abs(a), abs(b)):
                return k
    return n if len(ta["accepted"]) != len(tb["accepted"]) else None


def is_prefix(short, long, rel=1e-9):
    """`long` runs through the attempts of `short` (the last one's decision aside: a stop leaves its attempt marked rejected)"""
    n = len(short["accepted"])
    if len(long["accepted"]) < n:
        return False
    if n == 0:
        return True
    same = np.array_equal(short["accepted"][: n - 1], long["accepted"][: n - 1])
    return bool(same and np.allclose(short["radius"], long["radius"][:n], rtol=rel, atol=0)
                and np.allclose(short["cand_cost"], long["cand_cost"][:n], rtol=rel, atol=0))


def outer_replay(op, correspondences, src, cs, tgt, ct, init, sem):
    """The outer loop of align() (em_icp.hpp:179-187 / semantic_icp.hpp:151-158) around the oracle's inner solve, on the slots
    `correspondences(pose)` hands back: (pose, outer_iters, total_lm_iters, total_evals as the product counts them, accepted
    steps -- each of which costs the oracle a second sweep, so its own total_evals is the sum of the last two)."""
    cur = np.array(init, dtype=np.float64)
    outer = count = iters = evals = accepted = 0
    while True:
        if sem:
            count += 1
        idx, w = correspondences(cur)
        if (idx >= 0).any():
            ex = expectation(op, src, cs, tgt, ct, idx, w, cur)
            est, iters, evals, accepted = ex["pose"], iters + ex["lm_iters"], evals + ex["evals"], accepted + ex["seq"].count("a")
        else:
            est = cur
        lg = O.se3_log(O.se3_mul(O.se3_inv(cur), est))
        mse = 0.0
        for v in lg:
            mse += float(v) * float(v)
        done = mse < op.outer_tol or (count if sem else outer) > op.max_outer
        cur = est
        if not sem:
            outer += 1
        if done:
            return cur, (count if sem else outer), iters, evals, accepted
