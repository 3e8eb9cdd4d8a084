"""A numpy restatement of what sicp_graph_optimize does after the linearisation (include/sicp.h, "pose graph", rule 3): the
damped system, one Levenberg-Marquardt step, the block-Jacobi preconditioned conjugate gradients of the kernels and the driver's
step control.  On top of pose_graph_ref and pose_graph_prior_ref, which it imports unchanged; every function works in the dtype
it is given (np.float64, or np.longdouble on small graphs, where rounding noise is measured).

A case is a dict: g (a graph of pose_graph_cases), pri (priors of pose_graph_prior_ref, or None), e_on / p_on (enabled flags or
None), kind and a (the loss).  `lin` is what linearise() returns."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pose_graph_prior_ref as P
import pose_graph_ref as R

TERMINATIONS = ("gradient", "function", "parameter", "max_iterations", "min_radius", "invalid_steps")
DEFAULTS = dict(max_iterations=100, gradient_tolerance=1e-10, function_tolerance=1e-12, parameter_tolerance=1e-12, initial_radius=1e4,
                min_radius=1e-32, max_radius=1e16, min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32,
                max_consecutive_invalid_steps=5)


def case(g, pri=None, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0):
    return dict(g=g, pri=P.none() if pri is None else pri, e_on=e_on, p_on=p_on, kind=kind, a=a)


def _parts(c):
    g, pri = c["g"], c["pri"]
    e_on, p_on = P._masks(len(g["ei"]), len(pri["node"]), c["e_on"], c["p_on"])
    return g, pri, e_on, p_on, np.asarray(g["fixed"], dtype=bool)


def cost(c, poses, dtype=np.float64):
    """1/2 sum rho over the enabled edges and priors, summed in dtype"""
    g, pri, e_on, p_on, _ = _parts(c)
    x = np.asarray(poses, dtype=dtype)
    r = R.residual(x[g["ei"][e_on]], x[g["ej"][e_on]], g["z"][e_on].astype(dtype))
    om = g["omega"][e_on].astype(dtype)
    total = np.sum(R.loss(c["kind"], c["a"], np.einsum("ea,eab,eb->e", r, om, r))[0])
    if p_on.any():
        total = total + np.sum(P.priors(x, pri, c["kind"], c["a"])["rho"][p_on])
    return total / dtype(2)


def linearise(c, poses=None, dtype=np.float64):
    """cost, g [6n] and H at the poses, with the header's rules: a fixed node has the identity block, a zero gradient and no
    couplings; a node without enabled entries a zero block.  H is CSC in float64, a dense array in any other dtype."""
    g, pri, e_on, p_on, fixed = _parts(c)
    x = np.asarray(g["poses"] if poses is None else poses, dtype=dtype)
    n = len(x)
    ei, ej = g["ei"][e_on], g["ej"][e_on]
    E = R.edges(x, ei, ej, g["z"][e_on].astype(dtype), g["omega"][e_on].astype(dtype), c["kind"], c["a"])
    grad, D = R.node_sums(n, np.zeros(n, dtype=bool), ei, ej, E)
    total = np.sum(E["rho"])
    if len(pri["node"]):
        PE = P.priors(x, pri, c["kind"], c["a"])
        np.add.at(D, pri["node"][p_on], PE["H"][p_on])
        np.add.at(grad, pri["node"][p_on], PE["g"][p_on])
        total = total + np.sum(PE["rho"][p_on])
    D[fixed] = np.eye(6, dtype=dtype)
    grad[fixed] = 0
    free = ~fixed[ei] & ~fixed[ej]
    bi, bj, B = ei[free], ej[free], E["B"][free]
    k6 = np.arange(6)
    if dtype is np.float64:
        def index(a, b):
            rows = 6 * a[:, None, None] + k6[None, :, None] + 0 * k6[None, None, :]
            cols = 6 * b[:, None, None] + k6[None, None, :] + 0 * k6[None, :, None]
            return rows.ravel(), cols.ravel()
        nodes = np.arange(n)
        (r0, c0), (r1, c1) = index(nodes, nodes), index(bi, bj)
        H = sp.coo_matrix((np.concatenate([D.ravel(), B.ravel(), B.ravel()]), (np.concatenate([r0, r1, c1]), np.concatenate([c0, c1, r1]))),
                          shape=(6 * n, 6 * n)).tocsc()
    else:
        H = np.zeros((n, 6, n, 6), dtype=dtype)
        H[np.arange(n), :, np.arange(n), :] = D
        np.add.at(H, (bi[:, None, None], k6[None, :, None], bj[:, None, None], k6[None, None, :]), B)
        np.add.at(H, (bj[:, None, None], k6[None, None, :], bi[:, None, None], k6[None, :, None]), B)
        H = H.reshape(6 * n, 6 * n)
    return dict(cost=total / dtype(2), g=grad.ravel(), H=H, poses=x, fixed=fixed, dtype=dtype)


def diagonal(H):
    return H.diagonal() if sp.issparse(H) else np.diagonal(H).copy()


def damping(lin, radius, lo, hi):
    dt = lin["dtype"]
    return np.clip(diagonal(lin["H"]), dt(lo), dt(hi)) / dt(radius)


def damped_system(lin, radius, lo=1e-6, hi=1e32):
    """A = H + diag(clip(diag H, lo, hi)) / radius, g and H"""
    d = damping(lin, radius, lo, hi)
    H = lin["H"]
    A = (H + sp.diags(d)).tocsc() if sp.issparse(H) else H + np.diag(d)
    return A, lin["g"], H


def gain(c, lin, delta):
    """for a given step: the model decrease -g.delta - 1/2 delta^T H delta, the candidate poses, their cost and rho"""
    dt = lin["dtype"]
    delta = np.asarray(delta, dtype=dt)
    model = -(lin["g"] @ delta) - (delta @ (lin["H"] @ delta)) / dt(2)
    cand = R.retract(lin["poses"], lin["fixed"], delta)
    cc = cost(c, cand, dt)
    return dict(model=model, cand=cand, cand_cost=cc, rho=(lin["cost"] - cc) / model)


def lm_step(c, lin, radius, lo=1e-6, hi=1e32):
    """the direct solve of the damped system and its gain()"""
    A, g, _ = damped_system(lin, radius, lo, hi)
    delta = spla.spsolve(A, -g) if sp.issparse(A) else np.linalg.solve(A.astype(np.float64), -g.astype(np.float64)).astype(lin["dtype"])
    out = gain(c, lin, delta)
    out["delta"] = delta
    return out


def new_radius(radius, rho, max_radius=1e16):
    """the radius after an accepted step, in the dtype of rho"""
    dt = type(rho)
    t = dt(2) * rho - dt(1)
    return min(dt(max_radius), dt(radius) / max(dt(1) / dt(3), dt(1) - t * t * t))


# ---- the kernels' conjugate gradients -------------------------------------------------------------------------------------------
def _blocks(A, n):
    if sp.issparse(A):
        k6 = np.arange(6)
        rows = 6 * np.arange(n)[:, None, None] + k6[None, :, None] + 0 * k6[None, None, :]
        cols = 6 * np.arange(n)[:, None, None] + k6[None, None, :] + 0 * k6[None, :, None]
        return np.asarray(A[rows.ravel(), cols.ravel()]).reshape(n, 6, 6)
    return A.reshape(n, 6, n, 6)[np.arange(n), :, np.arange(n), :].copy()


def cholesky6(D):
    """per node the lower factor of a 6x6 block, column by column as the kernel forms it; ok[n] = every pivot was positive"""
    L = np.zeros_like(D)
    ok = np.ones(len(D), dtype=bool)
    for i in range(6):
        for j in range(i + 1):
            s = D[:, i, j].copy()
            for k in range(j):
                s = s - L[:, i, k] * L[:, j, k]
            if i == j:
                bad = ~(s > 0)
                ok &= ~bad
                L[:, i, i] = np.sqrt(np.where(bad, 1, s))
            else:
                L[:, i, j] = s / L[:, j, j]
    return L, ok


def cholesky6_solve(L, r):
    """(L L^T)^-1 r per node"""
    y = np.zeros_like(r)
    z = np.zeros_like(r)
    for i in range(6):
        s = r[:, i].copy()
        for k in range(i):
            s = s - L[:, i, k] * y[:, k]
        y[:, i] = s / L[:, i, i]
    for i in range(5, -1, -1):
        s = y[:, i].copy()
        for k in range(i + 1, 6):
            s = s - L[:, k, i] * z[:, k]
        z[:, i] = s / L[:, i, i]
    return z


def pcg(A, b, eta, max_iters, keep=()):
    """Block-Jacobi preconditioned conjugate gradients on A x = b from x = 0, as the kernels run them: alpha = rz / pq,
    beta = rz' / rz, the stop sqrt(rr) <= eta sqrt(bb) tested after the update, `iterations` counted as S->cg_iters.  Returns
    x, iterations, ratios (|r| / |b| of the recursive residual after every iteration), state ("converged", "max" or "breakdown")
    and iterates {k: x_k} for the k in `keep`."""
    n = len(b) // 6
    L, ok = cholesky6(_blocks(A, n))
    apply = lambda r: cholesky6_solve(L, r.reshape(n, 6)).ravel()
    x, r = np.zeros_like(b), b.copy()
    z = apply(r)
    p = z.copy()
    rz, rr = r @ z, r @ r
    bb = rr
    out = dict(x=x, iterations=0, ratios=[], state="max", iterates={})
    if not ok.all() or not np.isfinite(rz) or not np.isfinite(rr):
        out["state"] = "breakdown"
        return out
    if bb == 0:
        out["state"] = "converged"
        return out
    for _ in range(max_iters):
        q = A @ p
        pq = p @ q
        if not np.isfinite(pq) or not pq > 0:
            out["state"] = "breakdown"
            break
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = apply(r)
        rz_new, rr = r @ z, r @ r
        if not np.isfinite(rz_new) or not np.isfinite(rr):
            out["state"] = "breakdown"
            break
        beta = rz_new / rz
        rz = rz_new
        out["iterations"] += 1
        out["ratios"].append(float(np.sqrt(rr) / np.sqrt(bb)))
        if out["iterations"] in keep:
            out["iterates"][out["iterations"]] = x.copy()
        if np.sqrt(rr) <= eta * np.sqrt(bb):
            out["state"] = "converged"
            break
        p = z + beta * p
    out["x"] = x
    return out


# ---- the driver's loop ----------------------------------------------------------------------------------------------------------
def trace(c, params=None, n=None):
    """The loop of sicp_graph_optimize with direct solves in place of the conjugate gradients.  Returns (records, end): one
    record per iteration -- the radius it ran at, outcome ("accepted", "rejected" or "invalid"), rho, the cost and the radius
    after it -- and the state at the end (the fields of sicp_graph_info by their names, termination as a name)."""
    p = dict(DEFAULTS)
    p.update(params or {})
    if n is not None:
        p["max_iterations"] = n
    lin = linearise(c)
    radius, factor, invalid = p["initial_radius"], 2.0, 0
    end = dict(iterations=0, accepted_steps=0, rejected_steps=0, invalid_steps=0, initial_cost=float(lin["cost"]))
    records = []
    while True:
        gmax = np.abs(lin["g"]).max()
        if np.isnan(gmax):
            gmax = np.inf
        if not gmax > p["gradient_tolerance"]:
            end["termination"] = "gradient"; break
        if end["iterations"] >= p["max_iterations"]:
            end["termination"] = "max_iterations"; break
        if radius < p["min_radius"]:
            end["termination"] = "min_radius"; break
        end["iterations"] += 1
        rec = dict(radius=radius, rho=None)
        records.append(rec)
        valid = bool(np.isfinite(lin["g"]).all() and np.isfinite(lin["H"].data if sp.issparse(lin["H"]) else lin["H"]).all())
        if valid:
            with np.errstate(all="ignore"):
                s = lm_step(c, lin, radius, p["min_lm_diagonal"], p["max_lm_diagonal"])
            valid = bool(np.isfinite(s["cand_cost"]) and np.isfinite(s["model"]) and s["model"] > 0)
            if valid:
                x2 = float(np.sum(lin["poses"] ** 2))
                if np.linalg.norm(s["delta"]) <= p["parameter_tolerance"] * (np.sqrt(x2) + p["parameter_tolerance"]):
                    rec.update(outcome="parameter", cost=float(lin["cost"]), radius_after=radius)
                    end["termination"] = "parameter"; break
        if not valid:
            end["invalid_steps"] += 1
            invalid += 1
            rec.update(outcome="invalid", cost=float(lin["cost"]))
            if invalid >= p["max_consecutive_invalid_steps"]:
                rec["radius_after"] = radius
                end["termination"] = "invalid_steps"; break
            radius /= factor
            factor *= 2.0
            rec["radius_after"] = radius
            continue
        invalid = 0
        rho = float(s["rho"])
        rec["rho"] = rho
        if rho > p["min_relative_decrease"]:
            before = float(lin["cost"])
            change = before - float(s["cand_cost"])
            lin = linearise(c, s["cand"])
            end["accepted_steps"] += 1
            radius = float(new_radius(radius, rho, p["max_radius"]))
            factor = 2.0
            rec.update(outcome="accepted", cost=float(lin["cost"]), radius_after=radius)
            if abs(change) <= p["function_tolerance"] * before:
                end["termination"] = "function"; break
        else:
            end["rejected_steps"] += 1
            radius /= factor
            factor *= 2.0
            rec.update(outcome="rejected", cost=float(lin["cost"]), radius_after=radius)
    end.update(final_cost=float(lin["cost"]), radius=radius, poses=lin["poses"])
    return records, end


def step_of(before, after):
    """per node log(T_before^-1 T_after), [6n]: the step a call has taken, read off the poses"""
    return R.log(R.mul(R.inverse(before), after)).ravel()
