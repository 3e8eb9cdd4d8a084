"""A numpy restatement of the pose graph's priors and enabled flags (include/sicp.h, "pose graph", rules 5 - 12), on top of
pose_graph_ref, which it imports unchanged.

Priors are a dict: node [P] int32, kind [P] (POSE = 0, POSITION = 1), z [P, 7], omega [P, 6, 6].  A pose prior uses all of z and
omega; a position prior keeps its point in z[:3] and its 3x3 information in omega[:3, :3] (the rest is ignored).
    pose      r = log(z^-1 T_k),  dr / d delta_k = Jr^-1(r)
    position  r = t_k - p,        dr / d delta_k = [R_k | 0]
s = r^T Omega r, the graph's loss, the block w J^T Omega J and the gradient w J^T Omega r.  A disabled edge or prior contributes
to nothing.  For pose priors there is a second oracle that needs none of this file's algebra: identity_twin() turns each into an
ordinary edge from one extra node fixed at the identity pose, for the unchanged pose_graph_ref.assemble / minimise."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import pose_graph_ref as R

POSE, POSITION = 0, 1
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0.0])


def make(node, kind, z, omega):
    """priors from per-prior rows: z rows of 7 (pose) or 3 (position), omega 6x6 or 3x3"""
    P = len(node)
    Z, Om = np.zeros((P, 7)), np.zeros((P, 6, 6))
    for p in range(P):
        zz, oo = np.asarray(z[p], dtype=np.float64), np.asarray(omega[p], dtype=np.float64)
        Z[p, :len(zz)] = zz
        Om[p, :oo.shape[0], :oo.shape[1]] = oo
    return dict(node=np.asarray(node, dtype=np.int32), kind=np.asarray(kind, dtype=np.int32), z=Z, omega=Om)


def none():
    return make([], [], [], [])


def pose_residual(T, z):
    return R.log(R.mul(R.inverse(z), T))


def position_residual(T, p):
    return T[..., 4:] - p


def jacobians(poses, pri):
    """dr / d delta_k of every prior, [P, 6, 6]: a position prior's 3x6 in the first three rows, zeros below"""
    T = poses[pri["node"]]
    pos = pri["kind"] == POSITION
    J = np.zeros((len(T), 6, 6), dtype=poses.dtype)
    if (~pos).any():
        J[~pos] = R.jr_inv(pose_residual(T[~pos], pri["z"][~pos].astype(poses.dtype)))
    if pos.any():
        J[pos, :3, :3] = R.rot(T[pos, :4])
    return J


def priors(poses, pri, kind=R.LOSS_NONE, a=1.0):
    """the per-prior outputs: r [P, 6] (a position prior: r, then zeros), s, w, rho, J, H [P, 6, 6], g [P, 6]"""
    dt = poses.dtype
    T = poses[pri["node"]]
    P = len(T)
    pos = pri["kind"] == POSITION
    z, om = pri["z"].astype(dt), pri["omega"].astype(dt).copy()
    om[pos, 3:, :] = 0
    om[pos, :, 3:] = 0
    r = np.zeros((P, 6), dtype=dt)
    if (~pos).any():
        r[~pos] = pose_residual(T[~pos], z[~pos])
    if pos.any():
        r[pos, :3] = position_residual(T[pos], z[pos, :3])
    s = np.einsum("pa,pab,pb->p", r, om, r)
    rho, w = R.loss(kind, a, s)
    J = jacobians(poses, pri)
    W = om * w[:, None, None]
    Jt = np.swapaxes(J, -1, -2)
    return {"r": r, "s": s, "w": w, "rho": rho, "J": J, "H": Jt @ W @ J, "g": np.einsum("pba,pb->pa", J, np.einsum("pab,pb->pa", W, r))}


def floors(T, pri):
    """pose_graph_cases.floors for priors: the size of what a block is formed from"""
    pos = pri["kind"] == POSITION
    zt = np.where(pos[:, None], pri["z"][:, :3], pri["z"][:, 4:])
    size = np.maximum(1.0, np.max(np.abs(np.concatenate([T[:, 4:], zt], axis=1)), axis=1))
    om = np.where(pos, np.abs(pri["omega"][:, :3, :3]).reshape(len(T), -1).max(axis=1), np.abs(pri["omega"]).reshape(len(T), -1).max(axis=1))
    return {"r": size, "s": om * size ** 2, "rho": om * size ** 2, "w": 1.0 + 0 * size, "g": om * size, "H": 0 * size}


def _masks(m, P, e_on, p_on):
    e_on = np.ones(m, dtype=bool) if e_on is None else np.asarray(e_on, dtype=bool)
    p_on = np.ones(P, dtype=bool) if p_on is None else np.asarray(p_on, dtype=bool)
    return e_on, p_on


def node_sums(g, pri, E, PE, e_on=None, p_on=None):
    """gradient [n, 6] and diagonal blocks [n, 6, 6] over the enabled edges and priors; a fixed node: the identity and zero"""
    e_on, p_on = _masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    n = len(g["poses"])
    Ee = {k: v[e_on] for k, v in E.items()}
    grad, H = R.node_sums(n, np.zeros(n, dtype=bool), g["ei"][e_on], g["ej"][e_on], Ee)
    np.add.at(H, pri["node"][p_on], PE["H"][p_on])
    np.add.at(grad, pri["node"][p_on], PE["g"][p_on])
    fixed = np.asarray(g["fixed"], dtype=bool)
    H[fixed] = np.eye(6)
    grad[fixed] = 0
    return grad, H


def assemble(poses, g, pri, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0):
    """(cost, g [6n], H sparse [6n, 6n]) over the enabled edges and priors, with the rules for fixed nodes"""
    e_on, p_on = _masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    fixed = np.asarray(g["fixed"], dtype=bool)
    n = len(poses)
    c, grad, H = R.assemble(poses, fixed, g["ei"][e_on], g["ej"][e_on], g["z"][e_on], g["omega"][e_on], kind, a)
    PE = priors(poses, pri, kind, a)
    c += 0.5 * float(PE["rho"][p_on].sum())
    free = p_on & ~fixed[pri["node"]]
    grad = grad.reshape(n, 6).copy()
    np.add.at(grad, pri["node"][free], PE["g"][free])
    k6 = np.arange(6)
    nodes = pri["node"][free]
    rows = (6 * nodes[:, None, None] + k6[None, :, None]) + 0 * k6[None, None, :]
    cols = (6 * nodes[:, None, None] + k6[None, None, :]) + 0 * k6[None, :, None]
    H = (H + sp.coo_matrix((PE["H"][free].ravel().astype(np.float64), (rows.ravel(), cols.ravel())), shape=(6 * n, 6 * n))).tocsc()
    return c, grad.ravel(), H


def cost(poses, g, pri, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0):
    e_on, p_on = _masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    c = R.cost(poses, g["ei"][e_on], g["ej"][e_on], g["z"][e_on], g["omega"][e_on], kind, a)
    return c + 0.5 * float(priors(poses, pri, kind, a)["rho"][p_on].sum())


def minimise(g, pri, e_on=None, p_on=None, kind=R.LOSS_NONE, a=1.0, poses=None, initial_radius=1e4, rel_gradient=1e-12, max_iterations=300,
             min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """pose_graph_ref.minimise's Levenberg-Marquardt (the same step control, the same polish on the gradient's word) on the cost
    with priors and flags.  Returns (poses, info)."""
    fixed = np.asarray(g["fixed"], dtype=bool)
    x = np.array(g["poses"] if poses is None else poses, dtype=np.float64)
    c, grad, H = assemble(x, g, pri, e_on, p_on, kind, a)
    g0 = np.max(np.abs(grad))
    radius, factor = initial_radius, 2.0
    info = {"iterations": 0, "accepted": 0, "rejected": 0, "converged": False, "initial_cost": c}
    while info["iterations"] < max_iterations:
        if np.max(np.abs(grad)) <= rel_gradient * g0:
            info["converged"] = True
            break
        if radius < 1e-32:
            break
        info["iterations"] += 1
        D = np.clip(H.diagonal(), min_lm_diagonal, max_lm_diagonal) / radius
        delta = spla.spsolve((H + sp.diags(D)).tocsc(), -grad)
        model = -(grad @ delta) - 0.5 * (delta @ (H @ delta))
        cand = R.retract(x, fixed, delta)
        cc = cost(cand, g, pri, e_on, p_on, kind, a)
        rho = (c - cc) / model if model > 0 and np.isfinite(cc) else -1.0
        if rho > min_relative_decrease:
            x = cand
            c, grad, H = assemble(x, g, pri, e_on, p_on, kind, a)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            factor = 2.0
            info["accepted"] += 1
        else:
            radius /= factor
            factor *= 2.0
            info["rejected"] += 1
    while info["iterations"] < max_iterations:  # (the polish of pose_graph_ref.minimise)
        info["iterations"] += 1
        D = np.clip(H.diagonal(), min_lm_diagonal, max_lm_diagonal) * 1e-12
        cand = R.retract(x, fixed, spla.spsolve((H + sp.diags(D)).tocsc(), -grad))
        cc, gc, Hc = assemble(cand, g, pri, e_on, p_on, kind, a)
        if not np.max(np.abs(gc)) < np.max(np.abs(grad)):
            break
        x, c, grad, H = cand, cc, gc, Hc
        info["converged"] = info["converged"] or bool(np.max(np.abs(grad)) <= rel_gradient * g0)
    info.update(cost=c, gradient_max_norm=float(np.max(np.abs(grad))), g=grad, H=H)
    return x, info


def identity_twin(g, pri, e_on=None, p_on=None):
    """The graph with one extra node, fixed at the identity pose, and every enabled POSE prior (k, z, Omega) as the ordinary edge
    (extra, k, z, Omega); the disabled edges left out.  For the unchanged pose_graph_ref."""
    e_on, p_on = _masks(len(g["ei"]), len(pri["node"]), e_on, p_on)
    assert not (pri["kind"][p_on] == POSITION).any(), "a position prior is no edge"
    n = len(g["poses"])
    return dict(poses=np.concatenate([g["poses"], IDENTITY[None]]), fixed=np.append(np.asarray(g["fixed"], dtype=bool), True),
                ei=np.concatenate([g["ei"][e_on], np.full(int(p_on.sum()), n)]).astype(np.int32),
                ej=np.concatenate([g["ej"][e_on], pri["node"][p_on]]).astype(np.int32),
                z=np.concatenate([g["z"][e_on], pri["z"][p_on]]), omega=np.concatenate([g["omega"][e_on], pri["omega"][p_on]]))


def add_to(pg, pri):
    """the priors into a PoseGraph, in id order (runs of one kind per call); returns the first id"""
    first, P = None, len(pri["node"])
    p = 0
    while p < P:
        q = p
        while q < P and pri["kind"][q] == pri["kind"][p]:
            q += 1
        if pri["kind"][p] == POSITION:
            got = pg.add_priors(pri["node"][p:q], pri["z"][p:q, :3], np.ascontiguousarray(pri["omega"][p:q, :3, :3]), kind=POSITION)
        else:
            got = pg.add_priors(pri["node"][p:q], pri["z"][p:q], pri["omega"][p:q], kind=POSE)
        assert got == p
        first = got if first is None else first
        p = q
    return first
