"""A numpy restatement of the pose graph's rules (include/sicp.h, "pose graph"), written from the formulas and batched over
edges.  Every function works in the dtype of its inputs, so the same code runs in float64 and in np.longdouble (the CPU test
measures the float64 rounding noise that way).

Poses are qt[..., 7] = [qx qy qz qw tx ty tz]; tangents are [upsilon; omega]; an edge (i, j, z, Omega) has
r = log(z^-1 T_i^-1 T_j), s = r^T Omega r, cost = 1/2 sum rho(s), and under T <- T exp(delta)
dr/d delta_j = Jr^-1(r), dr/d delta_i = -Jr^-1(r) Ad(T_j^-1 T_i)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LOSS_NONE, LOSS_CAUCHY = 0, 1
SERIES_THETA = 0.25  # below it every coefficient is its series in theta^2


def _f(dt, num, den=1):
    return dt.type(num) / dt.type(den)


def hat(v):
    o = np.zeros(v.shape[:-1] + (3, 3), dtype=v.dtype)
    o[..., 0, 1], o[..., 0, 2] = -v[..., 2], v[..., 1]
    o[..., 1, 0], o[..., 1, 2] = v[..., 2], -v[..., 0]
    o[..., 2, 0], o[..., 2, 1] = -v[..., 1], v[..., 0]
    return o


def rot(q):
    x, y, z, w = (q[..., k] for k in range(4))
    R = np.empty(q.shape[:-1] + (3, 3), dtype=q.dtype)
    R[..., 0, 0] = 1 - 2 * (y * y + z * z); R[..., 0, 1] = 2 * (x * y - w * z); R[..., 0, 2] = 2 * (x * z + w * y)
    R[..., 1, 0] = 2 * (x * y + w * z); R[..., 1, 1] = 1 - 2 * (x * x + z * z); R[..., 1, 2] = 2 * (y * z - w * x)
    R[..., 2, 0] = 2 * (x * z - w * y); R[..., 2, 1] = 2 * (y * z + w * x); R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def mul(a, b):
    ax, ay, az, aw = (a[..., k] for k in range(4))
    bx, by, bz, bw = (b[..., k] for k in range(4))
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                  aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)
    q = q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))
    t = a[..., 4:] + np.einsum("...ij,...j->...i", rot(a[..., :4]), b[..., 4:])
    return np.concatenate([q, t], axis=-1)


def inverse(a):
    q = a[..., :4] * np.array([-1, -1, -1, 1], dtype=a.dtype)
    t = -np.einsum("...ij,...j->...i", rot(q), a[..., 4:])
    return np.concatenate([q, t], axis=-1)


def _series(t2, coeffs):
    """sum coeffs[k] t2^k (Horner)"""
    v = np.zeros_like(t2) + coeffs[-1]
    for c in coeffs[-2::-1]:
        v = v * t2 + c
    return v


def coefficients(theta):
    """c of Jl_so3^-1 = I - Phi/2 + c Phi^2, and a1, a2, a3 of Barfoot's Q; series below SERIES_THETA"""
    dt = theta.dtype
    t2 = theta * theta
    small = theta < SERIES_THETA
    th = np.where(small, dt.type(1), theta)
    s, c = np.sin(th), np.cos(th)
    cc = 1 / (th * th) - (1 + c) / (2 * th * s)
    a1 = (th - s) / th ** 3
    a2 = (th * th + 2 * c - 2) / (2 * th ** 4)
    a3 = (2 * th - 3 * s + th * c) / (2 * th ** 5)
    fact = [dt.type(1)]
    for k in range(1, 17):
        fact.append(fact[-1] * k)
    bern = [_f(dt, 1, 6), _f(dt, 1, 30), _f(dt, 1, 42), _f(dt, 1, 30), _f(dt, 5, 66), _f(dt, 691, 2730)]  # |B_2n|
    cs = _series(t2, [bern[n] / fact[2 * n + 2] for n in range(6)])
    a1s = _series(t2, [(-1) ** k / fact[2 * k + 3] for k in range(6)])
    a2s = _series(t2, [(-1) ** k / fact[2 * k + 4] for k in range(6)])
    a3s = _series(t2, [(-1) ** k * (k + 1) / fact[2 * k + 5] for k in range(6)])
    return np.where(small, cs, cc), np.where(small, a1s, a1), np.where(small, a2s, a2), np.where(small, a3s, a3)


def exp(xi):
    """SE(3) exponential of [upsilon; omega]"""
    dt = xi.dtype
    u, w = xi[..., :3], xi[..., 3:]
    th = np.sqrt(np.sum(w * w, axis=-1))
    small = th < 1e-8
    ts = np.where(small, dt.type(1), th)
    half = np.where(small, _f(dt, 1, 2) - th * th / 48, np.sin(ts / 2) / ts)
    q = np.concatenate([w * half[..., None], np.cos(th / 2)[..., None]], axis=-1)
    b = np.where(small, _f(dt, 1, 2) - th * th / 24, (1 - np.cos(ts)) / (ts * ts))
    c = np.where(small, _f(dt, 1, 6) - th * th / 120, (ts - np.sin(ts)) / ts ** 3)
    W = hat(w)
    V = np.eye(3, dtype=dt) + b[..., None, None] * W + c[..., None, None] * (W @ W)
    return np.concatenate([q, np.einsum("...ij,...j->...i", V, u)], axis=-1)


def log(T):
    dt = T.dtype
    q = np.where(T[..., 3:4] < 0, -T[..., :4], T[..., :4])
    v, w = q[..., :3], q[..., 3]
    n = np.sqrt(np.sum(v * v, axis=-1))
    small = n < 1e-10
    ns = np.where(small, dt.type(1), n)
    f = np.where(small, 2 / w - _f(dt, 2, 3) * n * n / w ** 3, 2 * np.arctan2(ns, w) / ns)
    phi = v * f[..., None]
    th = np.sqrt(np.sum(phi * phi, axis=-1))
    c = coefficients(th)[0]
    F = hat(phi)
    Vi = np.eye(3, dtype=dt) - F / 2 + c[..., None, None] * (F @ F)
    return np.concatenate([np.einsum("...ij,...j->...i", Vi, T[..., 4:]), phi], axis=-1)


def jl_inv(xi):
    dt = xi.dtype
    rho, phi = xi[..., :3], xi[..., 3:]
    th = np.sqrt(np.sum(phi * phi, axis=-1))
    c, a1, a2, a3 = (k[..., None, None] for k in coefficients(th))
    F, P = hat(phi), hat(rho)
    A = np.eye(3, dtype=dt) - F / 2 + c * (F @ F)
    Q = (P / 2 + a1 * (F @ P + P @ F + F @ P @ F) + a2 * (F @ F @ P + P @ F @ F - 3 * (F @ P @ F))
         + a3 * (F @ P @ F @ F + F @ F @ P @ F))
    J = np.zeros(xi.shape[:-1] + (6, 6), dtype=dt)
    J[..., :3, :3] = A
    J[..., 3:, 3:] = A
    J[..., :3, 3:] = -(A @ Q @ A)
    return J


def jr_inv(xi):
    return jl_inv(-xi)


def adjoint(T):
    R = rot(T[..., :4])
    A = np.zeros(T.shape[:-1] + (6, 6), dtype=T.dtype)
    A[..., :3, :3] = R
    A[..., 3:, 3:] = R
    A[..., :3, 3:] = hat(T[..., 4:]) @ R
    return A


def residual(Ti, Tj, z):
    return log(mul(inverse(z), mul(inverse(Ti), Tj)))


def loss(kind, a, s):
    """rho(s), w = rho'(s)"""
    if kind == LOSS_CAUCHY:
        a2 = s.dtype.type(a) ** 2
        return a2 * np.log1p(s / a2), 1 / (1 + s / a2)
    return s, np.ones_like(s)


def edges(poses, ei, ej, z, omega, kind=LOSS_NONE, a=1.0):
    """the per-edge outputs: r, s, w, rho, Ji, Jj, Hi, Hj, B, gi, gj"""
    Ti, Tj = poses[ei], poses[ej]
    r = residual(Ti, Tj, z)
    s = np.einsum("ea,eab,eb->e", r, omega, r)
    rho, w = loss(kind, a, s)
    Jj = jr_inv(r)
    Ji = -Jj @ adjoint(mul(inverse(Tj), Ti))
    W = omega * w[:, None, None]
    t = lambda M: np.swapaxes(M, -1, -2)
    Wr = np.einsum("eab,eb->ea", W, r)
    return {"r": r, "s": s, "w": w, "rho": rho, "Ji": Ji, "Jj": Jj, "Hi": t(Ji) @ W @ Ji, "Hj": t(Jj) @ W @ Jj, "B": t(Ji) @ W @ Jj,
            "gi": np.einsum("eba,eb->ea", Ji, Wr), "gj": np.einsum("eba,eb->ea", Jj, Wr)}


def node_sums(n, fixed, ei, ej, E):
    """gradient [n, 6] and diagonal blocks [n, 6, 6]: a fixed node has the identity and zero, a node without edges zeros"""
    H = np.zeros((n, 6, 6), dtype=E["r"].dtype)
    g = np.zeros((n, 6), dtype=E["r"].dtype)
    np.add.at(H, ei, E["Hi"]); np.add.at(H, ej, E["Hj"])
    np.add.at(g, ei, E["gi"]); np.add.at(g, ej, E["gj"])
    H[fixed] = np.eye(6)
    g[fixed] = 0
    return g, H


def assemble(poses, fixed, ei, ej, z, omega, kind=LOSS_NONE, a=1.0):
    """(cost, g [6n], H sparse [6n, 6n]) of the normal equations with the rules for fixed nodes"""
    n = len(poses)
    fixed = np.asarray(fixed, dtype=bool)
    E = edges(poses, ei, ej, z, omega, kind, a)
    g, D = node_sums(n, fixed, ei, ej, E)
    k6 = np.arange(6)
    rows = (6 * np.arange(n)[:, None, None] + k6[None, :, None]) + 0 * k6[None, None, :]
    cols = (6 * np.arange(n)[:, None, None] + k6[None, None, :]) + 0 * k6[None, :, None]
    R, Cc, V = [rows.ravel()], [cols.ravel()], [D.ravel()]
    free = ~fixed[ei] & ~fixed[ej]
    bi, bj, B = ei[free], ej[free], E["B"][free]
    r = 6 * bi[:, None, None] + k6[None, :, None] + 0 * k6[None, None, :]
    c = 6 * bj[:, None, None] + k6[None, None, :] + 0 * k6[None, :, None]
    R += [r.ravel(), c.ravel()]; Cc += [c.ravel(), r.ravel()]; V += [B.ravel(), B.ravel()]
    H = sp.coo_matrix((np.concatenate(V).astype(np.float64), (np.concatenate(R), np.concatenate(Cc))), shape=(6 * n, 6 * n)).tocsc()
    return 0.5 * float(np.sum(E["rho"])), g.ravel().astype(np.float64), H


def cost(poses, ei, ej, z, omega, kind=LOSS_NONE, a=1.0):
    r = residual(poses[ei], poses[ej], z)
    return 0.5 * float(np.sum(loss(kind, a, np.einsum("ea,eab,eb->e", r, omega, r))[0]))


def retract(poses, fixed, delta):
    out = mul(poses, exp(delta.reshape(-1, 6)))
    keep = np.asarray(fixed, dtype=bool) | np.all(delta.reshape(-1, 6) == 0, axis=1)
    out[keep] = poses[keep]
    return out


def minimise(poses, fixed, ei, ej, z, omega, kind=LOSS_NONE, a=1.0, initial_radius=1e4, rel_gradient=1e-12, max_iterations=300,
             min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32):
    """The reference minimiser: Levenberg-Marquardt with a sparse direct solve of the full damped system, under the step control
    of the issue, until max |g| <= rel_gradient * (the initial max |g|).  Returns (poses, info)."""
    x = np.array(poses, dtype=np.float64)
    c, g, H = assemble(x, fixed, ei, ej, z, omega, kind, a)
    g0 = np.max(np.abs(g))
    radius, factor = initial_radius, 2.0
    info = {"iterations": 0, "accepted": 0, "rejected": 0, "converged": False, "first_step_rejected": None, "initial_cost": c}
    while info["iterations"] < max_iterations:
        if np.max(np.abs(g)) <= rel_gradient * g0:
            info["converged"] = True
            break
        if radius < 1e-32:  # (stalled: the cost's own rounding hides any further decrease)
            break
        info["iterations"] += 1
        D = np.clip(H.diagonal(), min_lm_diagonal, max_lm_diagonal) / radius
        delta = spla.spsolve((H + sp.diags(D)).tocsc(), -g)
        model = -(g @ delta) - 0.5 * (delta @ (H @ delta))
        cand = retract(x, fixed, delta)
        cc = cost(cand, ei, ej, z, omega, kind, a)
        rho = (c - cc) / model if model > 0 and np.isfinite(cc) else -1.0
        if info["first_step_rejected"] is None:
            info["first_step_rejected"] = not rho > min_relative_decrease
        if rho > min_relative_decrease:
            x = cand
            c, g, H = assemble(x, fixed, ei, ej, z, omega, kind, a)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            factor = 2.0
            info["accepted"] += 1
        else:
            radius /= factor
            factor *= 2.0
            info["rejected"] += 1
    # Where the cost is large (outliers under a quadratic loss) its rounding, eps * cost, hides the decrease of a step long
    # before the gradient is down by 1e-12: sqrt(eps * cost * lambda_max) is what the acceptance test can reach.  From there
    # the steps are taken on the gradient's word alone: Gauss-Newton steps, kept while max |g| falls -- also beyond the 1e-12,
    # down to the gradient's own rounding, so that the reference's distance from the minimum is small next to any tolerance a
    # test gives the code under test.
    while info["iterations"] < max_iterations:
        info["iterations"] += 1
        D = np.clip(H.diagonal(), min_lm_diagonal, max_lm_diagonal) * 1e-12
        cand = retract(x, fixed, spla.spsolve((H + sp.diags(D)).tocsc(), -g))
        cc, gc, Hc = assemble(cand, fixed, ei, ej, z, omega, kind, a)
        if not np.max(np.abs(gc)) < np.max(np.abs(g)):
            break
        x, c, g, H = cand, cc, gc, Hc
        info["polish"] = info.get("polish", 0) + 1
        info["converged"] = info["converged"] or bool(np.max(np.abs(g)) <= rel_gradient * g0)
    info.update(cost=c, gradient_max_norm=float(np.max(np.abs(g))), g=g, H=H)
    return x, info


def tangent_distance(a, b):
    """|log(a^-1 b)| over all nodes"""
    return float(np.linalg.norm(log(mul(inverse(a), b))))
