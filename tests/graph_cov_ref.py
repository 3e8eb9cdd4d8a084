"""A numpy / scipy restatement of the pose-graph covariances (include/sicp.h, "pose-graph covariances"), built on
pose_graph_ref.assemble and the graphs of pose_graph_cases.

A query is a pair (a, b) of nodes, a = -1 for a marginal.  J has the block J_a = -Ad(T_b^-1 T_a) at a and the identity at b (a
fixed end has no block); cov = J H^-1 J^T with H the undamped Gauss-Newton matrix, a fixed node's block the identity, and an
identity block for every free node without edges.  reference() solves with a sparse LU; pcg() restates the lock-step
preconditioned conjugate gradients of the kernels: per-column scalars, and a column that is done is frozen."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph
import scipy.sparse.linalg as spla

import pose_graph_ref as R

OK, NOT_CONVERGED, UNANCHORED, BREAKDOWN = 0, 1, 2, 3


def degrees(g):
    return np.bincount(np.concatenate([g["ei"], g["ej"]]), minlength=len(g["poses"]))


def anchored(g):
    """per node: its connected component holds a fixed node"""
    n = len(g["poses"])
    A = sp.coo_matrix((np.ones(len(g["ei"])), (g["ei"], g["ej"])), shape=(n, n))
    _, comp = csgraph.connected_components(A, directed=False)
    has = np.zeros(comp.max() + 1, dtype=bool)
    has[comp[np.asarray(g["fixed"], dtype=bool)]] = True
    return has[comp]


def system(g, kind=R.LOSS_NONE, a=1.0, poses=None):
    """H (sparse, 6N x 6N) with identity blocks for the free nodes without edges"""
    poses = g["poses"] if poses is None else poses
    _, _, H = R.assemble(poses, g["fixed"], g["ei"], g["ej"], g["z"], g["omega"], kind, a)
    lone = ~np.asarray(g["fixed"], dtype=bool) & (degrees(g) == 0)
    return (H + sp.diags(np.repeat(lone.astype(np.float64), 6))).tocsc()


def jacobian_a(Ta, Tb):
    """J_a = -Ad(T_b^-1 T_a)"""
    return -R.adjoint(R.mul(R.inverse(Tb), Ta))


def jacobian(g, qa, qb, poses=None):
    """J of every query, dense [nq, 6, 6N]; a fixed end has no block"""
    poses = g["poses"] if poses is None else poses
    fixed = np.asarray(g["fixed"], dtype=bool)
    n = len(poses)
    J = np.zeros((len(qb), 6, 6 * n))
    for q, (a, b) in enumerate(zip(qa, qb)):
        if not fixed[b]:
            J[q, :, 6 * b:6 * b + 6] = np.eye(6)
        if a >= 0 and not fixed[a]:
            J[q, :, 6 * a:6 * a + 6] = jacobian_a(poses[a], poses[b])
    return J


def statuses(g, qa, qb):
    fixed, anch = np.asarray(g["fixed"], dtype=bool), anchored(g)
    st = np.zeros(len(qb), dtype=np.int32)
    for q, (a, b) in enumerate(zip(qa, qb)):
        ends = [b] + ([a] if a >= 0 else [])
        if any(not fixed[k] and not anch[k] for k in ends):
            st[q] = UNANCHORED
    return st


def symmetrise(S):
    return 0.5 * (S + np.swapaxes(S, -1, -2))


def _kept(g):
    """the nodes of the system that is solved: the anchored components and the lone free nodes (an unanchored component's
    right-hand sides are zero, and its part of H is singular)"""
    fixed = np.asarray(g["fixed"], dtype=bool)
    return np.repeat(anchored(g) | (~fixed & (degrees(g) == 0)), 6)


def reference(g, qa, qb, kind=R.LOSS_NONE, a=1.0, poses=None):
    """(cov [nq, 6, 6], status [nq], H): sparse LU solves of J^T; NaN where the status is UNANCHORED"""
    H = system(g, kind, a, poses)
    keep = _kept(g)
    lu = spla.splu(H[keep][:, keep].tocsc())
    J = jacobian(g, qa, qb, poses)
    st = statuses(g, qa, qb)
    cov = np.full((len(qb), 6, 6), np.nan)
    for q in range(len(qb)):
        if st[q] == OK:
            Jk = J[q][:, keep]
            cov[q] = symmetrise(Jk @ lu.solve(np.ascontiguousarray(Jk.T)))
    return cov, st, H


def lambda_min(H):
    if H.shape[0] <= 1200:
        return float(np.linalg.eigvalsh(H.toarray())[0])
    return float(spla.eigsh(H, k=1, sigma=0, which="LM", return_eigenvectors=False)[0])


def bound(J, tolerance, lam_min):
    """The a-priori bound of the stopping rule on an entry of J X: column k has |r| <= tolerance |b_k|, so
    |x - x*| <= tolerance |b_k| / lambda_min with |b_k| = |row k of J|, and an entry of J (x - x*) is at most |J|_2 times that."""
    rows = np.sqrt((J * J).sum(axis=1)).max()
    return float(np.linalg.norm(J, 2) * tolerance * rows / lam_min)


def pcg(H, B, tolerance=1e-10, max_iterations=None):
    """Lock-step block-Jacobi PCG on the columns of B: (X, flag [m], iterations [m]) with flag 1 = converged, 2 = breakdown,
    3 = the iteration limit.  Every column has its own alpha, beta and r.z; a column whose flag is set is no longer written."""
    n6, m = B.shape
    n = n6 // 6
    bsr = H.tobsr(blocksize=(6, 6))
    rows = np.repeat(np.arange(n), np.diff(bsr.indptr))
    on_diagonal = bsr.indices == rows
    blocks = np.zeros((n, 6, 6))
    blocks[rows[on_diagonal]] = bsr.data[on_diagonal]
    Minv = np.linalg.inv(blocks)
    H = H.tocsr()
    apply = lambda V: np.matmul(Minv, V.reshape(n, 6, -1)).reshape(n6, -1)
    limit = max(20 * n, 200) if max_iterations is None else max_iterations
    B = np.ascontiguousarray(B)
    X, Rr = np.zeros_like(B), B.copy()
    Z = apply(Rr)
    P = Z.copy()
    rz, bb = (Rr * Z).sum(axis=0), (Rr * Rr).sum(axis=0)
    flag, iters = np.zeros(m, dtype=int), np.zeros(m, dtype=int)
    flag[bb == 0] = 1
    while True:
        act = np.flatnonzero(flag == 0)
        if len(act) == 0:
            break
        Pa = P if len(act) == m else P[:, act]
        Q = H @ Pa
        pq = (Pa * Q).sum(axis=0)
        bad = ~np.isfinite(pq) | ~(pq > 0)
        if bad.any():
            flag[act[bad]] = 2
            act, Q, pq = act[~bad], Q[:, ~bad], pq[~bad]
        cols = slice(None) if len(act) == m else act  # (all columns: views instead of gathered copies)
        alpha = rz[act] / pq
        X[:, cols] += alpha * P[:, cols]
        Rr[:, cols] -= alpha * Q
        Zc = apply(Rr[:, cols])
        Z[:, cols] = Zc
        new_rz, rr = (Rr[:, cols] * Zc).sum(axis=0), (Rr[:, cols] * Rr[:, cols]).sum(axis=0)
        bad = ~np.isfinite(new_rz) | ~np.isfinite(rr)
        flag[act[bad]] = 2
        beta = np.where(bad, 0.0, new_rz / rz[act])
        rz[act] = new_rz
        iters[act[~bad]] += 1
        done = ~bad & (np.sqrt(rr) <= tolerance * np.sqrt(bb[act]))
        flag[act[done]] = 1
        flag[act[~bad & ~done & (iters[act] >= limit)]] = 3
        go = flag[act] == 0
        if go.all() and len(act) == m:
            P *= beta
            P += Z
        else:
            P[:, act[go]] = Z[:, act[go]] + beta[go] * P[:, act[go]]
    return X, flag, iters


def restated(g, qa, qb, kind=R.LOSS_NONE, a=1.0, tolerance=1e-10, max_iterations=None, poses=None):
    """the kernels' method in numpy: (cov, status, iterations of the longest column)"""
    H = system(g, kind, a, poses)
    J = jacobian(g, qa, qb, poses)
    st = statuses(g, qa, qb)
    cov = np.full((len(qb), 6, 6), np.nan)
    fixed = np.asarray(g["fixed"], dtype=bool)
    for q, (qa_, qb_) in enumerate(zip(qa, qb)):
        if st[q] == OK and fixed[qb_] and (qa_ < 0 or fixed[qa_]):
            cov[q] = 0.0
    todo = [q for q in range(len(qb)) if st[q] == OK and np.isnan(cov[q, 0, 0])]
    longest = 0
    if todo:
        B = np.concatenate([J[q].T for q in todo], axis=1)
        X, flag, iters = pcg(H, B, tolerance, max_iterations)
        longest = int(iters.max())
        for k, q in enumerate(todo):
            f = flag[6 * k:6 * k + 6]
            st[q] = BREAKDOWN if (f == 2).any() else NOT_CONVERGED if (f != 1).any() else OK
            if st[q] != BREAKDOWN:
                cov[q] = symmetrise(J[q] @ X[:, 6 * k:6 * k + 6])
    return cov, st, longest


def queries(g, seed, pairs=4):
    """`pairs` random pairs of distinct nodes plus one pair that ends at the (first) fixed node: (qa, qb) int32"""
    rng = np.random.default_rng(seed)
    n = len(g["poses"])
    qa, qb = [], []
    for _ in range(pairs):
        a, b = rng.choice(n, size=2, replace=False)
        qa.append(int(a)); qb.append(int(b))
    f = int(np.flatnonzero(g["fixed"])[0])
    qa.append(int((f + 1 + rng.integers(0, n - 1)) % n)); qb.append(f)
    return np.array(qa, dtype=np.int32), np.array(qb, dtype=np.int32)


# ---- the cases of the CPU and the GPU tests: name -> (graph, loss, cauchy_a, queries) ---------------------------------------------
def _cases():
    import pose_graph_cases as cases

    return {
        "two_nodes": (lambda: cases.two_nodes(), R.LOSS_NONE, 1.0),
        "triangle": (lambda: cases.triangle(), R.LOSS_NONE, 1.0),
        "chain_and_lone_node": (lambda: cases.chain(), R.LOSS_NONE, 1.0),
        "ring65_8_closures": (lambda: cases.ring(closures=8), R.LOSS_NONE, 1.0),
        "hub300": (lambda: cases.hub(), R.LOSS_NONE, 1.0),
        "counted300": (lambda: cases.counted(300), R.LOSS_NONE, 1.0),
        "ring65_cauchy_outliers": (lambda: cases.ring(closures=6, outliers=2), R.LOSS_CAUCHY, 1.5),
        "hub11000": (lambda: cases.hub(spokes=11000), R.LOSS_NONE, 1.0),
    }


CASE_NAMES = tuple(_cases())


def case(name):
    """(graph, loss, cauchy_a, qa, qb): 4 random pairs and one that ends at the fixed node; the chain's lone node is asked for too"""
    make, kind, a = _cases()[name]
    g = make()
    qa, qb = queries(g, seed=100 + CASE_NAMES.index(name))
    if name == "chain_and_lone_node":
        lone = len(g["poses"]) - 1
        qa, qb = np.append(qa, [lone, 0]).astype(np.int32), np.append(qb, [0, lone]).astype(np.int32)
    return g, kind, a, qa, qb
