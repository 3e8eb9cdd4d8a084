"""numpy restatement of sicp_segment_planes (include/sicp.h, "planes of a cloud", rules 1 - 6).  Imports nothing of the product.

Every operation is a float64 operation of numpy or of Python's float, rounded on its own in the order the rules give; the
Jacobi is restated rotation by rotation, operation by operation.  fits() keeps, per refined plane, the matrix the Jacobi was
given and the normal it returned, for the CPU test that holds the restated solver against np.linalg.eigh."""
import math

import numpy as np

import filter_ref

MAX_HYPOTHESES = 4096
MAX_PLANES = 16
MAX_IGNORE = 16
LANE_POINTS = 4
TILE = 256 * LANE_POINTS  # candidates one workgroup of the score kernel tests (the shapes the GPU tests straddle; no rule depends on it)
HYP_GROUP = 64            # hypotheses one workgroup of the score kernel loops over (likewise)
TREE_RUN = 512            # caller indices one workgroup of a tree sum reduces, level over level (likewise)
GOLDEN = 0x9E3779B97F4A7C15
DEFAULTS = dict(distance_threshold=0.2, axis=None, min_cos=0.0, seed=1, num_hypotheses=1024, max_planes=1, min_inliers=100, refine=1,
                ignore=())


class TooFewPoints(ValueError):
    pass


def draws(seed, first, count):
    """rule 2: draws first .. first + count of the SplitMix64 stream seeded with `seed`, as uint64"""
    k = np.arange(first, first + count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & ((1 << 64) - 1)) + (k + np.uint64(1)) * np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sample_indices(seed, r, H, m):
    """rule 2: [H, 3] indices into cand"""
    z = draws(seed, 3 * r * H, 3 * H)
    u = (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    j = np.floor(np.float64(m) * u).astype(np.int64)
    return np.minimum(j, m - 1).reshape(H, 3)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def hypotheses(P, idx, tt, axis, min_cos):
    """rule 2: a [H, 3], n [H, 3], nn [H], thr [H] = (t t) nn, valid [H] of the sampled rows idx [H, 3] of P (float64)"""
    a, b, c = P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    nn = dot3(n[:, 0], n[:, 1], n[:, 2], n[:, 0], n[:, 1], n[:, 2])
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2]) & (nn > 0.0)
    if axis is not None:
        ax, ay, az = (np.float64(v) for v in axis)
        aa = dot3(ax, ay, az, ax, ay, az)
        na = dot3(n[:, 0], n[:, 1], n[:, 2], ax, ay, az)
        mc = np.float64(min_cos)
        valid &= na * na >= ((mc * mc) * nn) * aa
    return a, n, nn, tt * nn, valid


def inliers(P, a, n, thr):
    """rule 3: the test of every row of P against one plane"""
    d = P - a
    e = (n[0] * d[:, 0] + n[1] * d[:, 1]) + n[2] * d[:, 2]
    return e * e <= thr, e


def scores(P, a, n, thr, valid, chunk=64):
    """rule 3: the inlier count of every hypothesis over the rows of P (0 for an invalid one)"""
    H = len(a)
    out = np.zeros(H, np.int64)
    for h0 in range(0, H, chunk):
        A, N = a[h0:h0 + chunk], n[h0:h0 + chunk]
        dx = P[None, :, 0] - A[:, None, 0]
        dy = P[None, :, 1] - A[:, None, 1]
        dz = P[None, :, 2] - A[:, None, 2]
        e = (N[:, None, 0] * dx + N[:, None, 1] * dy) + N[:, None, 2] * dz
        out[h0:h0 + chunk] = (e * e <= thr[h0:h0 + chunk, None]).sum(axis=1)
    out[~valid] = 0
    return out


def tree(values, present, n_points):
    """rules 5 and 6: the filter's tree sum with +0.0 added once"""
    return filter_ref.tree_sum(values, present, n_points) + 0.0


def jacobi_rotate(A, V, p, q):
    """one rotation of the cyclic Jacobi (A := J^T A J, V := V J), every operation a float64 operation of its own"""
    apq = A[p][q]
    if apq == 0.0:
        return
    tau = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = (1.0 if tau >= 0 else -1.0) / (abs(tau) + math.sqrt(1.0 + tau * tau))
    c = 1.0 / math.sqrt(1.0 + t * t)
    s = t * c
    for k in range(3):
        akp, akq = A[k][p], A[k][q]
        A[k][p] = c * akp - s * akq
        A[k][q] = s * akp + c * akq
    for k in range(3):
        apk, aqk = A[p][k], A[q][k]
        A[p][k] = c * apk - s * aqk
        A[q][k] = s * apk + c * aqk
    for k in range(3):
        vkp, vkq = V[k][p], V[k][q]
        V[k][p] = c * vkp - s * vkq
        V[k][q] = s * vkp + c * vkq


def smallest_eigenvector(Q):
    """rule 5: Q = (xx, yx, yy, zx, zy, zz) -> the eigenvector column of smallest |eigenvalue|, the last one at ties"""
    Q = [float(v) for v in Q]
    A = [[Q[0], Q[1], Q[3]], [Q[1], Q[2], Q[4]], [Q[3], Q[4], Q[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(30):
        off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2]
        dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2]
        if off <= 1e-300 or off <= 1e-34 * dia:
            break
        jacobi_rotate(A, V, 0, 1)
        jacobi_rotate(A, V, 0, 2)
        jacobi_rotate(A, V, 1, 2)
    e = [abs(A[0][0]), abs(A[1][1]), abs(A[2][2])]
    col, em = 0, e[0]
    if e[1] <= em:
        em, col = e[1], 1
    if e[2] <= em:
        em, col = e[2], 2
    return [V[0][col], V[1][col], V[2][col]]


def orient(c, axis):
    """rules 4 and 5: coeff (4 floats) with its sign fixed"""
    s = 0.0
    if axis is not None:
        s = (c[0] * float(axis[0]) + c[1] * float(axis[1])) + c[2] * float(axis[2])
    flip = s < 0.0
    if s == 0.0:
        flip = next((v < 0.0 for v in (c[3], c[2], c[1], c[0]) if v != 0.0), False)
    return [-v for v in c] if flip else list(c)


def check_params(labels, distance_threshold, axis, min_cos, num_hypotheses, max_planes, min_inliers, refine, ignore):
    """rule 7's ranges; returns the axis as None or three floats"""
    if not (math.isfinite(distance_threshold) and distance_threshold > 0.0):
        raise ValueError("distance_threshold")
    if axis is not None:
        axis = [float(v) for v in axis]
        if not all(math.isfinite(v) for v in axis):
            raise ValueError("axis")
        if all(v == 0.0 for v in axis):
            axis = None
    if axis is None and min_cos != 0.0:
        raise ValueError("min_cos without an axis")
    if axis is not None and not (0.0 < min_cos <= 1.0):
        raise ValueError("min_cos")
    if not 1 <= num_hypotheses <= MAX_HYPOTHESES or not 1 <= max_planes <= MAX_PLANES or min_inliers < 3 or refine not in (0, 1):
        raise ValueError("a count")
    if len(ignore) > MAX_IGNORE or (labels is None and len(ignore)):
        raise ValueError("ignore")
    return axis


def segment_planes(xyz, labels=None, mask=None, distance_threshold=0.2, axis=None, min_cos=0.0, seed=1, num_hypotheses=1024, max_planes=1,
                   min_inliers=100, refine=1, ignore=()):
    """the call: {"plane_id", "coeff", "count", "hyp_index", "hyp_count", "centroid", "rms", the fields of sicp_plane_info,
    "fits": per refined plane (Q, S, normal before orientation)}"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n_points = len(xyz)
    axis = check_params(labels, distance_threshold, axis, min_cos, num_hypotheses, max_planes, min_inliers, refine, ignore)
    finite = np.isfinite(xyz).all(axis=1)
    cand0 = finite.copy()
    if mask is not None:
        cand0 &= np.asarray(mask).reshape(n_points) != 0
    if labels is not None and len(ignore):
        cand0 &= ~np.isin(np.asarray(labels, np.uint32), np.asarray(list(ignore), np.uint32))
    if cand0.sum() < 3:
        raise TooFewPoints(int(cand0.sum()))
    P64 = np.where(finite[:, None], xyz, np.float32(0)).astype(np.float64)
    H = num_hypotheses
    t = np.float64(distance_threshold)
    tt = t * t
    plane_id = np.full(n_points, -1, np.int32)
    free = cand0.copy()
    out = dict(coeff=[], count=[], hyp_index=[], hyp_count=[], centroid=[], rms=[], fits=[])
    rounds, n_invalid = 0, 0
    for r in range(max_planes):
        cand = np.flatnonzero(free)
        m = len(cand)
        if m < 3:
            break
        P = P64[cand]
        a, n, nn, thr, valid = hypotheses(P, sample_indices(seed, r, H, m), tt, axis, min_cos)
        sc = scores(P, a, n, thr, valid)
        rounds += 1
        n_invalid += int((~valid).sum())
        if not valid.any():
            break
        best = int(sc[valid].max())
        h = int(np.flatnonzero(valid & (sc == best))[0])
        if best < min_inliers:
            break
        ma, mn, mnn, mthr = a[h], n[h], nn[h], thr[h]
        inl, _ = inliers(P, ma, mn, mthr)
        assert int(inl.sum()) == best
        if refine:
            member = np.zeros(n_points, bool)
            member[cand[inl]] = True
            cnt = np.float64(best)
            g = np.array([tree(P64[:, k], member, n_points) / cnt for k in range(3)])
            d = P64 - g
            prods = (d[:, 0] * d[:, 0], d[:, 1] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 0], d[:, 2] * d[:, 1], d[:, 2] * d[:, 2])
            Q = [tree(p, member, n_points) for p in prods]
            u = smallest_eigenvector(Q)
            out["fits"].append((Q, max(float(np.abs(p[member]).sum()) for p in prods), list(u)))
            c4 = orient(u + [-((u[0] * g[0] + u[1] * g[1]) + u[2] * g[2])], axis)
            ma, mn = g, np.array(c4[:3])
            mnn = (mn[0] * mn[0] + mn[1] * mn[1]) + mn[2] * mn[2]
            mthr = tt * mnn
            inl, _ = inliers(P, ma, mn, mthr)
        else:
            ln = math.sqrt(mnn)
            u = [float(mn[0]) / ln, float(mn[1]) / ln, float(mn[2]) / ln]
            c4 = orient(u + [-((u[0] * float(ma[0]) + u[1] * float(ma[1])) + u[2] * float(ma[2]))], axis)
        member = np.zeros(n_points, bool)
        member[cand[inl]] = True
        count = int(inl.sum())
        cnt = np.float64(count)
        dd = P64 - ma
        e = (mn[0] * dd[:, 0] + mn[1] * dd[:, 1]) + mn[2] * dd[:, 2]
        with np.errstate(invalid="ignore", divide="ignore"):
            cen = [tree(P64[:, k], member, n_points) / cnt for k in range(3)]
            q = tree(e * e, member, n_points) / mnn
            rms = math.sqrt((q if q > 0.0 else 0.0) / cnt) if count else float("nan")
        out["coeff"].append(c4); out["count"].append(count); out["hyp_index"].append(h); out["hyp_count"].append(best)
        out["centroid"].append(cen); out["rms"].append(rms)
        plane_id[cand[inl]] = r
        free[cand[inl]] = False
    k = len(out["count"])
    return {
        "plane_id": plane_id,
        "coeff": np.array(out["coeff"], np.float64).reshape(k, 4),
        "count": np.array(out["count"], np.int32),
        "hyp_index": np.array(out["hyp_index"], np.int32),
        "hyp_count": np.array(out["hyp_count"], np.int32),
        "centroid": np.array(out["centroid"], np.float64).reshape(k, 3),
        "rms": np.array(out["rms"], np.float64),
        "n_points": n_points, "n_finite": int(finite.sum()), "n_candidates": int(cand0.sum()), "n_assigned": int((plane_id >= 0).sum()),
        "n_planes": k, "rounds": rounds, "n_invalid_hypotheses": n_invalid,
        "fits": out["fits"],
    }
