"""numpy restatement of the initial alignment without a pose prior (exec/bootstrap.h; INTEGRATION.md "Bootstrap"):
box filter, voxel grid, radius neighbourhoods, normals, FPFH and SAC-IA with its splitmix64 sampling.  Test-only."""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

DEFAULTS = dict(box_max=35.0, leaf_size=0.4, normal_radius=3.0, feature_radius=3.0, min_sample_distance=0.4,
                max_corr_distance=0.8, max_iterations=500, nr_samples=3, k_correspondences=10, seed=1)
M64 = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed: int):
        self.state = seed & M64

    def next(self) -> int:
        self.state = (self.state + 0x9E3779B97F4A7C15) & M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    def index(self, n: int) -> int:
        u = float(self.next() >> 11) * 2.0 ** -53
        return int(np.floor(float(n) * u))


def voxel_keypoints(xyz, box_max=35.0, leaf=0.4):
    """centroids (f64 sums in ascending index, divided, rounded once to f32) of the occupied voxels, ascending voxel index"""
    p = np.asarray(xyz, dtype=np.float32)
    p = p[np.isfinite(p).all(axis=1)]
    keep = (p[:, 0].astype(np.float64) < box_max) & (p[:, 1].astype(np.float64) < box_max) & (p[:, 2].astype(np.float64) < box_max)
    p = p[keep]
    if len(p) == 0:
        return np.zeros((0, 3), np.float32)
    inv = np.float32(1.0) / np.float32(leaf)
    ijk = np.floor(p * inv).astype(np.int64)
    mn = np.floor(p.min(axis=0) * inv).astype(np.int64)
    mx = np.floor(p.max(axis=0) * inv).astype(np.int64)
    div = mx - mn + 1
    if div[0] * div[1] * div[2] > 2**31 - 1:
        raise OverflowError("voxel grid overflows int32")
    rel = ijk - mn
    vid = rel[:, 0] + rel[:, 1] * div[0] + rel[:, 2] * div[0] * div[1]
    order = np.lexsort((np.arange(len(p)), vid))
    vs, ps = vid[order], p[order].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, vs[1:] != vs[:-1]])
    counts = np.diff(np.r_[starts, len(vs)])
    acc = np.zeros((len(starts), 3))
    for j in range(int(counts.max())):  # sequential per voxel
        live = counts > j
        acc[live] += ps[starts[live] + j]
    return (acc / counts[:, None]).astype(np.float32)


def d2_f32(a, b):
    d = (a - b).astype(np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def radius_lists(kp, r):
    """CSR neighbour lists (the point itself included), d^2 < f32(r^2) in f32, sorted by (d^2, index)"""
    kp = np.asarray(kp, dtype=np.float32)
    r2 = np.float32(r * r)
    cand = cKDTree(kp.astype(np.float64)).query_ball_point(kp.astype(np.float64), r * 1.001 + 1e-6)
    off, idx, dd = [0], [], []
    for i, c in enumerate(cand):
        c = np.asarray(c, dtype=np.int64)
        d = d2_f32(kp[c], kp[i])
        sel = d < r2
        c, d = c[sel], d[sel]
        o = np.lexsort((c, d))
        idx.append(c[o]); dd.append(d[o])
        off.append(off[-1] + len(c))
    return np.array(off, np.int64), np.concatenate(idx).astype(np.int32), np.concatenate(dd).astype(np.float32)


def normals(kp, off, idx):
    m = len(kp)
    out = np.full((m, 3), np.nan)
    P = kp.astype(np.float64)
    cnt = np.diff(off)
    ok = cnt >= 3
    seg = np.repeat(np.arange(m), cnt)
    mean = np.zeros((m, 3))
    np.add.at(mean, seg, P[idx])
    mean /= np.maximum(cnt, 1)[:, None]
    D = P[idx] - mean[seg]
    cov = np.zeros((m, 3, 3))
    np.add.at(cov, seg, D[:, :, None] * D[:, None, :])
    cov /= np.maximum(cnt, 1)[:, None, None]
    w, v = np.linalg.eigh(cov[ok])
    n = v[:, :, 0]
    flip = np.einsum("ij,ij->i", -P[ok], n) < 0
    n[flip] *= -1
    out[ok] = n
    gap = np.full(m, np.nan)
    gap[ok] = w[:, 1] - w[:, 0]
    return out, gap


def pair_features(p1, n1, p2, n2):
    """pcl::computePairFeatures in f64 (vectorised): f1, f2, f3 and the validity mask"""
    dp = p2 - p1
    f4 = np.sqrt((dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2])
    valid = f4 != 0
    f4s = np.where(valid, f4, 1.0)
    a1 = ((n1[:, 0] * dp[:, 0] + n1[:, 1] * dp[:, 1]) + n1[:, 2] * dp[:, 2]) / f4s
    a2 = ((n2[:, 0] * dp[:, 0] + n2[:, 1] * dp[:, 1]) + n2[:, 2] * dp[:, 2]) / f4s
    sw = np.abs(a1) < np.abs(a2)  # acos(|a1|) > acos(|a2|)
    u = np.where(sw[:, None], n2, n1)
    m = np.where(sw[:, None], n1, n2)
    dp = np.where(sw[:, None], -dp, dp)
    f3 = np.where(sw, -a2, a1)
    v = np.stack([dp[:, 1] * u[:, 2] - dp[:, 2] * u[:, 1], dp[:, 2] * u[:, 0] - dp[:, 0] * u[:, 2], dp[:, 0] * u[:, 1] - dp[:, 1] * u[:, 0]], 1)
    vn = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    valid &= vn != 0
    v = v / np.where(vn != 0, vn, 1.0)[:, None]
    w = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    f2 = (v[:, 0] * m[:, 0] + v[:, 1] * m[:, 1]) + v[:, 2] * m[:, 2]
    f1 = np.arctan2((w[:, 0] * m[:, 0] + w[:, 1] * m[:, 1]) + w[:, 2] * m[:, 2], (u[:, 0] * m[:, 0] + u[:, 1] * m[:, 1]) + u[:, 2] * m[:, 2])
    return f1, f2, f3, valid


def bins(f1, f2, f3):
    b1 = np.clip(np.floor(11.0 * (f1 + np.pi) / (2.0 * np.pi)), 0, 10).astype(np.int64)
    b2 = np.clip(np.floor(11.0 * (f2 + 1.0) / 2.0), 0, 10).astype(np.int64)
    b3 = np.clip(np.floor(11.0 * (f3 + 1.0) / 2.0), 0, 10).astype(np.int64)
    return b1, b2, b3


def fpfh(kp, nrm, off, idx, d2):
    m = len(kp)
    P = kp.astype(np.float64)
    cnt = np.diff(off)
    seg = np.repeat(np.arange(m), cnt)
    okn = ~np.isnan(nrm[:, 0])
    sel = (idx != seg) & okn[seg] & okn[idx]
    p, q = seg[sel], idx[sel].astype(np.int64)
    f1, f2, f3, valid = pair_features(P[p], nrm[p], P[q], nrm[q])
    p = p[valid]
    b1, b2, b3 = bins(f1[valid], f2[valid], f3[valid])
    counts = np.zeros((m, 33))
    for off_b, b in ((0, b1), (11, b2), (22, b3)):
        np.add.at(counts, (p, off_b + b), 1.0)
    spfh = counts * (100.0 / np.maximum(cnt - 1, 1))[:, None]
    spfh[~okn] = np.nan
    out = np.full((m, 33), np.nan, np.float32)
    use = (d2 > 0) & okn[idx] & okn[seg]
    acc = np.zeros((m, 33))
    np.add.at(acc, seg[use], spfh[idx[use]] / d2[use].astype(np.float64)[:, None])
    for t in range(3):
        s = acc[:, 11 * t:11 * t + 11].sum(axis=1)
        acc[:, 11 * t:11 * t + 11] *= np.where(s != 0, 100.0 / np.where(s != 0, s, 1.0), 1.0)[:, None]
    out[okn] = acc[okn].astype(np.float32)
    return out


def features(kp, normal_radius=3.0, feature_radius=3.0):
    """lists of the feature radius, normals from the normal radius' lists (their own when the radii differ), FPFH"""
    if len(kp) == 0:
        z = np.zeros(0)
        return dict(off=np.zeros(1, np.int64), idx=z.astype(np.int32), d2=z.astype(np.float32), normals=np.zeros((0, 3)),
                    gap=z, fpfh=np.zeros((0, 33), np.float32))
    off, idx, d2 = radius_lists(kp, feature_radius)
    if normal_radius == feature_radius:
        n, gap = normals(kp, off, idx)
    else:
        n, gap = normals(kp, *radius_lists(kp, normal_radius)[:2])
    return dict(off=off, idx=idx, d2=d2, normals=n, gap=gap, fpfh=fpfh(kp, n, off, idx, d2))


def feature_knn(sf, tf, k):
    """k nearest target features (f32 L2, bins summed in order; ties to the lower index); -1 beyond / without a feature"""
    ok_t = ~np.isnan(tf[:, 0])
    tv = np.flatnonzero(ok_t)
    out = np.full((len(sf), k), -1, np.int32)
    for a in range(0, len(sf), 128):
        q = sf[a:a + 128]
        d = np.zeros((len(q), len(tv)), np.float32)
        for b in range(33):
            df = q[:, b:b + 1] - tf[tv, b][None, :]
            d = d + df * df
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        res = tv[o].astype(np.int32)
        if res.shape[1] < k:
            res = np.concatenate([res, np.full((len(q), k - res.shape[1]), -1, np.int32)], 1)
        res[np.isnan(q[:, 0])] = -1
        out[a:a + 128] = res
    return out


def umeyama(src, tgt):
    """rigid transform (no scale, reflection fixed) taking src onto tgt, f64: rows 0..2 of the 4x4 matrix"""
    s, t = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    cs, ct = s.mean(axis=0), t.mean(axis=0)
    H = (s - cs).T @ (t - ct)
    U, _, Vt = np.linalg.svd(H)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return np.hstack([R, (ct - R @ cs)[:, None]])


def fit_rank_ratio(src, tgt):
    """second over first singular value of the pairs' cross-covariance.  The rotation of the rigid fit is unique only when
    this matrix has rank 2 or more: at 0 (either side collinear -- one target keypoint drawn for two of three samples is
    enough) every rotation about the common line is an optimum, and the result belongs to the solver."""
    s, t = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    sv = np.linalg.svd((s - s.mean(axis=0)).T @ (t - t.mean(axis=0)), compute_uv=False)
    return float(sv[1] / sv[0]) if sv[0] > 0 else 0.0


def transform_f32(M, p):
    """f64 products and sums ((m0 x + m1 y) + m2 z) + m3, rounded to f32"""
    P = p.astype(np.float64)
    cols = [((M[r, 0] * P[:, 0] + M[r, 1] * P[:, 1]) + M[r, 2] * P[:, 2]) + M[r, 3] for r in range(3)]
    return np.stack(cols, 1).astype(np.float32)


def truncated_error(M, src_kp, tgt_tree, tgt_kp, t):
    q = transform_f32(M, src_kp)
    _, j = tgt_tree.query(q.astype(np.float64))
    e = d2_f32(q, tgt_kp[j]).astype(np.float64)
    t = float(np.float32(t))
    return float(np.sum(np.where(e <= t, e / t, 1.0)))


def sac_ia(src_kp, src_f, tgt_kp, tgt_f, knn=None, stats=None, **kw):
    """SampleConsensusInitialAlignment: (best iteration, its error, all errors, all matrices).  `stats` (a dict) receives
    what the run went through: "halvings" (times min_sample_distance was halved), "k_eff", "draws" (sample draws),
    "samples" ([(source indices, target indices)] per iteration) and "ambiguous": the iterations whose pairs do not fix a
    rotation (fit_rank_ratio below 1e-6), where any two solvers may return different optima."""
    P = dict(DEFAULTS, **kw)
    halvings = draws = 0
    samples, ambiguous = [], []
    k, nr = P["k_correspondences"], P["nr_samples"]
    if knn is None:
        knn = feature_knn(src_f, tgt_f, k)
    valid = np.flatnonzero(~np.isnan(src_f[:, 0]))
    k_eff = min(k, int((~np.isnan(tgt_f[:, 0])).sum()))
    rng = SplitMix64(P["seed"])
    tree = cKDTree(tgt_kp.astype(np.float64))
    errs, Ms = [], []
    nv = len(valid)
    for _ in range(P["max_iterations"]):
        smp, fails, min_d = [], 0, np.float32(P["min_sample_distance"])
        while len(smp) < nr:
            si = int(valid[rng.index(nv)])
            draws += 1
            ok = True
            for sj in smp:
                d = src_kp[si] - src_kp[sj]
                dist = np.sqrt(np.float32((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                if si == sj or dist < min_d:
                    ok = False
                    break
            if ok:
                smp.append(si)
                fails = 0
            else:
                fails += 1
            if fails >= 3 * nv:
                min_d = np.float32(min_d * np.float32(0.5))
                fails = 0
                halvings += 1
        tj = [int(knn[s, rng.index(k_eff)]) for s in smp]
        M = umeyama(src_kp[smp], tgt_kp[tj])
        samples.append((list(smp), tj))
        if fit_rank_ratio(src_kp[smp], tgt_kp[tj]) < 1e-6:
            ambiguous.append(len(Ms))
        Ms.append(M)
        errs.append(truncated_error(M, src_kp, tree, tgt_kp, P["max_corr_distance"]))
    if stats is not None:
        stats.update(halvings=halvings, k_eff=k_eff, draws=draws, samples=samples, ambiguous=ambiguous)
    errs = np.array(errs)
    best = int(np.argmin(errs))
    return best, float(errs[best]), errs, np.array(Ms)
