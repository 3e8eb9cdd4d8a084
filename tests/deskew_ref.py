"""sicp_deskew restated in numpy (include/sicp.h, "deskewing a scan").

deskew(): rules 3 and 4 -- the per-point arithmetic in float64, every operation a numpy operation of its own (numpy contracts
nothing), in the order the header fixes, on the knot table the library hands back: bit-exact.  compose_knots(): rule 2 composed
here, for a tolerance check of that table.  twist_knots(): rule 8 with Sophus' exp and log written out."""
from __future__ import annotations

import numpy as np

QNAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]
COUNTS = ("n_points", "n_finite", "n_moved", "n_bad_time", "n_clamped_lo", "n_clamped_hi")


# ---- SE(3), qt = [qx qy qz qw tx ty tz] ---------------------------------------------------------------------------------------
def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def normalised(qt):
    qt = np.asarray(qt, np.float64)
    return np.concatenate([qt[:4] / np.linalg.norm(qt[:4]), qt[4:]])


def mul(a, b):
    return np.concatenate([_qmul(a[:4], b[:4]), a[4:] + _rot(a[:4]) @ b[4:]])


def inverse(a):
    q = np.array([-a[0], -a[1], -a[2], a[3]])
    return np.concatenate([q, -(_rot(q) @ a[4:])])


def compose_knots(knot_qt, ref_qt=None):
    """rule 2: K_k = ref^-1 T_k, consecutive quaternions in one hemisphere"""
    knot_qt = np.asarray(knot_qt, np.float64).reshape(-1, 7)
    inv = inverse(normalised(knot_qt[-1] if ref_qt is None else ref_qt))
    K = np.stack([mul(inv, normalised(T)) for T in knot_qt])
    for k in range(1, len(K)):
        if K[k, :4] @ K[k - 1, :4] < 0:
            K[k, :4] = -K[k, :4]
    return K


def _hat(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])


def se3_exp(a):
    a = np.asarray(a, np.float64)
    u, w = a[:3], a[3:]
    th = np.linalg.norm(w)
    if th < 1e-10:
        return np.concatenate([0.5 * w, [1.0], u])
    W = _hat(w)
    V = np.eye(3) + (1 - np.cos(th)) / th**2 * W + (th - np.sin(th)) / th**3 * (W @ W)
    return np.concatenate([np.sin(0.5 * th) / th * w, [np.cos(0.5 * th)], V @ u])


def se3_log(qt):
    qt = np.asarray(qt, np.float64)
    n = np.linalg.norm(qt[:3])
    if n < 1e-10:
        w = 2.0 / qt[3] * qt[:3]
    else:
        w = 2.0 * np.arctan(n / qt[3]) / n * qt[:3]
    th = np.linalg.norm(w)
    W = _hat(w)
    c = 1.0 / 12.0 if th < 1e-10 else (1.0 - th * np.cos(0.5 * th) / (2.0 * np.sin(0.5 * th))) / th**2
    Vi = np.eye(3) - 0.5 * W + c * (W @ W)
    return np.concatenate([Vi @ qt[4:], w])


def twist_knots(delta_qt, t0, t1, n_knots):
    """rule 8: knot k = exp(s_k log(delta)) at t0 + s_k (t1 - t0), s_k = k / (n_knots - 1)"""
    xi = se3_log(normalised(delta_qt))
    s = np.arange(n_knots, dtype=np.float64) / np.float64(n_knots - 1)
    return t0 + s * (t1 - t0), np.stack([se3_exp(sk * xi) for sk in s])


# ---- rules 3 and 4 ------------------------------------------------------------------------------------------------------------
def deskew(xyz, times, knot_time, K):
    """xyz [n, 3] float32, times [n] float64, knot_time [m] float64 ascending, K [m, 7] float64: the table of rule 2.
    Returns {"points": [n, 3] float32, the six counts}"""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(times, np.float64)
    kt = np.ascontiguousarray(knot_time, np.float64)
    K = np.ascontiguousarray(K, np.float64).reshape(-1, 7)
    m = len(kt)
    out = xyz.copy()
    finite = np.isfinite(xyz).all(axis=1)
    good = np.isfinite(t)
    bad = finite & ~good
    mv = finite & good
    out[bad] = QNAN
    res = dict(n_points=len(xyz), n_finite=int(finite.sum()), n_moved=int(mv.sum()), n_bad_time=int(bad.sum()), n_clamped_lo=0, n_clamped_hi=0)
    if mv.any():
        with np.errstate(all="ignore"):
            tm = t[mv]
            p = xyz[mv].astype(np.float64)
            a = np.clip(np.searchsorted(kt, tm, side="right") - 1, 0, m - 2)  # the largest index with kt[a] <= t, limited
            lo, hi = tm < kt[0], tm > kt[m - 1]
            u = (tm - kt[a]) / (kt[a + 1] - kt[a])
            u = np.where(lo, 0.0, np.where(hi, 1.0, u))
            w = 1.0 - u
            c = (w[:, None] * K[a]) + (u[:, None] * K[a + 1])
            qx, qy, qz, qw = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
            xx, yy, zz, ww = qx * qx, qy * qy, qz * qz, qw * qw
            s = ((xx + yy) + zz) + ww
            k = 2.0 / s
            xy, xz, yz = qx * qy, qx * qz, qy * qz
            wx, wy, wz = qw * qx, qw * qy, qw * qz
            rows = (
                (1.0 - k * (yy + zz), k * (xy - wz), k * (xz + wy), c[:, 4]),
                (k * (xy + wz), 1.0 - k * (xx + zz), k * (yz - wx), c[:, 5]),
                (k * (xz - wy), k * (yz + wx), 1.0 - k * (xx + yy), c[:, 6]),
            )
            moved = np.empty((len(tm), 3), np.float32)
            for r, (m0, m1, m2, m3) in enumerate(rows):
                moved[:, r] = ((((m0 * p[:, 0]) + (m1 * p[:, 1])) + (m2 * p[:, 2])) + m3).astype(np.float32)
        out[mv] = moved
        res["n_clamped_lo"], res["n_clamped_hi"] = int(lo.sum()), int(hi.sum())
    res["points"] = out
    return res
