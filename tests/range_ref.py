"""The numpy restatement of sicp_range_image / sicp_range_labels (include/sicp.h, "range image and labels from it", rules 1-13):
the same float32 operations with np.float32 operands, the same doubles, the same two fixed bisections (vectorised: every point
walks its own lo / hi), the 64-bit winner key, the window's visiting order, the k smallest (bits(d2), order) and the vote.
`tab` is {"cos_half", "sin_half", "row_edge"} -- what sicp_range_tables handed back when a result is compared to the bit, or
tables() below, the same formulas in numpy, when only the restatement itself is under test.  `p` is anything with the fields of
sicp_range_params."""
import types

import numpy as np

F = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
COUNTS = ("n_points", "n_finite", "n_kept", "n_out_of_range", "n_outside_fov", "n_pixels_hit")
IMAGES = ("index", "range_sq", "x", "y", "z", "label", "count")
GROUP = 256        # points one workgroup of a per-point launch takes per pass (the shapes the GPU tests straddle; no rule depends on it)
MAX_GROUPS = 1024  # workgroups a per-point launch has at most: more finite points than GROUP MAX_GROUPS and some take a second pass (likewise)


def params(**kw):
    """the defaults of sicp_default_range_params with any field overridden; a width without col_shift moves the shift to W / 2"""
    d = dict(width=2048, height=64, fov_up=3.0 * np.pi / 180.0, fov_down=-25.0 * np.pi / 180.0, min_range=0.5, max_range=120.0,
             clockwise=1, col_shift=1024, window=5, k=5, max_dist_sq=1.0)
    d.update(kw)
    if "width" in kw and "col_shift" not in kw:
        d["col_shift"] = d["width"] // 2
    return types.SimpleNamespace(**d)


def edge_angles(p, beam=None):
    """the elevations a_0 .. a_H of the row edges"""
    H = int(p.height)
    if beam is not None and H > 1:
        b = np.asarray(beam, dtype=np.float64)
        a = np.empty(H + 1)
        a[0] = b[0] + (b[0] - b[1]) / 2.0
        a[1:H] = (b[:-1] + b[1:]) / 2.0
        a[H] = b[H - 1] - (b[H - 2] - b[H - 1]) / 2.0
        return a
    a = float(p.fov_up) + (float(p.fov_down) - float(p.fov_up)) * (np.arange(H + 1, dtype=np.float64) / float(H))
    a[H] = float(p.fov_down)
    return a


def tables(p, beam=None):
    W = int(p.width)
    t = np.tan(edge_angles(p, beam))
    ang = 2.0 * np.pi * np.arange(W // 2, dtype=np.float64) / float(W)
    return {"cos_half": np.cos(ang), "sin_half": np.sin(ang), "row_edge": t * np.abs(t)}


def _bisect(n, top, pred):
    """lo = 0, hi = top; while (hi - lo > 1) { mid = (lo + hi) >> 1; if (pred(mid)) lo = mid; else hi = mid; } for n walkers"""
    lo = np.zeros(n, dtype=np.int64)
    hi = np.full(n, top, dtype=np.int64)
    while True:
        act = hi - lo > 1
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        t = pred(mid)
        lo = np.where(act & t, mid, lo)
        hi = np.where(act & ~t, mid, hi)


def project(xyz, p, tab, origin=None):
    """rules 1-5: per point r2, finite / kept / outside flags, row, col and pixel (-1: none)"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    W, H = int(p.width), int(p.height)
    o = np.zeros(3, dtype=F) if origin is None else np.asarray(origin, dtype=F)
    e, ch, sh = tab["row_edge"], tab["cos_half"], tab["sin_half"]
    min_sq, max_sq = float(p.min_range) * float(p.min_range), float(p.max_range) * float(p.max_range)
    with np.errstate(all="ignore"):
        finite = np.isfinite(xyz).all(axis=1)
        dx, dy, dz = xyz[:, 0] - o[0], xyz[:, 1] - o[1], xyz[:, 2] - o[2]
        r2 = (dx * dx + dy * dy) + dz * dz
        assert r2.dtype == F
        R = r2.astype(np.float64)
        kept = finite & (R >= min_sq) & (R < max_sq)
        X, Y, Z = dx.astype(np.float64), dy.astype(np.float64), dz.astype(np.float64)
        D = X * X + Y * Y
        Zs = Z * np.abs(Z)
        outside = kept & ((Zs > e[0] * D) | ~(Zs >= e[H] * D))
        row = _bisect(n, H, lambda mid: Zs < e[mid] * D)
        lower = ~((dy > 0) | ((dy == 0) & (dx > 0)))
        xp, yp = np.where(lower, -X, X), np.where(lower, -Y, Y)
        sec = _bisect(n, W // 2, lambda mid: (ch[mid] * yp - sh[mid] * xp) >= 0.0) + np.where(lower, W // 2, 0)
    c = W - 1 - sec if int(p.clockwise) else sec
    col = (c + int(p.col_shift)) % W
    inview = kept & ~outside
    pixel = np.where(inview, row * W + col, -1).astype(np.int32)
    return dict(r2=r2, finite=finite, kept=kept, outside=outside, inview=inview, row=row, col=col, sector=sec, pixel=pixel)


def image(xyz, labels, p, tab, origin=None):
    """rules 6-7: the dense images [H, W], pixel / visible per point and the counts"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    W, H = int(p.width), int(p.height)
    pr = project(xyz, p, tab, origin)
    idx = np.flatnonzero(pr["inview"])
    pix = pr["pixel"][idx].astype(np.int64)
    key = (pr["r2"][idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    order = np.lexsort((key, pix))
    first = np.ones(len(order), dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win_pix, win_pt = pix[order][first], idx[order][first]
    index = np.full(H * W, -1, dtype=np.int32)
    index[win_pix] = win_pt
    out = {"index": index}
    out["range_sq"] = np.zeros(H * W, dtype=F)
    out["range_sq"][win_pix] = pr["r2"][win_pt]
    for d, name in enumerate("xyz"):
        out[name] = np.zeros(H * W, dtype=F)
        out[name][win_pix] = xyz[win_pt, d]
    out["label"] = np.zeros(H * W, dtype=np.uint32)
    if labels is not None:
        out["label"][win_pix] = np.asarray(labels, dtype=np.uint32)[win_pt]
    out["count"] = np.bincount(pix, minlength=H * W).astype(np.uint32)
    for k in IMAGES:
        out[k] = out[k].reshape(H, W)
    out["pixel"] = pr["pixel"]
    out["visible"] = np.zeros(n, dtype=np.uint8)
    out["visible"][win_pt] = 1
    out.update(n_points=n, n_finite=int(pr["finite"].sum()), n_kept=int(pr["kept"].sum()),
               n_out_of_range=int(pr["finite"].sum() - pr["kept"].sum()), n_outside_fov=int(pr["outside"].sum()),
               n_pixels_hit=len(win_pix))
    return out


def vote(xyz, labels, pixel_label, p, tab, origin=None):
    """rules 8-12: {"labels": uint32 [n], "votes": uint8 [n], "n_voted", "n_unvoted"} and, for the tests, "neighbours": the
    number of neighbours (<= k) every point voted with"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    W, H, S, K = int(p.width), int(p.height), int(p.window), int(p.k)
    im = image(xyz, labels, p, tab, origin)
    pl = np.ascontiguousarray(pixel_label, dtype=np.uint32).reshape(H * W)
    own = np.zeros(n, dtype=np.uint32) if labels is None else np.asarray(labels, dtype=np.uint32).copy()
    own[~np.isfinite(xyz).all(axis=1)] = 0  # (set_cloud dropped the point with its label)
    out_l, out_v, out_nb = own.copy(), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int32)
    idx = np.flatnonzero(im["pixel"] >= 0)
    m = len(idx)
    if m:
        r, c = im["pixel"][idx] // W, im["pixel"][idx] % W
        win = im["index"].reshape(-1)
        half = S // 2
        keys = np.full((m, S * S), EMPTY, dtype=np.uint64)
        labs = np.zeros((m, S * S), dtype=np.uint32)
        order = 0
        with np.errstate(all="ignore"):
            for wr in range(-half, half + 1):
                for wc in range(-half, half + 1):
                    rr, cc = r + wr, (c + wc) % W
                    ok = (rr >= 0) & (rr < H)
                    q = np.where(ok, rr, 0) * W + cc
                    w = win[q]
                    ok &= w >= 0
                    wp = xyz[np.where(ok, w, 0)]
                    ex, ey, ez = xyz[idx, 0] - wp[:, 0], xyz[idx, 1] - wp[:, 1], xyz[idx, 2] - wp[:, 2]
                    d2 = (ex * ex + ey * ey) + ez * ez
                    assert d2.dtype == F
                    ok &= d2.astype(np.float64) < float(p.max_dist_sq)
                    key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(order)
                    keys[:, order] = np.where(ok, key, EMPTY)
                    labs[:, order] = pl[q]
                    order += 1
        pos = np.argsort(keys, axis=1, kind="stable")[:, :K]
        kk = np.take_along_axis(keys, pos, axis=1)
        ll = np.take_along_axis(labs, pos, axis=1)
        nb = kk != EMPTY
        valid = nb & (ll != 0)
        cnt = ((ll[:, :, None] == ll[:, None, :]) & valid[:, None, :]).sum(axis=2)
        score = np.where(valid, (cnt.astype(np.int64) << 32) + (0xFFFFFFFF - ll.astype(np.int64)), -1)
        best = np.argmax(score, axis=1)
        rows = np.arange(m)
        has = valid.any(axis=1)
        out_l[idx[has]] = ll[rows, best][has]
        out_v[idx[has]] = cnt[rows, best][has].astype(np.uint8)
        out_nb[idx] = nb.sum(axis=1)
    nv = int((out_v > 0).sum())
    return {"labels": out_l, "votes": out_v, "neighbours": out_nb, "n_voted": nv, "n_unvoted": n - nv, "image": im}
