"""The numpy restatement of sicp_camera_image / sicp_camera_labels / sicp_camera_unproject (include/sicp.h, "camera: depth frames
and image labels", rules 1-14): the same doubles, one numpy operation per rounded operation (numpy contracts nothing), the
64-bit winner key, the truncated window and the fixed-count undistortion.  `mat` is {"cam_to_cloud", "cloud_to_cam"}, each
[3, 4] float64 -- what sicp_camera_matrices handed back when a result is compared to the bit, or matrices() below, the same
formulas in numpy, when only the restatement itself is under test.  `p` is anything with the fields of sicp_camera_params."""
import types

import numpy as np

F = np.float32
COUNTS = ("n_points", "n_finite", "n_kept", "n_outside", "n_pixels_hit")
LABEL_COUNTS = ("n_labelled", "n_occluded", "n_unclassed")
IMAGES = ("index", "depth", "x", "y", "z", "label", "count")
PER_POINT = ("pixel", "u", "v", "visible")
GROUP = 256        # points one workgroup of a per-point launch takes per pass (the shapes the GPU tests straddle; no rule depends on it)
MAX_GROUPS = 1024  # workgroups a per-point launch has at most: more finite points than GROUP MAX_GROUPS and some take a second pass (likewise)


def params(**kw):
    """the defaults of sicp_default_camera_params with any field overridden"""
    d = dict(width=640, height=480, fx=525.0, fy=525.0, cx=319.5, cy=239.5, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, min_depth=0.3,
             max_depth=100.0, max_tan_sq=4.0, depth_scale=0.001, undistort_iterations=20, window=5, occlusion_abs=0.3,
             occlusion_rel=0.02)
    d.update(kw)
    return types.SimpleNamespace(**d)


def matrices(qt=None):
    """camera -> cloud as the engine forms a pose matrix (Eigen's toRotationMatrix, no normalisation) and (R^T | -R^T t)"""
    q = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float64) if qt is None else np.asarray(qt, dtype=np.float64)
    x, y, z, w = q[:4]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    t = q[4:]
    back = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)])
    return {"cam_to_cloud": np.concatenate([R, t[:, None]], axis=1), "cloud_to_cam": np.concatenate([R.T, back[:, None]], axis=1)}


def _rows(m, x, y, z):
    """rule 1 / rule 13: ((m0 x + m1 y) + m2 z) + m3 per row"""
    return [((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)]


def _distortion(p, x, y):
    """rule 4: rad, tx, ty from the pair x, y"""
    k1, k2, p1, p2, k3 = float(p.k1), float(p.k2), float(p.p1), float(p.p2), float(p.k3)
    a, b, c = x * x, y * y, x * y
    r2 = a + b
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    tx = (2.0 * p1) * c + p2 * (r2 + 2.0 * a)
    ty = p1 * (r2 + 2.0 * b) + (2.0 * p2) * c
    return r2, rad, tx, ty


def project(xyz, p, mat):
    """rules 1-5: per point Zc, the finite / kept / inview / inimage flags, u, v (float64), zf and the pixel (-1: none)"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    W, H = int(p.width), int(p.height)
    m = np.asarray(mat["cloud_to_cam"], dtype=np.float64)
    with np.errstate(all="ignore"):
        finite = np.isfinite(xyz).all(axis=1)
        q = xyz.astype(np.float64)
        Xc, Yc, Zc = _rows(m, q[:, 0], q[:, 1], q[:, 2])
        kept = finite & (Zc >= float(p.min_depth)) & (Zc < float(p.max_depth))
        xn, yn = Xc / Zc, Yc / Zc
        r2, rad, tx, ty = _distortion(p, xn, yn)
        inview = kept & (r2 <= float(p.max_tan_sq))
        xd, yd = xn * rad + tx, yn * rad + ty
        u, v = float(p.fx) * xd + float(p.cx), float(p.fy) * yd + float(p.cy)
        cf, rf = np.floor(u + 0.5), np.floor(v + 0.5)
        inimage = inview & (cf >= 0) & (cf <= W - 1) & (rf >= 0) & (rf <= H - 1)
        pixel = np.where(inimage, np.where(inimage, rf, 0) * W + np.where(inimage, cf, 0), -1).astype(np.int32)
        zf = np.where(inimage, Zc, 0.0).astype(F)
    return dict(Zc=Zc, finite=finite, kept=kept, inview=inview, inimage=inimage, u=u, v=v, zf=zf, pixel=pixel)


def image(xyz, labels, p, mat):
    """rule 6 and the outputs of sicp_camera_image: the dense images [H, W], the per-point arrays and the counts"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    W, H = int(p.width), int(p.height)
    pr = project(xyz, p, mat)
    idx = np.flatnonzero(pr["inimage"])
    pix = pr["pixel"][idx].astype(np.int64)
    key = (pr["zf"][idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)
    order = np.lexsort((key, pix))
    first = np.ones(len(order), dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    win_pix, win_pt = pix[order][first], idx[order][first]
    out = {"index": np.full(H * W, -1, dtype=np.int32), "depth": np.zeros(H * W, dtype=F)}
    out["index"][win_pix] = win_pt
    out["depth"][win_pix] = pr["zf"][win_pt]
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
    with np.errstate(all="ignore"):
        out["u"] = np.where(pr["inview"], pr["u"], np.nan).astype(F)
        out["v"] = np.where(pr["inview"], pr["v"], np.nan).astype(F)
    out["visible"] = np.zeros(n, dtype=np.uint8)
    out["visible"][win_pt] = 1
    out["zf"] = pr["zf"]
    out.update(n_points=n, n_finite=int(pr["finite"].sum()), n_kept=int(pr["kept"].sum()),
               n_outside=int((pr["kept"] & ~pr["inimage"]).sum()), n_pixels_hit=len(win_pix))
    return out


def labels(xyz, own, pixel_label, p, mat):
    """rules 7-9: {"labels": uint32 [n], "state": uint8 [n], the counts, "image": image()}"""
    xyz = np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3)
    n = len(xyz)
    W, H, half = int(p.width), int(p.height), int(p.window) // 2
    im = image(xyz, own, p, mat)
    pl = np.ascontiguousarray(pixel_label, dtype=np.uint32).reshape(H * W)
    out_l = np.zeros(n, dtype=np.uint32) if own is None else np.asarray(own, dtype=np.uint32).copy()
    out_l[~np.isfinite(xyz).all(axis=1)] = 0  # (set_cloud dropped the point with its label)
    state = np.zeros(n, dtype=np.uint8)
    idx = np.flatnonzero(im["pixel"] >= 0)
    if len(idx):
        r, c = im["pixel"][idx] // W, im["pixel"][idx] % W
        front = np.full((H + 2 * half, W + 2 * half), np.inf, dtype=F)  # beyond the border and in an empty pixel: no winner
        front[half:half + H, half:half + W] = np.where(im["index"] >= 0, im["depth"], F(np.inf))
        zmin = np.full(len(idx), np.inf, dtype=F)
        for wr in range(2 * half + 1):
            for wc in range(2 * half + 1):
                zmin = np.minimum(zmin, front[r + wr, c + wc])
        with np.errstate(all="ignore"):
            zd, zm = im["zf"][idx].astype(np.float64), zmin.astype(np.float64)
            occluded = (zd - zm) > (float(p.occlusion_abs) + float(p.occlusion_rel) * zm)
        cls = pl[im["pixel"][idx]]
        st = np.where(occluded, 2, np.where(cls != 0, 1, 3)).astype(np.uint8)
        state[idx] = st
        seen = st == 1
        out_l[idx[seen]] = cls[seen]
    return {"labels": out_l, "state": state, "n_labelled": int((state == 1).sum()), "n_occluded": int((state == 2).sum()),
            "n_unclassed": int((state == 3).sum()), "image": im}


def unproject(depth, p, mat):
    """rules 11-13: {"xyz": float32 [H W, 3] (NaN: invalid), "valid": uint8 [H, W], "n_valid"}; depth uint16 or float32 [H, W]"""
    W, H = int(p.width), int(p.height)
    d = np.ascontiguousarray(depth).reshape(H, W)
    assert d.dtype in (np.uint16, np.float32)
    m = np.asarray(mat["cam_to_cloud"], dtype=np.float64)
    with np.errstate(all="ignore"):
        Z = d.astype(np.float64) * float(p.depth_scale) if d.dtype == np.uint16 else d.astype(np.float64)
        valid = np.isfinite(Z) & (Z >= float(p.min_depth)) & (Z < float(p.max_depth))
        c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
        xd, yd = (c - float(p.cx)) / float(p.fx), (r - float(p.cy)) / float(p.fy)
        x, y = xd, yd
        for _ in range(int(p.undistort_iterations)):
            _, rad, tx, ty = _distortion(p, x, y)
            x, y = (xd - tx) / rad, (yd - ty) / rad
        rows = _rows(m, x * Z, y * Z, Z)
        xyz = np.stack([np.where(valid, v, np.nan).astype(F).reshape(-1) for v in rows], axis=1)
    return {"xyz": xyz, "valid": valid.astype(np.uint8), "n_valid": int(valid.sum())}
