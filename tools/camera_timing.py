#!/usr/bin/env python3
"""Times of sicp_camera_image / sicp_camera_labels / sicp_camera_unproject on the GPU -> profiles/camera/timing.json.

Two workloads.  The 100 K-point source scan of synth.lidar_pair(seed=2) through a KITTI-like camera (1242 x 375, fx = fy = 721.5,
mounted on the scanner and looking along its +x): the image with every output read back, the labels (window 5) read back, into
another handle's slot, and in place.  And a 640 x 480 uint16 depth frame with a label image into a slot.  Each whole C call
through the Python binding is timed beside the host route it replaces, in the same process on the same host: a plain vectorised
float64 numpy projection / windowed front-depth test / back-projection (the rays of the back-projection cached per camera, as a
careful caller would) and the sicp_set_cloud the result needs.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape.  A run is the median of `--reps` calls; `--runs` runs (default 5) give each figure's spread, and
"beats_numpy" says whether the call's slowest run is below the host route's fastest.  --trace runs every call a few times for a run
under `rocprofv3 --kernel-trace --stats` (tools/README.md); --kernel-stats folds that run's kernel rows into the JSON."""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import camera_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
KITTI = dict(width=1242, height=375, fx=721.5377, fy=721.5377, cx=609.5593, cy=172.854, max_depth=80.0)
ON_THE_SCANNER = np.array([-0.5, 0.5, -0.5, 0.5, 0.27, 0.0, -0.08])  # camera z = scan x, camera x = -scan y, camera y = -scan z


def runs_of(fn, reps, runs, warmup=3):
    for _ in range(warmup):
        fn()
    med = []
    for _ in range(runs):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        med.append(round(statistics.median(ms), 4))
    return {"runs": med, "median": round(statistics.median(med), 4), "min": min(med), "max": max(med), "reps_per_run": reps}


# ---- the host route: plain vectorised numpy ---------------------------------------------------------------------------------------
def np_project(xyz, p, mat):
    m = mat["cloud_to_cam"]
    pc = xyz.astype(np.float64) @ m[:, :3].T + m[:, 3]
    with np.errstate(all="ignore"):
        Z = pc[:, 2]
        x, y = pc[:, 0] / Z, pc[:, 1] / Z
        r2 = x * x + y * y
        rad = 1 + r2 * (p.k1 + r2 * (p.k2 + r2 * p.k3))
        u = p.fx * (x * rad + 2 * p.p1 * x * y + p.p2 * (r2 + 2 * x * x)) + p.cx
        v = p.fy * (y * rad + p.p1 * (r2 + 2 * y * y) + 2 * p.p2 * x * y) + p.cy
        col, row = np.floor(u + 0.5), np.floor(v + 0.5)
        ok = (Z >= p.min_depth) & (Z < p.max_depth) & (r2 <= p.max_tan_sq) & (col >= 0) & (col < p.width) & (row >= 0) & (row < p.height)
    idx = np.flatnonzero(ok)
    pix = (row[idx] * p.width + col[idx]).astype(np.int64)
    return idx, pix, Z.astype(np.float32), u, v


def np_image(xyz, lab, p, mat, per_point=True):
    n_px = p.width * p.height
    idx, pix, zf, u, v = np_project(xyz, p, mat)
    order = np.lexsort((idx, zf[idx], pix))
    first = np.ones(len(order), dtype=bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    wp, wi = pix[order][first], idx[order][first]
    index = np.full(n_px, -1, np.int32)
    index[wp] = wi
    depth = np.zeros(n_px, np.float32)
    depth[wp] = zf[wi]
    img = np.zeros((4, n_px), np.float32)
    img[:3, wp] = xyz[wi].T
    label = np.zeros(n_px, np.uint32)
    label[wp] = lab[wi]
    count = np.bincount(pix, minlength=n_px).astype(np.uint32)
    out = dict(index=index, depth=depth, xyz=img, label=label, count=count, idx=idx, pix=pix, zf=zf)
    if per_point:
        pixel = np.full(len(xyz), -1, np.int32)
        pixel[idx] = pix
        visible = np.zeros(len(xyz), np.uint8)
        visible[wi] = 1
        out.update(pixel=pixel, u=u.astype(np.float32), v=v.astype(np.float32), visible=visible)
    return out


def np_labels(xyz, lab, classes, p, mat):
    W, H, half = p.width, p.height, p.window // 2
    im = np_image(xyz, lab, p, mat, per_point=False)
    front = np.full((H + 2 * half, W + 2 * half), np.inf, np.float32)
    front[half:half + H, half:half + W] = np.where(im["index"] >= 0, im["depth"], np.float32(np.inf)).reshape(H, W)
    zmin = front[half:half + H, half:half + W].copy()
    for wr in range(2 * half + 1):
        for wc in range(2 * half + 1):
            np.minimum(zmin, front[wr:wr + H, wc:wc + W], out=zmin)
    idx, pix = im["idx"], im["pix"]
    zm = zmin.reshape(-1)[pix].astype(np.float64)
    seen = ~((im["zf"][idx].astype(np.float64) - zm) > (p.occlusion_abs + p.occlusion_rel * zm))
    cls = classes.reshape(-1)[pix]
    take = seen & (cls != 0)
    out = lab.copy()
    out[idx[take]] = cls[take]
    return out


def np_rays(p):
    c, r = np.meshgrid(np.arange(p.width, dtype=np.float64), np.arange(p.height, dtype=np.float64))
    xd, yd = (c - p.cx) / p.fx, (r - p.cy) / p.fy
    x, y = xd, yd
    for _ in range(p.undistort_iterations):
        r2 = x * x + y * y
        rad = 1 + r2 * (p.k1 + r2 * (p.k2 + r2 * p.k3))
        x, y = (xd - (2 * p.p1 * x * y + p.p2 * (r2 + 2 * x * x))) / rad, (yd - (p.p1 * (r2 + 2 * y * y) + 2 * p.p2 * x * y)) / rad
    return np.stack([x.reshape(-1), y.reshape(-1), np.ones(x.size)], axis=1)


def np_unproject(depth, rays, p, mat):
    Z = depth.reshape(-1).astype(np.float64) * p.depth_scale
    valid = (Z >= p.min_depth) & (Z < p.max_depth)
    m = mat["cam_to_cloud"]
    xyz = ((rays * Z[:, None]) @ m[:, :3].T + m[:, 3]).astype(np.float32)
    xyz[~valid] = np.nan
    return xyz, valid


def fold_kernel_stats(path, out):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "camera_" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no camera kernel row in {path}")
    kernels = {}
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        kernels[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                         "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    out["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (tools/camera_timing.py --trace)", "rows": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a --trace run under rocprofv3: folded into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "camera", "timing.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.load(f)
        fold_kernel_stats(a.kernel_stats, out)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["kernels"], indent=1))
        return
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    lab = lab.astype(np.uint32)
    n = len(xyz)
    p = sicp.default_camera_params(**KITTI)
    qt = ON_THE_SCANNER
    mat = sicp.camera_matrices(qt)
    fp = sicp.default_camera_params(k1=-0.0999, k2=0.3926, p1=0.0019, p2=-0.0013, k3=-0.6762)  # 640 x 480 with a lens
    rng = np.random.default_rng(4)
    depth = rng.integers(400, 8000, (480, 640)).astype(np.uint16)
    depth[rng.random((480, 640)) < 0.15] = 0
    frame_label = rng.integers(1, 12, (480, 640)).astype(np.uint32)
    gicp = sicp.default_params(sicp.MODE_GICP)
    with sicp.Engine(0, gicp) as e, sicp.Engine(0, gicp) as scan:
        e.set_source(xyz, lab)
        img = e.camera_image(sicp.SOURCE, p, qt, per_point=True)
        classes = np.where(img["label"] > 0, img["label"], 3).astype(np.uint32)  # the picture a perfect network would return, no pixel empty
        if a.trace:
            for _ in range(8):
                e.camera_image(sicp.SOURCE, p, qt, per_point=True)
                e.camera_labels(sicp.SOURCE, classes, p, qt)
                e.camera_labels(sicp.SOURCE, classes, sicp.default_camera_params(**dict(KITTI, window=15)), qt)
                e.camera_unproject(depth, fp, None, frame_label, dst=scan)
            return
        ref = camera_ref.labels(xyz, lab, classes, p, mat)
        got = e.camera_labels(sicp.SOURCE, classes, p, qt)
        fref = camera_ref.unproject(depth, fp, sicp.camera_matrices(None))
        fgot = e.camera_unproject(depth, fp)
        equal = all(img[k].tobytes() == ref["image"][k].tobytes() for k in camera_ref.IMAGES + camera_ref.PER_POINT) and \
            got["labels"].tobytes() == ref["labels"].tobytes() and got["state"].tobytes() == ref["state"].tobytes() and \
            fgot["xyz"].tobytes() == fref["xyz"].tobytes()
        # the plain numpy route says the same as the restatement wherever no point sits on a pixel edge
        plain = np_labels(xyz, lab, classes, p, mat)
        out = {"date": time.strftime("%Y-%m-%d"), "reps_per_run": a.reps, "runs": a.runs, "points": n, "image": [int(p.height), int(p.width)],
               "window": int(p.window), "frame": [480, 640], "frame_valid_pixels": int(fgot["info"]["n_valid"]),
               "info": {k: v for k, v in got["info"].items() if k != "t_total_ms"},
               "equal_to_the_restatement": bool(equal),
               "plain_numpy_labels_that_differ_from_the_restatement": int((plain != ref["labels"]).sum()),
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding; a run is the median of reps_per_run calls",
               "not_measured": ["more than one device", "clouds above 100 000 points", "other image sizes", "float32 depth frames"]}
        t = lambda fn: runs_of(fn, a.reps, a.runs)  # noqa: E731
        out["sicp_camera_image_every_output_ms"] = t(lambda: e.camera_image(sicp.SOURCE, p, qt, per_point=True))
        out["sicp_camera_image_no_per_point_ms"] = t(lambda: e.camera_image(sicp.SOURCE, p, qt))
        out["sicp_camera_labels_read_back_ms"] = t(lambda: e.camera_labels(sicp.SOURCE, classes, p, qt))
        out["sicp_camera_labels_dst_other_handle_ms"] = t(lambda: e.camera_labels(sicp.SOURCE, classes, p, qt, dst=scan, dst_which=sicp.SOURCE))
        out["sicp_camera_labels_dst_in_place_ms"] = t(lambda: e.camera_labels(sicp.SOURCE, classes, p, qt, dst=e))
        e.set_source(xyz, lab)
        out["sicp_camera_unproject_dst_ms"] = t(lambda: e.camera_unproject(depth, fp, None, frame_label, dst=scan, want_points=False))
        out["sicp_camera_unproject_dst_and_points_ms"] = t(lambda: e.camera_unproject(depth, fp, None, frame_label, dst=scan))
        rays = np_rays(fp)
        ident = sicp.camera_matrices(None)

        def host_labels():
            scan.set_source(xyz, np_labels(xyz, lab, classes, p, mat))

        def host_frame():
            pts, _ = np_unproject(depth, rays, fp, ident)
            scan.set_source(pts, frame_label.reshape(-1))

        out["numpy_image_ms"] = t(lambda: np_image(xyz, lab, p, mat))
        out["numpy_labels_ms"] = t(lambda: np_labels(xyz, lab, classes, p, mat))
        out["numpy_labels_and_set_cloud_ms"] = t(host_labels)
        out["numpy_unproject_cached_rays_and_set_cloud_ms"] = t(host_frame)
        out["numpy_rays_once_per_camera_ms"] = t(lambda: np_rays(fp))
        out["set_cloud_of_the_whole_scan_ms"] = t(lambda: scan.set_source(xyz, lab))
        pairs = {"sicp_camera_image_every_output_ms": "numpy_image_ms", "sicp_camera_labels_read_back_ms": "numpy_labels_ms",
                 "sicp_camera_labels_dst_other_handle_ms": "numpy_labels_and_set_cloud_ms",
                 "sicp_camera_labels_dst_in_place_ms": "numpy_labels_and_set_cloud_ms",
                 "sicp_camera_unproject_dst_ms": "numpy_unproject_cached_rays_and_set_cloud_ms"}
        out["against_numpy"] = {g: {"numpy": h, "ratio_of_medians": round(out[h]["median"] / out[g]["median"], 2),
                                    "beats_numpy": bool(out[g]["max"] < out[h]["min"])} for g, h in pairs.items()}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
