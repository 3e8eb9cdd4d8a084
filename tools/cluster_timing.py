#!/usr/bin/env python3
"""Times of sicp_cluster on the GPU -> profiles/cluster/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) with labels 1 and 2 ignored and same_label = 1, at tolerance 0.5 and
0.3: the whole C call with every output array (sized by a call before the clock starts); the same through Engine.cluster (which
makes the sizing call each time); beside them sicp_merge_clouds of the same cloud at leaf_size = tolerance (the same sort plus
linear passes: a floor) and one run of the numpy / scipy restatement (tests/cluster_ref.py), whose answer the call's must equal.
Worst-case shapes: one cluster of 100 000 points as a sheet (the ordered centroid sum of one cluster is serial) and as a dense
ball (about 3 000 points per cell: the pair pass).

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs only the 0.5 street call a few
times, for a run under `rocprofv3 --kernel-trace --stats` (tools/README.md)."""
from __future__ import annotations

import argparse
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

import cluster_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
TABLE = ("cluster_id", "label", "count", "first_index", "centroid", "bbox_min", "bbox_max")


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def raw_call(e, p):
    """the C call with arrays of its own, sized once: -> (a function that makes the call, the sizing call's info)"""
    info = e.cluster(sicp.SOURCE, p)["info"]
    n, k = max(info["n_points"], 1), max(info["n_clusters"], 1)
    cid, cnt, first = np.empty(n, np.int32), np.empty(k, np.int32), np.empty(k, np.int32)
    lab, cen = np.empty(k, np.uint32), np.empty((k, 3), np.float64)
    lo, hi = np.empty((k, 3), np.float32), np.empty((k, 3), np.float32)
    ip, up, fp, dp = (C.POINTER(t) for t in (C.c_int32, C.c_uint32, C.c_float, C.c_double))
    out = sicp.SicpClusterInfo()

    def call():
        rc = sicp.lib().sicp_cluster(e._h, sicp.SOURCE, C.byref(p), cid.ctypes.data_as(ip), k, lab.ctypes.data_as(up), cnt.ctypes.data_as(ip),
                                     first.ctypes.data_as(ip), cen.ctypes.data_as(dp), lo.ctypes.data_as(fp), hi.ctypes.data_as(fp), C.byref(out))
        assert rc == sicp.OK, rc

    return call, info


def shape_row(e, xyz, lab, p, reps):
    e.set_source(xyz, lab)
    call, info = raw_call(e, p)
    return {"points": len(xyz), "info": {k: v for k, v in info.items() if k != "t_total_ms"}, "sicp_cluster_ms": timed(call, reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster", "timing.json"))
    a = ap.parse_args()
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    P = sicp.default_cluster_params
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e:
        if a.trace:
            e.set_source(xyz, lab)
            call, _ = raw_call(e, P(ignore=(1, 2), tolerance=0.5))
            for _ in range(6):
                call()
            return
        out = {"reps": a.reps, "street_scan_100k": {}, "one_cluster_of_100k": {},
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls",
               "not_measured": ["more than one device", "clouds above 100 000 points"]}
        for tol in (0.5, 0.3):
            p = P(ignore=(1, 2), tolerance=tol)
            row = shape_row(e, xyz, lab, p, a.reps)
            row["engine_cluster_ms_sizing_call_included"] = timed(lambda: e.cluster(sicp.SOURCE, p), a.reps)
            mp = sicp.default_merge_params(leaf_size=tol)
            row["sicp_merge_clouds_same_cloud_leaf_eq_tolerance_ms"] = timed(lambda: sicp.merge_clouds([(e, sicp.SOURCE)], None, mp), a.reps)
            t = time.perf_counter()
            ref = cluster_ref.cluster(xyz, lab, tol, 10, 0, 1, (1, 2))
            row["restatement_on_the_cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            got = e.cluster(sicp.SOURCE, p)
            row["equal_to_the_restatement"] = all(got[k].tobytes() == ref[k].tobytes() for k in TABLE)
            out["street_scan_100k"][str(tol)] = row
        # one cluster of 100 000 points
        one = P(tolerance=0.5, min_points=1)
        u, v = np.meshgrid(np.arange(250) * 0.45, np.arange(400) * 0.45, indexing="ij")
        sheet = np.stack([u.ravel(), v.ravel(), 0.05 * np.sin(u.ravel())], axis=1).astype(np.float32)
        out["one_cluster_of_100k"]["sheet_spacing_0.9_tolerance"] = shape_row(e, sheet, np.full(len(sheet), 3, np.uint32), one, a.reps)
        rng = np.random.default_rng(1)
        d = rng.normal(size=(100_000, 3))
        d *= (1.0 * rng.uniform(0, 1, 100_000) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        ball = d.astype(np.float32)
        out["one_cluster_of_100k"]["ball_radius_2_tolerances"] = shape_row(e, ball, np.full(len(ball), 3, np.uint32), one, max(a.reps // 4, 3))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
