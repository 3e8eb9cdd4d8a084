#!/usr/bin/env python3
"""Times of sicp_deskew on the GPU -> profiles/deskew/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) with a time per point by azimuth and the 33 knots of a constant twist
(30 m/s, 1 rad/s over 0.1 s): the whole C call through the Python binding without dst (the points read back), with dst = the
handle itself (deskewed in place: the points become the slot's cloud, indexed, without being read back by the caller), and the
host route the call replaces: the same deskew vectorised in numpy (tests/deskew_ref.py on the same relative knots) followed by
sicp_set_cloud of the result -- timed in the same process; set_cloud alone beside them, since both routes with a new cloud pay it.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs only the call without dst a few
times, for a run under `rocprofv3 --kernel-trace --stats` (tools/README.md); --kernel-stats folds that run's kernel row into the
JSON beside the bytes the kernel moves."""
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

import deskew_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
N_KNOTS = 33
TWIST = np.array([3.0, 0.1, 0.0, 0.0, 0.01, 0.1])
T0, T1 = 0.0, 0.1


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def kernel_bytes(n, n_knots, groups):
    """what the kernel reads and writes: x y z (12) + time (8) in, x y z (12) out per point; the table once per workgroup"""
    return 32 * n + groups * 64 * n_knots


def fold_kernel_stats(path, out):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "deskew_kernel" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no deskew_kernel row in {path}")
    r = rows[0]
    calls, avg_ns = int(r["Calls"]), float(r["AverageNs"])
    n = out["points"]
    groups = min((n + 255) // 256, 512)  # kDeskewMaxGroups (csrc/kernels.h)
    b = kernel_bytes(n, N_KNOTS, groups)
    out["kernel"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (tools/deskew_timing.py --trace)", "calls": calls,
                     "average_us": round(avg_ns / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3), "max_us": round(float(r["MaxNs"]) / 1e3, 3),
                     "bytes": b, "gb_per_s": round(b / avg_ns, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a --trace run under rocprofv3: folded into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deskew", "timing.json"))
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            out = json.load(f)
        fold_kernel_stats(a.kernel_stats, out)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["kernel"], indent=1))
        return
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    n = len(xyz)
    times = T0 + (np.arctan2(xyz[:, 1], xyz[:, 0]).astype(np.float64) + np.pi) / (2 * np.pi) * (T1 - T0)
    kt, kq = sicp.deskew_twist_knots(deskew_ref.se3_exp(TWIST), T0, T1, N_KNOTS)
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e, sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as scan:
        e.set_source(xyz, lab)
        if a.trace:
            for _ in range(8):
                e.deskew(sicp.SOURCE, times, kt, kq)
            return
        got = e.deskew(sicp.SOURCE, times, kt, kq)
        K = got["knots"]
        ref = deskew_ref.deskew(xyz, times, kt, K)
        out = {"date": time.strftime("%Y-%m-%d"), "reps": a.reps, "points": n, "knots": N_KNOTS,
               "info": {k: v for k, v in got["info"].items() if k != "t_total_ms"},
               "equal_to_the_restatement": got["points"].tobytes() == ref["points"].tobytes(),
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding",
               "not_measured": ["more than one device", "clouds above 100 000 points", "times that are not sorted"]}
        out["sicp_deskew_no_dst_points_read_back_ms"] = timed(lambda: e.deskew(sicp.SOURCE, times, kt, kq), a.reps)
        out["sicp_deskew_no_dst_no_points_ms"] = timed(lambda: e.deskew(sicp.SOURCE, times, kt, kq, want_points=False), a.reps)

        def device_route():  # the raw scan is in the slot (its upload is the same in both routes); deskewed into `scan`'s slot
            e.deskew(sicp.SOURCE, times, kt, kq, dst=scan, dst_which=sicp.SOURCE, want_points=False)

        def in_place():  # every call deskews the previous call's result: the same shape and work
            e.deskew(sicp.SOURCE, times, kt, kq, dst=e, want_points=False)

        def host_route():
            scan.set_source(deskew_ref.deskew(xyz, times, kt, K)["points"], lab)

        out["sicp_deskew_dst_other_handle_ms"] = timed(device_route, a.reps)
        out["sicp_deskew_dst_in_place_ms"] = timed(in_place, a.reps)
        out["numpy_deskew_and_set_cloud_ms"] = timed(host_route, a.reps)
        out["numpy_deskew_alone_ms"] = timed(lambda: deskew_ref.deskew(xyz, times, kt, K), a.reps)
        out["set_cloud_of_the_whole_scan_ms"] = timed(lambda: scan.set_source(xyz, lab), a.reps)
        out["host_route_over_dst_in_place"] = round(out["numpy_deskew_and_set_cloud_ms"]["median"] / out["sicp_deskew_dst_in_place_ms"]["median"], 2)
        out["host_route_over_dst_other_handle"] = round(out["numpy_deskew_and_set_cloud_ms"]["median"] / out["sicp_deskew_dst_other_handle_ms"]["median"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
