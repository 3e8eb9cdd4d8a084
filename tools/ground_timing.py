#!/usr/bin/env python3
"""Times of sicp_segment_ground on the GPU -> profiles/ground/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) (the scan of the cluster, filter and plane profiles; the sensor at the
origin 1.73 m over the road), the defaults and two other grids: the whole C call through the Python binding with every output
read back; the same with select = 1 into another handle; and in place (the cloud is set again before every call, outside the
clock).  Beside them one run of the numpy restatement (tests/ground_ref.py), whose bytes the call's must equal, and
sicp_segment_planes with one plane on the same scan (profiles/plane/timing.json has its history).

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs the default call a few times, for a
run under `rocprofv3 --kernel-trace --stats`; --kernel-trace FILE reads that run's kernel trace csv and adds the kernels' times,
the fit kernel's against the bytes its 2 n_iter + 1 passes move, and the share of the longest cell, to the json."""
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

import ground_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
INTS = ("ground", "cell", "status", "n_members", "n_ground", "n_fit")
DOUBLES = ("height", "normal", "centroid", "lambda_min", "lpr")
TRACE_CALLS = 6
GRIDS = {"defaults_16x32": {}, "8x16": dict(n_rings=8, n_sectors=16), "64x256": dict(n_rings=64, n_sectors=256, elevation_rings=16)}


def timed(fn, reps, warmup=3, before=None):
    ms = []
    for k in range(warmup + reps):
        if before:
            before()
        t = time.perf_counter()
        fn()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def equal(got, ref):
    ok = all(got[k].tobytes() == ref[k].astype(got[k].dtype).tobytes() for k in INTS)
    for k in DOUBLES:
        a, b = np.array(got[k]), np.array(ref[k], np.float64)
        ok = ok and bool((np.isnan(a) == np.isnan(b)).all()) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()
    return ok


def kernel_stats(path, out):
    dur = {}
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if "ground_" in name or "rocprim" in name:
            short = name.split("(anonymous namespace)::")[-1].split("(")[0] if "ground_" in name else "rocprim: " + name.split("<")[0].split("::")[-1]
            dur.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    st = lambda v: {"launches": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}  # noqa: E731
    res = {"source": "rocprofv3 --kernel-trace --stats of `ground_timing.py --trace`, a run of its own", "kernels": {k: st(v) for k, v in dur.items()}}
    fit = next((v for k, v in dur.items() if "fit" in k), None)
    row = out["settings"]["defaults_16x32"]
    if fit:
        n_iter, cand, longest = 3, row["info"]["n_candidates"], row["longest_cell"]
        passes = 2 * n_iter + 1
        us = statistics.median(fit[1:] if len(fit) > 1 else fit)
        res["fit_kernel"] = {"median_us": round(us, 2), "passes": passes, "bytes_per_member_and_pass": 12, "bytes_moved": cand * 12 * passes,
                             "GB_per_s": round(cand * 12 * passes / us / 1e3, 2), "longest_cell_members": longest,
                             "longest_cell_share_of_candidates": round(longest / cand, 4),
                             "longest_cell_bytes": longest * 12 * passes,
                             "longest_cell_GB_per_s_if_it_alone_set_the_time": round(longest * 12 * passes / us / 1e3, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ground", "timing.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        with open(a.out) as f:
            out = json.load(f)
        out["kernel_trace"] = kernel_stats(a.kernel_trace, out)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["kernel_trace"], indent=1))
        return
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    P = sicp.default_ground_params
    S = sicp.SOURCE
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e, sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as other:
        e.set_source(xyz, lab)
        if a.trace:
            for _ in range(TRACE_CALLS):
                e.segment_ground(S, P())
            return
        out = {"reps": a.reps, "points": len(xyz), "settings": {},
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding, every output read back",
               "not_measured": ["more than one device", "clouds above 100 000 points", "a caller's ring table", "labels ignored, a mask"]}
        for name, kw in GRIDS.items():
            row = {"sicp_segment_ground_ms": timed(lambda: e.segment_ground(S, P(**kw)), a.reps)}
            got = e.segment_ground(S, P(**kw))
            row["info"] = {k: v for k, v in got["info"].items() if k != "t_total_ms"}
            row["longest_cell"] = int(got["n_members"].max())
            t = time.perf_counter()
            ref = ground_ref.segment_ground(xyz, lab, **kw)
            row["restatement_on_the_cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            row["equal_to_the_restatement"] = equal(got, ref)
            if name == "defaults_16x32":
                row["with_dst_select_1_ms"] = timed(lambda: e.segment_ground(S, P(select=1), dst=other, dst_which=S), a.reps)
                row["n_selected"] = other.n[S]
                row["in_place_select_1_ms"] = timed(lambda: e.segment_ground(S, P(select=1), dst=e), a.reps, before=lambda: e.set_source(xyz, lab))
                e.set_source(xyz, lab)
                row["set_source_alone_ms"] = timed(lambda: e.set_source(xyz, lab), a.reps)
                pp = sicp.default_plane_params(distance_threshold=0.2, axis=(0, 0, 1), min_cos=0.95, num_hypotheses=256, max_planes=1)
                row["sicp_segment_planes_one_plane_H_256_ms"] = timed(lambda: e.segment_planes(S, pp), a.reps)
            out["settings"][name] = row
            print(name, json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
