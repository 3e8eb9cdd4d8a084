#!/usr/bin/env python3
"""Times of sicp_filter on the GPU -> profiles/filter/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) (the cluster's generator): the statistical test (mean_k = 20), the
radius test (0.5 m, 2 neighbours), both together, and a pure selection by mask into dst -- the whole C call with every
per-point output.  Two comparisons from the same run: the host route the selection replaces (the mask applied in numpy and
sicp_set_cloud of the kept arrays; the sicp_cluster call that makes the mask is the same in both routes and timed beside them),
and one run of the numpy / scipy restatement (tests/filter_ref.py) per test, whose answer the call's must equal.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs only the call with both tests a few
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

import filter_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
ARRAYS = ("keep", "mean_dist", "neighbors")


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filter", "timing.json"))
    a = ap.parse_args()
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    P = sicp.default_filter_params
    tests = {"statistical_mean_k_20": dict(mean_k=20), "radius_0.5_2_neighbours": dict(mean_k=0, radius=0.5, min_neighbors=2),
             "both": dict(mean_k=20, radius=0.5, min_neighbors=2)}
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e, sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as scan:
        e.set_source(xyz, lab)
        if a.trace:
            for _ in range(6):
                e.filter(sicp.SOURCE, P(**tests["both"]))
            return
        out = {"reps": a.reps, "points": len(xyz), "tests": {}, "selection": {},
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding, every per-point output read back",
               "not_measured": ["more than one device", "clouds above 100 000 points", "kernel times"]}
        for name, kw in tests.items():
            p = P(**kw)
            row = {"sicp_filter_ms": timed(lambda: e.filter(sicp.SOURCE, p), a.reps)}
            got = e.filter(sicp.SOURCE, p)
            row["info"] = {k: v for k, v in got["info"].items() if k != "t_total_ms"}
            t = time.perf_counter()
            ref = filter_ref.filter(xyz, lab, None, kw.get("mean_k", 20), 2.0, kw.get("radius", 0.0), kw.get("min_neighbors", 2))
            row["restatement_on_the_cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            row["equal_to_the_restatement"] = all(got[k].tobytes() == ref[k].tobytes() for k in ARRAYS)
            out["tests"][name] = row
        # the same statistical test on a SEMANTIC handle: the cloud grouped by label, one search per label, the lists merged
        with sicp.Engine(0, sicp.default_params(sicp.MODE_SEMANTIC)) as sem:
            sem.set_source(xyz, lab)
            p = P(mean_k=20)
            row = {"labels": int(len(np.unique(lab))), "sicp_filter_ms": timed(lambda: sem.filter(sicp.SOURCE, p), a.reps)}
            row["equal_to_the_flat_handle"] = all(sem.filter(sicp.SOURCE, p)[k].tobytes() == e.filter(sicp.SOURCE, p)[k].tobytes() for k in ARRAYS)
            out["tests"]["statistical_mean_k_20_semantic_handle"] = row
        # the selection: speckle leaves (the INTEGRATION.md recipe), on the device and on the host
        cp = sicp.default_cluster_params(ignore=(1, 2), tolerance=0.5, min_points=10)
        out["selection"]["sicp_cluster_ms_same_in_both_routes"] = timed(lambda: e.cluster(sicp.SOURCE, cp), a.reps)
        cid = e.cluster(sicp.SOURCE, cp)["cluster_id"]
        sel = P(mean_k=0)

        def device_route():
            keep = ((cid >= 0) | np.isin(lab, (1, 2))).astype(np.uint8)
            e.filter(sicp.SOURCE, sel, keep, dst=scan, dst_which=sicp.SOURCE)

        def host_route():
            keep = (cid >= 0) | np.isin(lab, (1, 2))
            scan.set_source(xyz[keep], lab[keep])

        out["selection"]["filter_mask_dst_ms"] = timed(device_route, a.reps)
        out["selection"]["numpy_mask_and_set_cloud_ms"] = timed(host_route, a.reps)
        out["selection"]["set_cloud_of_the_whole_scan_ms"] = timed(lambda: scan.set_source(xyz, lab), a.reps)
        out["selection"]["points_kept"] = int(((cid >= 0) | np.isin(lab, (1, 2))).sum())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
