#!/usr/bin/env python3
"""Times of sicp_segment_planes on the GPU -> profiles/plane/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) (the cluster's and the filter's generator), distance_threshold 0.1, no
axis: H in {256, 1024, 4096} x max_planes in {1, 4} x refine in {0, 1} -- the whole C call through the Python binding with
every output read back.  Beside each, one run of the numpy restatement (tests/plane_ref.py), whose bytes the call's must equal:
that host time is the comparison, there is no earlier form of the call.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs only H = 1024 and H = 4096 with one
plane and refine = 1 a few times, for a run under `rocprofv3 --kernel-trace --stats`; --kernel-trace FILE reads that run's
kernel trace csv and adds the score kernel's time and its share of the FP64 issue floor to the json."""
from __future__ import annotations

import argparse
import csv
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import plane_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
ARRAYS = ("plane_id", "coeff", "count", "hyp_index", "hyp_count", "centroid", "rms")
T = 0.1
TRACE_H = (1024, 4096)
TRACE_CALLS = 6
# the floor of the score kernel: FP64 vector instructions per point-plane test in its loop (v_add_f64 x 5, v_mul_f64 x 4,
# v_cmp_le_f64 x 1: the disassembly of plane_score_kernel) over the chip's FP64 vector issue rate, 256 CUs x 4 SIMDs x 16 lanes
# per cycle x 2.4 GHz = 39.3e12 lane-instructions per second (78.6 TFLOP/s counts a fused multiply-add as two)
FP64_PER_TEST = 10
FP64_LANE_RATE = 256 * 4 * 16 * 2.4e9


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def kernel_stats(path, points):
    """per kernel of the call, from rocprofv3's kernel trace csv: launches and times; the score kernel's launches alternate between
    H = 1024 and H = 4096 (one plane each), the first call of either is left out as warm-up"""
    dur = {}
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = r["Kernel_Name"]
        if "plane_" in name:
            short = name.split("(anonymous namespace)::")[-1].split("(")[0]
            dur.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    st = lambda v: {"launches": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    out = {"source": "rocprofv3 --kernel-trace --stats of `plane_timing.py --trace`, a run of its own", "kernels": {k: st(v) for k, v in dur.items()}}
    score = next((v for k, v in dur.items() if "score" in k), None)
    if score and len(score) == TRACE_CALLS * len(TRACE_H):
        out["score_kernel"] = {"fp64_instructions_per_test": FP64_PER_TEST, "lane_instructions_per_second": FP64_LANE_RATE}
        for k, H in enumerate(TRACE_H):
            mine = score[k::len(TRACE_H)][1:]
            floor = points * H * FP64_PER_TEST / FP64_LANE_RATE * 1e6
            out["score_kernel"][f"H_{H}"] = dict(st(mine), tests=points * H, floor_us=round(floor, 2),
                                                 fraction_of_floor=round(floor / statistics.median(mine), 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane", "timing.json"))
    a = ap.parse_args()
    if a.kernel_trace:
        with open(a.out) as f:
            out = json.load(f)
        out["kernel_trace"] = kernel_stats(a.kernel_trace, out["points"])
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
        print(json.dumps(out["kernel_trace"], indent=1))
        return
    xyz, lab, *_ = synth.lidar_pair(seed=2, n_points=100_000)
    P = sicp.default_plane_params
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e:
        e.set_source(xyz, lab)
        if a.trace:
            for _ in range(TRACE_CALLS):
                for H in TRACE_H:
                    e.segment_planes(sicp.SOURCE, P(distance_threshold=T, num_hypotheses=H))
            return
        out = {"reps": a.reps, "points": len(xyz), "distance_threshold": T, "settings": {},
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding, every output read back",
               "not_measured": ["more than one device", "clouds above 100 000 points", "an axis constraint"]}
        for H in (256, 1024, 4096):
            for planes in (1, 4):
                for refine in (0, 1):
                    kw = dict(distance_threshold=T, num_hypotheses=H, max_planes=planes, refine=refine)
                    p = P(**kw)
                    row = {"sicp_segment_planes_ms": timed(lambda: e.segment_planes(sicp.SOURCE, p), a.reps)}
                    got = e.segment_planes(sicp.SOURCE, p)
                    row["info"] = {k: v for k, v in got["info"].items() if k != "t_total_ms"}
                    row["count"] = got["count"].tolist()
                    t = time.perf_counter()
                    ref = plane_ref.segment_planes(xyz, lab, None, **kw)
                    row["restatement_on_the_cpu_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                    row["equal_to_the_restatement"] = all(got[k].tobytes() == ref[k].tobytes() for k in ARRAYS)
                    out["settings"][f"H_{H}_planes_{planes}_refine_{refine}"] = row
                    print(f"H {H} planes {planes} refine {refine}: {row['sicp_segment_planes_ms']} cpu {row['restatement_on_the_cpu_ms']} equal {row['equal_to_the_restatement']}", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
