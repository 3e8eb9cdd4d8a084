#!/usr/bin/env python3
"""Times of sicp_range_image / sicp_range_labels on the GPU -> profiles/range_image/timing.json.

The 100 K-point source scan of synth.lidar_pair(seed=2) projected at 64 x 2048 with the default parameters: the whole C calls
through the Python binding -- the image with every output read back; the vote (window 5, k 5) with the labels read back, into
another handle, and in place -- and the host route they replace: the vectorised numpy projection and windowed vote of
tests/range_ref.py, and the sicp_set_cloud the relabelled cloud needs, timed in the same process on the same host.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  --trace runs the image and the vote at window 5
and at window 7, k 16 a few times, for a run under `rocprofv3 --kernel-trace --stats` (tools/README.md); --kernel-stats folds that
run's kernel rows into the JSON, the vote kernel's beside its L2-gather floor."""
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

import range_ref  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
L2_GB_PER_S = 16800.0  # a gather served from the XCDs' L2, chip-wide, whole rows: the lower end of the 16.8-18.8 TB/s measured on MI355X


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"n": reps, "median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def fold_kernel_stats(path, out):
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if "range_" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no range kernel row in {path}")
    n = out["in_view_points"]
    kernels = {}
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        kernels[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 3), "min_us": round(float(r["MinNs"]) / 1e3, 3),
                         "max_us": round(float(r["MaxNs"]) / 1e3, 3)}
    out["kernels"] = {"source": "rocprofv3 --kernel-trace --stats, a run of its own (tools/range_timing.py --trace)", "rows": kernels}
    for name, k in kernels.items():
        if "range_vote_kernel<16>" in name:  # the --trace run's window 7, k 16 calls
            floor_bytes = 49 * 16 * n
            floor_us = floor_bytes / (L2_GB_PER_S * 1e3)
            k["gather_floor"] = {"bytes": floor_bytes, "assumed_l2_gb_per_s": L2_GB_PER_S, "floor_us": round(floor_us, 3),
                                 "achieved_fraction": round(floor_us / k["average_us"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernel-stats", help="the kernel_stats.csv of a --trace run under rocprofv3: folded into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range_image", "timing.json"))
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
    n = len(xyz)
    p = sicp.default_range_params()
    wide = sicp.default_range_params(window=7, k=16)
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e, sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as scan:
        e.set_source(xyz, lab)
        img = e.range_image(sicp.SOURCE, p)
        classes = img["label"]  # the picture a perfect network would return
        if a.trace:
            for _ in range(8):
                e.range_image(sicp.SOURCE, p)
                e.range_labels(sicp.SOURCE, classes, p)
                e.range_labels(sicp.SOURCE, classes, wide)
            return
        tab = sicp.range_tables(p)
        ref = range_ref.vote(xyz, lab, classes, p, tab)
        got = e.range_labels(sicp.SOURCE, classes, p)
        equal = all(img[k].tobytes() == ref["image"][k].tobytes() for k in range_ref.IMAGES + ("pixel", "visible")) and \
            got["labels"].tobytes() == ref["labels"].tobytes() and got["votes"].tobytes() == ref["votes"].tobytes()
        out = {"date": time.strftime("%Y-%m-%d"), "reps": a.reps, "points": n, "image": [int(p.height), int(p.width)], "window": int(p.window),
               "k": int(p.k), "in_view_points": int((img["pixel"] >= 0).sum()),
               "info": {k: v for k, v in got["info"].items() if k != "t_total_ms"},
               "equal_to_the_restatement": bool(equal),
               "clock": "time.perf_counter() around synchronous calls, after 3 warm-up calls of the same shape; whole calls through "
                        "the Python binding",
               "not_measured": ["more than one device", "clouds above 100 000 points", "images other than 64 x 2048"]}
        out["sicp_range_image_every_output_ms"] = timed(lambda: e.range_image(sicp.SOURCE, p), a.reps)
        out["sicp_range_image_no_per_point_ms"] = timed(lambda: e.range_image(sicp.SOURCE, p, per_point=False), a.reps)
        out["sicp_range_labels_read_back_ms"] = timed(lambda: e.range_labels(sicp.SOURCE, classes, p), a.reps)
        out["sicp_range_labels_window7_k16_read_back_ms"] = timed(lambda: e.range_labels(sicp.SOURCE, classes, wide), a.reps)
        out["sicp_range_labels_dst_other_handle_ms"] = timed(lambda: e.range_labels(sicp.SOURCE, classes, p, dst=scan, dst_which=sicp.SOURCE), a.reps)
        out["sicp_range_labels_dst_in_place_ms"] = timed(lambda: e.range_labels(sicp.SOURCE, classes, p, dst=e), a.reps)
        e.set_source(xyz, lab)

        def host_route():
            scan.set_source(xyz, range_ref.vote(xyz, lab, classes, p, tab)["labels"])

        out["numpy_image_ms"] = timed(lambda: range_ref.image(xyz, lab, p, tab), a.reps)
        out["numpy_vote_ms"] = timed(lambda: range_ref.vote(xyz, lab, classes, p, tab), max(a.reps // 4, 3), warmup=1)
        out["numpy_vote_and_set_cloud_ms"] = timed(host_route, max(a.reps // 4, 3), warmup=1)
        out["set_cloud_of_the_whole_scan_ms"] = timed(lambda: scan.set_source(xyz, lab), a.reps)
        out["numpy_image_over_sicp_range_image"] = round(out["numpy_image_ms"]["median"] / out["sicp_range_image_every_output_ms"]["median"], 2)
        out["host_route_over_dst_in_place"] = round(out["numpy_vote_and_set_cloud_ms"]["median"] / out["sicp_range_labels_dst_in_place_ms"]["median"], 2)
        out["host_route_over_dst_other_handle"] = round(out["numpy_vote_and_set_cloud_ms"]["median"] / out["sicp_range_labels_dst_other_handle_ms"]["median"], 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
