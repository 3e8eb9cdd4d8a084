#!/usr/bin/env python3
"""Times of the place database on the GPU -> profiles/place/timing.json.

One describe of a 100 K-point scan (both channels); one query against 1 K, 10 K and 100 K entries at 20 x 60 (random
descriptors through add_descriptors); a 16-query batch at 10 K entries; beside them the time of the numpy restatement
(tests/place_ref.py) for the same query, the HBM floor of reading the entries once, and the loop-closure figures of the scene of
tests/place_cases.py (the two registrations' distances that tests/test_gpu_place.py asserts on).

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up of the same shape; the median, minimum and maximum of `--reps` calls.  The times are whole calls: upload of the query,
kernels, sort, read-back.  No kernel trace is taken here."""
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

import place_cases as PC  # noqa: E402
import place_ref as PR  # noqa: E402
import synth  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")
HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X, HBM3E


def timed(fn, reps, warmup=2):
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
    ap.add_argument("--sizes", type=int, nargs="*", default=[1000, 10000, 100000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place", "timing.json"))
    a = ap.parse_args()
    R, S, C = 20, 60, 11
    out = {"shape": [R, S], "num_classes": C, "reps": a.reps,
           "clock": "time.perf_counter() around synchronous calls, after 2 warm-up calls of the same shape; whole calls",
           "not_measured": ["kernel times (no kernel trace was taken)", "shapes other than 20 x 60", "more than one device"]}

    # describe: a 100 K-point scan of the street
    xyz, lab, _, _, _, _ = synth.lidar_pair(seed=2, n_points=100_000)
    p = sicp.default_params(sicp.MODE_GICP)
    with sicp.Engine(0, p) as e:
        e.set_source(xyz, lab)
        out["describe_100k_points_ms"] = {}
        for name, ch in (("label", sicp.PLACE_LABEL), ("height", sicp.PLACE_HEIGHT)):
            with sicp.PlaceDB(0, sicp.default_place_params(channel=ch, num_classes=C)) as db:
                out["describe_100k_points_ms"][name] = timed(lambda: db.describe(e), a.reps)

    # search: random descriptors
    rng = np.random.default_rng(1)
    out["query_ms"] = {}
    with sicp.PlaceDB(0, sicp.default_place_params(num_classes=C)) as db:
        have = 0
        for n in a.sizes:
            while have < n:
                m = min(n - have, 20000)
                d = rng.integers(0, C + 1, (m, R, S)).astype(np.uint8)
                db.add_descriptors(d)
                have += m
            q = rng.integers(0, C + 1, (R, S)).astype(np.uint8)
            row = {"entries": n, "one_query": timed(lambda: db.query(q, top_k=5), a.reps),
                   "entry_bytes": n * R * S,
                   "hbm_floor_ms_reading_the_entries_once": round(n * R * S / HBM_PEAK_BYTES_PER_S * 1e3, 5)}
            if n == 10000:
                qs = rng.integers(0, C + 1, (16, R, S)).astype(np.uint8)
                row["batch_of_16_queries"] = timed(lambda: db.query(qs, top_k=5), a.reps)
                row["sixteen_lone_queries"] = timed(lambda: [db.query(qs[i], top_k=5) for i in range(16)], max(a.reps // 4, 2))
            if n <= 1000:  # the restatement for the same query (numpy on the host; one run)
                entries = db.get()
                t = time.perf_counter()
                want = PR.query(q, entries, top_k=5)
                row["numpy_restatement_ms"] = round((time.perf_counter() - t) * 1e3, 1)
                row["equal_to_the_restatement"] = db.query(q, top_k=5) == want
            out["query_ms"][str(n)] = row

    # the loop from a query to a registration, on the scene of the tests
    sc = PC.scene()
    with sicp.PlaceDB(0, sicp.default_place_params(num_classes=PC.SCENE_CLASSES, max_range=PC.SCENE_RANGE)) as db:
        with sicp.Engine(0, p) as e:
            for xyz, lab in sc["entries"]:
                e.set_source(xyz, lab)
                db.add(e)
        rows = []
        for k in range(4):
            f = PC.loop_closure_figures(db, sc, k)
            top = f.pop("candidates")
            f["top"] = top[0]
            f["runner_up_score"] = top[1]["score"]
            rows.append(f)
        out["loop_closure"] = {"distances": "(rotation rad, translation m)", "revisits": rows}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
