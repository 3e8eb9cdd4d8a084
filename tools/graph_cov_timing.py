#!/usr/bin/env python3
"""Times of the pose-graph covariances on the GPU -> profiles/graph_cov/timing.json.

Graphs: the rings with closures of tools/pose_graph_timing.py (n nodes, 3 n edges).
  * --sizes (10^4 and 10^5 nodes): the time per lock-step CG iteration at 6, 12, 24 and 48 columns (48: two chunks of the
    24-column SpMM): marginals of columns / 6 nodes with the tolerance at 1e-300, held to exactly 64 and to 256 iterations; the
    difference over 192.  Beside it the single-column iteration of sicp_graph_optimize, measured the same way in the same process.
  * --solve-sizes (10^3, 4 x 10^3 and 10^4 nodes): the iterations and the wall time of one marginal and of a batch of 8 relative
    covariances at the default tolerance (1e-10), with the automatic iteration limit (20 x the node count) or --max-iterations,
    whichever is smaller.

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after a
warm-up run of the same shape; the median, minimum and maximum of `--reps` runs.  No kernel trace is taken here."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pose_graph_timing import graph, spread, timed_optimize  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")


def timed(call, reps, warmup=1):
    ms, out = [], None
    for k in range(warmup + reps):
        t = time.perf_counter()
        out = call()
        if k >= warmup:
            ms.append((time.perf_counter() - t) * 1e3)
    return spread(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--solve-reps", type=int, default=3, help="runs of the solves at the default tolerance")
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000])
    ap.add_argument("--columns", type=int, nargs="*", default=[6, 12, 24, 48])
    ap.add_argument("--solve-sizes", type=int, nargs="*", default=[1_000, 4_000, 10_000])
    ap.add_argument("--max-iterations", type=int, default=40_000, help="the iteration limit of the solves at the default tolerance")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_cov", "timing.json"))
    a = ap.parse_args()
    out = {"reps": a.reps,
           "clock": "time.perf_counter() around synchronous calls, after a warm-up run of the same shape; whole calls, in ms",
           "not_measured": ["kernel times (no kernel trace was taken)", "more than one device", "graphs other than the ring with closures"],
           "graphs": {}, "solves": {}}
    for n in a.sizes:
        g = graph(n)
        row = {"nodes": n, "edges": len(g["ei"])}
        # the single-column iteration of the optimiser, as tools/pose_graph_timing.py measures it
        held = {}
        for k in (64, 256):
            p = sicp.default_graph_params(max_iterations=1, max_cg_iterations=k, cg_eta=1e-300, gradient_tolerance=0.0)
            held[k], hinfo = timed_optimize(g, p, a.reps)
            assert hinfo["cg_iterations"] == k, hinfo
        single = (held[256]["median"] - held[64]["median"]) / 192.0
        row["optimize_ms_per_cg_iteration"] = round(single, 5)
        rng = np.random.default_rng(5)
        with sicp.PoseGraph(0) as pg:
            pg.add_nodes(g["poses"], g["fixed"])
            pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
            per = {}
            for cols in a.columns:
                nodes = rng.choice(np.arange(1, n), size=cols // 6, replace=False).astype(np.int32)
                held = {}
                for k in (64, 256):
                    p = sicp.default_graph_cov_params(tolerance=1e-300, max_cg_iterations=k, check_every=64, max_columns=cols)
                    held[k], (_, st, info) = timed(lambda: pg.marginals(nodes, p), a.reps)
                    assert info["cg_iterations"] == k and info["passes"] == 1 and np.all(st == sicp.GRAPH_COV_NOT_CONVERGED), info
                ms = (held[256]["median"] - held[64]["median"]) / 192.0
                per[str(cols)] = {"with_64_iterations_ms": held[64], "with_256_iterations_ms": held[256], "ms_per_iteration": round(ms, 5),
                                  "us_per_iteration_and_column": round(ms * 1e3 / cols, 3),
                                  "against_as_many_single_column_iterations": round(ms / (cols * single), 3) if single > 0 else None}
            row["lock_step_cg"] = per
        out["graphs"][str(n)] = row
        print(json.dumps(row, indent=1), flush=True)
    for n in a.solve_sizes:
        g = graph(n)
        row = {"nodes": n, "edges": len(g["ei"]), "iteration_limit": min(a.max_iterations, max(20 * n, 200))}
        rng = np.random.default_rng(5)
        with sicp.PoseGraph(0) as pg:
            pg.add_nodes(g["poses"], g["fixed"])
            pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
            p = sicp.default_graph_cov_params(max_cg_iterations=row["iteration_limit"])
            node = np.array([n // 2], dtype=np.int32)
            ms, (_, st, info) = timed(lambda: pg.marginals(node, p), a.solve_reps)
            row["one_marginal_at_1e-10"] = {"ms": ms, "status": sicp.GRAPH_COV_STATUSES[int(st[0])], "info": info,
                                            "iterations_per_node": round(info["cg_iterations"] / n, 2)}
            qa = rng.choice(np.arange(1, n), size=8, replace=False).astype(np.int32)
            qb = ((qa + rng.integers(2, n // 2, size=8)) % n).astype(np.int32)
            qb[qb == 0] = 1
            qb[qb == qa] += 1
            ms, (_, st, info) = timed(lambda: pg.relative_covariances(qa, qb, p), a.solve_reps)
            row["eight_relative_covariances_at_1e-10"] = {"ms": ms, "statuses": [sicp.GRAPH_COV_STATUSES[int(k)] for k in st], "info": info}
        out["solves"][str(n)] = row
        print(json.dumps(row, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
