#!/usr/bin/env python3
"""One timing of the pose graph with priors and disabled edges -> a JSON file (profiles/graph_priors/timing.json keeps the run
of 2026-10-20 under "with_priors_and_disabled_edges").

The graph of tools/pose_graph_timing.py at 10^5 nodes / 3 x 10^5 edges, node 0 fixed, and on top of it a position prior (the true
position, 5 cm) on every 10th node and 1 % of the closures switched off.  The same measurements as that tool, with its clock:
one outer iteration whose linear solve is held to exactly 64 and to 256 conjugate-gradient steps (the difference over 192 is the
time per CG iteration), and the whole optimisation with 2000 CG steps allowed per solve.  Beside them the plain graph -- no
priors, every edge enabled -- in the same process."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pose_graph_cases as cases  # noqa: E402
import pose_graph_timing as base  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")


def timed(g, params, reps, priors=None, e_on=None, warmup=1):
    import time

    with sicp.PoseGraph(0, params) as pg:
        pg.add_nodes(g["poses"], g["fixed"])
        pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
        if priors is not None:
            pg.add_priors(*priors, kind=sicp.PRIOR_POSITION)
        if e_on is not None:
            pg.set_edges_enabled(e_on)
        ms, info = [], None
        for k in range(warmup + reps):
            pg.set_poses(g["poses"])
            t = time.perf_counter()
            info = pg.optimize()
            if k >= warmup:
                ms.append((time.perf_counter() - t) * 1e3)
        counts = pg.counts()
    return base.spread(ms), info, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--total-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_priors", "priors_timing.json"))
    a = ap.parse_args()
    n = a.nodes
    g = base.graph(n)
    m = len(g["ei"])
    truth = cases._circle(n, radius=n / 6.0)
    nodes = np.arange(0, n, 10, dtype=np.int32)
    priors = (nodes, truth[nodes, 4:], np.tile(np.eye(3) / 0.05 ** 2, (len(nodes), 1, 1)))
    rng = np.random.default_rng(5)
    e_on = np.ones(m, dtype=bool)
    e_on[n + rng.choice(m - n, size=(m - n) // 100, replace=False)] = False
    with sicp.PoseGraph(0) as pg:
        pg.add_nodes(g["poses"], g["fixed"])
        pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
        g0 = float(np.abs(pg.linearize()["gradient"]).max())
    out = {"nodes": n, "edges": m, "clock": "time.perf_counter() around synchronous calls, after a warm-up run of the same shape; whole calls, in ms",
           "position_priors": int(len(nodes)), "edges_disabled": int((~e_on).sum()), "gradient_tolerance": 1e-6 * g0, "reps": a.reps}
    for name, kw in (("plain", {}), ("priors_and_disabled_edges", dict(priors=priors, e_on=e_on))):
        row, held = {}, {}
        for k in (64, 256):
            p = sicp.default_graph_params(max_iterations=1, max_cg_iterations=k, cg_eta=1e-300, gradient_tolerance=0.0)
            held[k], info, counts = timed(g, p, a.reps, **kw)
            assert info["cg_iterations"] == k, info
        row["counts"] = counts
        row["one_outer_iteration_with_64_cg_steps_ms"], row["one_outer_iteration_with_256_cg_steps_ms"] = held[64], held[256]
        cg_ms = (held[256]["median"] - held[64]["median"]) / 192.0
        row["ms_per_cg_iteration"] = round(cg_ms, 5)
        row["outer_iteration_without_cg_ms"] = round(held[64]["median"] - 64 * cg_ms, 3)
        p = sicp.default_graph_params(gradient_tolerance=1e-6 * g0, max_iterations=100, max_cg_iterations=2000)
        total, info, _ = timed(g, p, a.total_reps, **kw)
        row["optimize_max_cg_2000"] = {"ms": total, "info": info, "ms_per_outer_iteration": round(total["median"] / max(info["iterations"], 1), 3)}
        out[name] = row
        print(name, json.dumps(row, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
