#!/usr/bin/env python3
"""Times of the pose graph on the GPU -> profiles/pose_graph/timing.json.

Graphs: a ring with closures at 10^4 nodes / 3 x 10^4 edges and at 10^5 nodes / 3 x 10^5 edges -- n odometry edges round a
circle (the last one closes it) and 2n closures between nodes 2 .. 50 steps apart, 2 cm / 1 degree of noise per edge, the
initial poses 5 cm / 0.05 rad off the truth, node 0 fixed.  Per graph: the whole optimisation until max |g| has fallen by 1e-6
(or 100 outer iterations), with 500 and with 2000 CG steps allowed per solve; the time per outer iteration (whole time /
iterations); and the time per conjugate-gradient iteration (one outer iteration with the linear
solve held to exactly 64 and to 256 steps: the difference over 192).  Beside them, on the same machine's CPU, the reference
minimiser's parts with scipy (tests/pose_graph_ref.py): one assembly and one sparse direct solve of the damped system -- one outer
iteration of the reference -- and, on request, the whole minimisation (minutes).

Clock: time.perf_counter() around calls that are synchronous (each ends in a stream synchronise inside the library), after
warm-up runs of the same shape; the median, minimum and maximum of `--reps` runs.  The poses are set back before every run.  No
kernel trace is taken here."""
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

import pose_graph_cases as cases  # noqa: E402
import pose_graph_ref as R  # noqa: E402

sicp = importlib.import_module("semantic-icp_amd")


def graph(n, seed=1):
    rng = np.random.default_rng(seed)
    truth = cases._circle(n, radius=n / 6.0)  # about 1 m between neighbours
    a = rng.integers(0, n, size=2 * n)
    ei = np.concatenate([np.arange(n), a]).astype(np.int32)
    ej = np.concatenate([(np.arange(n) + 1) % n, (a + rng.integers(2, 51, size=2 * n)) % n]).astype(np.int32)
    z = cases._measure(rng, truth, ei, ej)
    poses = R.mul(truth, R.exp(rng.normal(size=(n, 6)) * 0.05))
    poses[0] = truth[0]
    fixed = np.zeros(n, dtype=bool)
    fixed[0] = True
    return dict(poses=poses, fixed=fixed, ei=ei, ej=ej, z=z, omega=cases.default_omega(len(ei)))


def spread(ms):
    return {"n": len(ms), "median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def timed_optimize(g, params, reps, warmup=1):
    with sicp.PoseGraph(0, params) as pg:
        pg.add_nodes(g["poses"], g["fixed"])
        pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
        ms, info = [], None
        for k in range(warmup + reps):
            pg.set_poses(g["poses"])
            t = time.perf_counter()
            info = pg.optimize()
            if k >= warmup:
                ms.append((time.perf_counter() - t) * 1e3)
    return spread(ms), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--total-reps", type=int, default=3, help="runs of the whole optimisation")
    ap.add_argument("--sizes", type=int, nargs="*", default=[10_000, 100_000])
    ap.add_argument("--scipy-whole-below", type=int, default=0, help="run the whole reference minimisation below this many nodes (minutes at 10^4)")
    ap.add_argument("--no-scipy", action="store_true", help="leave the CPU reference out (for a run under a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph", "timing.json"))
    a = ap.parse_args()
    out = {"reps": a.reps,
           "clock": "time.perf_counter() around synchronous calls, after a warm-up run of the same shape; whole calls, in ms",
           "not_measured": ["kernel times (no kernel trace was taken)", "more than one device", "graphs other than the ring with closures"],
           "graphs": {}}
    for n in a.sizes:
        g = graph(n)
        m = len(g["ei"])
        row = {"nodes": n, "edges": m, "off_diagonal_block_bytes": 288 * m}
        with sicp.PoseGraph(0) as pg:
            pg.add_nodes(g["poses"], g["fixed"])
            pg.add_edges(g["ei"], g["ej"], g["z"], g["omega"])
            g0 = float(np.abs(pg.linearize()["gradient"]).max())
        # "convergence": max |g| down by 1e-6 from the start.  The default 500 CG steps a solve do not reach cg_eta on a chain
        # this long (block-Jacobi leaves the chain's conditioning as it is), so the run is timed with 2000 as well.
        row["initial_gradient_max_norm"] = g0
        row["gradient_tolerance"] = 1e-6 * g0
        for cap in (500, 2000):
            p = sicp.default_graph_params(gradient_tolerance=1e-6 * g0, max_iterations=100, max_cg_iterations=cap)
            total, info = timed_optimize(g, p, a.total_reps)
            row[f"optimize_max_cg_{cap}"] = {"ms": total, "info": info, "ms_per_outer_iteration": round(total["median"] / max(info["iterations"], 1), 3),
                                              "cg_iterations_per_outer_iteration": round(info["cg_iterations"] / max(info["iterations"], 1), 1)}
        held = {}
        for k in (64, 256):  # one outer iteration whose linear solve takes exactly k steps
            p = sicp.default_graph_params(max_iterations=1, max_cg_iterations=k, cg_eta=1e-300, gradient_tolerance=0.0)
            held[k], hinfo = timed_optimize(g, p, a.reps)
            assert hinfo["cg_iterations"] == k, hinfo
        row["one_outer_iteration_with_64_cg_steps_ms"] = held[64]
        row["one_outer_iteration_with_256_cg_steps_ms"] = held[256]
        cg_ms = (held[256]["median"] - held[64]["median"]) / 192.0
        row["ms_per_cg_iteration"] = round(cg_ms, 5)
        row["five_launches_per_cg_iteration_us_per_launch"] = round(cg_ms * 1e3 / 5.0, 2)
        # what one CG iteration must move: B from both sides, the diagonal blocks, the factors, and the five vectors a few times
        moved = 2 * 288 * m + n * 8 * (36 + 27) + n * 48 * 12
        row["bytes_per_cg_iteration_estimate"] = moved
        row["effective_GB_per_s_of_a_cg_iteration"] = round(moved / (cg_ms * 1e-3) / 1e9, 1) if cg_ms > 0 else None
        row["outer_iteration_without_cg_ms"] = round(held[64]["median"] - 64 * cg_ms, 3)
        if a.no_scipy:
            out["graphs"][str(n)] = row
            print(json.dumps(row, indent=1), flush=True)
            continue
        # the reference's parts on this machine's CPU
        t = time.perf_counter()
        c, grad, H = R.assemble(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"])
        t_asm = (time.perf_counter() - t) * 1e3
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
        D = np.clip(H.diagonal(), 1e-6, 1e32) / 1e4
        t = time.perf_counter()
        spla.spsolve((H + sp.diags(D)).tocsc(), -grad)
        t_solve = (time.perf_counter() - t) * 1e3
        row["scipy_cpu"] = {"assemble_ms": round(t_asm, 1), "spsolve_ms": round(t_solve, 1), "cpus": os.cpu_count()}
        if n < a.scipy_whole_below:
            t = time.perf_counter()
            _, rinfo = R.minimise(g["poses"], g["fixed"], g["ei"], g["ej"], g["z"], g["omega"], rel_gradient=1e-9)
            row["scipy_cpu"]["minimise_ms"] = round((time.perf_counter() - t) * 1e3, 1)
            row["scipy_cpu"]["minimise_info"] = {k: v for k, v in rinfo.items() if k not in ("g", "H")}
        out["graphs"][str(n)] = row
        print(json.dumps(row, indent=1), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
