#!/usr/bin/env python3
"""What SICP_SUBMIT_POSE_COVARIANCE costs an open stream: the align-only open-stream leg of bench.py (consecutive scans, EM-ICP,
resident clouds, 256 in flight, ticks of 4 LM evaluations) with no registration flagged and with every registration flagged,
per build.  The scans are generated once; every build runs in a child process of its own (forked before any HIP call).
usage (GPU box): stream_pose_cov_cost.py [--pairs 1024] [--points 100000] [--reps 3] --build LABEL=TREE[:flagged] ... [--out FILE]
  TREE: a built checkout ("" = this one); ":flagged" also measures that build with every registration flagged"""
import argparse, importlib, json, multiprocessing as mp, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=1024)
ap.add_argument("--points", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--build", action="append", default=[])
ap.add_argument("--out", default=None)
args = ap.parse_args()


def gen(k):
    return synth.lidar_sequence_scan(7, k, n_points=args.points, period=128)[:2]


def measure(tree, flagged, conn):
    sys.path.insert(0, os.path.abspath(tree) if tree else ROOT)
    sicp = importlib.import_module("semantic-icp_amd")
    cm = synth.confusion_matrix(11)
    p = sicp.default_params(sicp.MODE_EM); p.num_classes = 11; p.lm_batch = 4
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    out = {}
    for flag in ([False, True] if flagged else [False]):
        kw = dict(pose_covariance=True) if flag else {}
        rates = []
        for rep in range(args.reps + 1):  # (the first run warms pools, graphs and allocations up)
            with sicp.Stream(0, p, max_in_flight=256, confusion=cm) as S:
                ids = [S.add_cloud(*sc) for sc in scans]
                S.submit(ids[-1], ids[0], ident)
                S.drain()
                res = []
                t0 = time.perf_counter()
                for k in range(args.pairs):
                    S.submit(ids[k + 1], ids[k], ident, **kw)
                    if k % 64 == 0:
                        res += S.poll(wait=0)
                res += S.drain()
                dt = time.perf_counter() - t0
                assert len(res) == args.pairs and all(st == 0 for _, st, _, _ in res)
                if flag:
                    t1 = time.perf_counter()
                    for t, _, _, _ in res:
                        S.take_pose_covariance(t, 0.01, 0.01)
                    out["take_us_per_registration"] = round((time.perf_counter() - t1) * 1e6 / args.pairs, 2)
            if rep:
                rates.append(args.pairs / dt)
        key = "flagged" if flag else "unflagged"
        out[key + "_pairs_per_s"] = [round(r, 1) for r in rates]
        out[key + "_ms_per_pair_median"] = round(1e3 / float(np.median(rates)), 4)
    conn.send(out)
    conn.close()


with mp.get_context("fork").Pool(min(64, os.cpu_count() or 8)) as pool:
    scans = pool.map(gen, range(args.pairs + 1))
result = dict(pairs=args.pairs, points=args.points, in_flight=256, lm_batch=4, repeats=args.reps, builds={})
for spec in args.build:
    label, _, lib = spec.partition("=")
    flagged = lib.endswith(":flagged")
    lib = lib[:-len(":flagged")] if flagged else lib  # (the checkout)
    a, b = mp.get_context("fork").Pipe()
    child = mp.get_context("fork").Process(target=measure, args=(lib, flagged, b))
    child.start()
    b.close()
    try:
        result["builds"][label] = a.recv()
    except EOFError:
        result["builds"][label] = "failed"
    child.join()
    print(label, json.dumps(result["builds"][label]), flush=True)
for label, r in result["builds"].items():
    if isinstance(r, dict) and "flagged_ms_per_pair_median" in r:
        r["ms_per_flagged_registration_extra"] = round(r["flagged_ms_per_pair_median"] - r["unflagged_ms_per_pair_median"], 4)
print(json.dumps(result), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    json.dump(result, open(args.out, "w"), indent=1)
