#!/usr/bin/env python3
"""What sicp_evaluate costs at 100K x 100K points (LiDAR-like pairs, 11 labels, max_dist_sq = 25, a confusion table asked for).
Evidence for DESIGN.md 3.7, not a gate.  Three measurements, each a child process under a time limit of its own; the driver
stops at the first one that fails and writes what it has:
  wall    Engine.evaluate against the host route it replaces -- Engine.correspondences of a knn = 1 handle (the read-back of
          n x K slots in caller order) plus a numpy reduction of them -- alternating in one loop, wall clock per call; and the
          HIP-event time of the K = 1 search alone (sicp_search_batch)
  batch   64 pairs through one evaluate_batch call against 64 lone calls, alternating, wall clock per pair
  trace   the kernels of lone calls under `rocprofv3 --kernel-trace`: the evaluation kernel and the finalise step next to the
          K = 1 search of the same call (the profiler's kernel durations: the call has no event hook of its own)
Every figure comes with its spread over the repeats: median, min, max, 10th and 90th percentile.
usage (GPU box): tools/evaluate_timing.py [--out FILE] [--reps N] [--pairs N]      (the driver)
                 tools/evaluate_timing.py --step wall|batch|traced ...              (one measurement, prints one JSON line)"""
import argparse, csv, glob, importlib, json, os, shutil, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, GATE, CLASSES = 100_000, 25.0, 11


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(n=int(v.size), median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4))


def pair(k):
    import np_ref, synth
    src, sl, tgt, tl, T, _ = synth.lidar_pair(seed=100 + k, n_points=N)
    return src, sl, tgt, tl, np_ref.mat_to_qt(T)


def engine(sicp, mode, data, **kw):
    src, sl, tgt, tl, _ = data
    p = sicp.default_params(mode)
    p.num_classes = CLASSES
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    e.set_source(src, sl)
    e.set_target(tgt, tl)
    return e


def host_route(e, qt, sl, tl):
    """what a caller did before: read the K = 1 correspondences back and reduce them"""
    idx, d2, _ = e.correspondences(qt)
    idx, d2 = idx[:, 0], d2[:, 0]
    inl = idx >= 0
    ls, lt = sl[inl].astype(np.int64) - 1, tl[idx[inl]].astype(np.int64) - 1
    conf = np.bincount(ls * CLASSES + lt, minlength=CLASSES * CLASSES).reshape(CLASSES, CLASSES)
    s = float(d2[inl].astype(np.float64).sum())
    n = int(inl.sum())
    return dict(inliers=n, label_agree=int((ls == lt).sum()), sum_d2=s, fitness=n / len(idx), inlier_rmse=(s / n) ** 0.5 if n else float("nan"),
                confusion=conf)


def step_wall(args):
    sicp = importlib.import_module("semantic-icp_amd")
    data = pair(0)
    qt = data[4]
    ev = engine(sicp, sicp.MODE_GICP, data)
    host = engine(sicp, sicp.MODE_GICP, data, knn=1, gate_sq=GATE)
    a, b = ev.evaluate(qt, GATE, num_classes=CLASSES), host_route(host, qt, data[1], data[3])
    assert a["inliers"] == b["inliers"] and np.array_equal(a["confusion"], b["confusion"]), "the two routes disagree"
    for _ in range(3):  # warm-up: arena blocks, code objects, the host route's features
        ev.evaluate(qt, GATE, num_classes=CLASSES)
        host_route(host, qt, data[1], data[3])
    t_ev, t_plain, t_host = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); ev.evaluate(qt, GATE, num_classes=CLASSES); t_ev.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); ev.evaluate(qt, GATE); t_plain.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); host_route(host, qt, data[1], data[3]); t_host.append((time.perf_counter() - t0) * 1e3)
    search = [sicp.search_batch([host], qt[None, :], what=0, use_hint=False, repeat=20) for _ in range(args.reps)]
    res = dict(n_points=N, inliers=a["inliers"], evaluate_ms=spread(t_ev), evaluate_no_table_ms=spread(t_plain), host_route_ms=spread(t_host),
               search_k1_event_us=spread([1e3 * (s[-1] if isinstance(s, tuple) else s) for s in search]))
    ev.close(); host.close()
    return res


def step_batch(args):
    sicp = importlib.import_module("semantic-icp_amd")
    data = [pair(k) for k in range(8)]  # eight distinct pairs, each on pairs / 8 handles of its own
    es = [engine(sicp, sicp.MODE_GICP, data[k % 8]) for k in range(args.pairs)]
    qts = np.stack([data[k % 8][4] for k in range(args.pairs)])
    for _ in range(2):
        lone = [e.evaluate(q, GATE, num_classes=CLASSES) for e, q in zip(es, qts)]
        both = sicp.evaluate_batch(es, qts, GATE, num_classes=CLASSES)
    assert all(s == sicp.OK and r["sum_d2"] == l["sum_d2"] and np.array_equal(r["confusion"], l["confusion"]) for (s, r), l in zip(both, lone))
    t_lone, t_batch = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        for e, q in zip(es, qts):
            e.evaluate(q, GATE, num_classes=CLASSES)
        t_lone.append((time.perf_counter() - t0) * 1e3 / args.pairs)
        t0 = time.perf_counter()
        sicp.evaluate_batch(es, qts, GATE, num_classes=CLASSES)
        t_batch.append((time.perf_counter() - t0) * 1e3 / args.pairs)
    for e in es:
        e.close()
    return dict(pairs=args.pairs, n_points=N, lone_ms_per_pair=spread(t_lone), batch_ms_per_pair=spread(t_batch))


def step_traced(args):
    """the program rocprofv3 traces: set-up, then `reps` lone calls (their kernels are the last `reps` of each name)"""
    sicp = importlib.import_module("semantic-icp_amd")
    data = pair(0)
    ev = engine(sicp, sicp.MODE_GICP, data)
    for _ in range(3 + args.reps):
        ev.evaluate(data[4], GATE, num_classes=CLASSES)
    ev.close()
    return dict(calls=3 + args.reps)


def kernel_spreads(trace_dir, reps):
    f = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda x: int(x["Start_Timestamp"]))
    out = {}
    for key, frag in (("evaluate_jobs_us", "evaluate_jobs_kernel"), ("evaluate_finalize_us", "evaluate_finalize_jobs_kernel"),
                      ("search_k1_us", "bvh_knn_packet")):
        us = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in rows if frag in x["Kernel_Name"]]
        if us:
            out[key] = spread(us[-reps:])
    return out


def child(seconds, cmd):
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1, None
    return 0, json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["wall", "batch", "traced"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaluate", "timing.json"))
    ap.add_argument("--trace-dir", default=os.path.join(tempfile.gettempdir(), "sicp_evaluate_trace"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps({"wall": step_wall, "batch": step_batch, "traced": step_traced}[args.step](args)), flush=True)
        return 0
    me = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--pairs", str(args.pairs)]
    res, rc = {}, 0
    for name, seconds, cmd in (
            ("wall", 240, me + ["--step", "wall"]),
            ("batch", 300, me + ["--step", "batch"]),
            ("trace", 240, ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", args.trace_dir, "--"] + me + ["--step", "traced"])):
        if name == "trace":
            shutil.rmtree(args.trace_dir, ignore_errors=True)
        rc, got = child(seconds, cmd)
        print(f"[evaluate_timing] {name}: {'ok' if rc == 0 else 'failed (%d)' % rc}", file=sys.stderr, flush=True)
        if rc != 0:  # nothing more is started on the GPU after a step that failed
            res[name] = {"failed": rc}
            break
        res[name] = kernel_spreads(args.trace_dir, args.reps) if name == "trace" else got
    shutil.rmtree(args.trace_dir, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return rc


if __name__ == "__main__":
    sys.exit(main())
