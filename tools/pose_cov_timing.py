"""Cost of sicp_pose_covariance on 100K x 100K EM pairs (K = 4) next to the align() it would follow: wall time per lone
call, per pair of a batch call, and per align(), medians over repeats.  Evidence for DESIGN.md, not a gate.
usage (GPU box): pose_cov_timing.py [pairs] [repeats] [--wide N] [--tree DIR] [--out FILE --label NAME]
--tree DIR: measure the built checkout DIR instead of this one (another commit on the same box)
--wide N: also a batch call of N handles (the pairs' clouds again on handles of their own), per pair
--out FILE: the result is also stored in FILE (a JSON object, one entry per --label: runs of several builds side by side)"""
import argparse, importlib, json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth
ap = argparse.ArgumentParser()
ap.add_argument("pairs", type=int, nargs="?", default=8)
ap.add_argument("reps", type=int, nargs="?", default=5)
ap.add_argument("--wide", type=int, default=0)
ap.add_argument("--tree", default=ROOT)
ap.add_argument("--out", default=None)
ap.add_argument("--label", default="run")
args = ap.parse_args()
pairs, reps = args.pairs, args.reps
data = [synth.lidar_pair(seed=100 + k, n_points=100_000) for k in range(pairs)]
sys.path.insert(0, os.path.abspath(args.tree))
sicp = importlib.import_module("semantic-icp_amd")


def engine(k):
    src, sl, tgt, tl, T, cm = data[k % pairs]
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = cm.shape[0]
    e = sicp.Engine(0, p)
    e.set_confusion(cm); e.set_source(src, sl); e.set_target(tgt, tl)
    return e


es, qts = [], []
for k in range(max(pairs, args.wide)):
    e = engine(k)
    qt, _ = e.align()
    es.append(e); qts.append(qt)
qts = np.stack(qts)
for e, q in zip(es, qts):  # warm-up: arena blocks, code objects
    e.pose_covariance(q)
sicp.pose_covariance_batch(es[:pairs], qts[:pairs])
if args.wide:
    sicp.pose_covariance_batch(es[:args.wide], qts[:args.wide])
lone, batch, wide, align = [], [], [], []
for _ in range(reps):
    t0 = time.perf_counter()
    for e, q in zip(es[:pairs], qts[:pairs]):
        e.pose_covariance(q)
    lone.append((time.perf_counter() - t0) * 1e3 / pairs)
    t0 = time.perf_counter()
    sicp.pose_covariance_batch(es[:pairs], qts[:pairs])
    batch.append((time.perf_counter() - t0) * 1e3 / pairs)
    if args.wide:
        t0 = time.perf_counter()
        sicp.pose_covariance_batch(es[:args.wide], qts[:args.wide])
        wide.append((time.perf_counter() - t0) * 1e3 / args.wide)
    t0 = time.perf_counter()
    for e in es[:pairs]:
        e.align(want_stats=False)
    align.append((time.perf_counter() - t0) * 1e3 / pairs)
r = es[0].pose_covariance(qts[0], 0.01, 0.01)
res = dict(pairs=pairs, repeats=reps, n_points=100_000, mode="EM", K=4, active_slots=r["active"],
           ms_per_pair_lone=round(float(np.median(lone)), 3), ms_per_pair_batch=round(float(np.median(batch)), 3),
           ms_per_align=round(float(np.median(align)), 3),
           sigma_1cm_std_mm_mrad=[round(float(np.sqrt(v)) * 1e3, 4) for v in np.diag(r["covariance"])])
if args.wide:
    res["wide_batch_pairs"] = args.wide
    res["ms_per_pair_wide_batch"] = round(float(np.median(wide)), 3)
print(json.dumps(res), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    prev = json.load(open(args.out)) if os.path.exists(args.out) else {}
    prev[args.label] = res
    json.dump(prev, open(args.out, "w"), indent=1)
for e in es:
    e.close()
