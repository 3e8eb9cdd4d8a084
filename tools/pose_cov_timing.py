"""Cost of sicp_pose_covariance on 100K x 100K EM pairs (K = 4) next to the align() it would follow: wall time per lone
call, per pair of a batch call, and per align(), medians over repeats.  Evidence for DESIGN.md, not a gate.
usage (GPU box): pose_cov_timing.py [pairs] [repeats]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth
sicp = importlib.import_module("semantic-icp_amd")
pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
es, qts = [], []
for k in range(pairs):
    src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=100 + k, n_points=100_000)
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = cm.shape[0]
    e = sicp.Engine(0, p)
    e.set_confusion(cm); e.set_source(src, sl); e.set_target(tgt, tl)
    qt, _ = e.align()
    es.append(e); qts.append(qt)
qts = np.stack(qts)
for e, q in zip(es, qts):  # warm-up: arena blocks, code objects
    e.pose_covariance(q)
lone, batch, align = [], [], []
for _ in range(reps):
    t0 = time.perf_counter()
    for e, q in zip(es, qts):
        e.pose_covariance(q)
    lone.append((time.perf_counter() - t0) * 1e3 / pairs)
    t0 = time.perf_counter()
    sicp.pose_covariance_batch(es, qts)
    batch.append((time.perf_counter() - t0) * 1e3 / pairs)
    t0 = time.perf_counter()
    for e in es:
        e.align(want_stats=False)
    align.append((time.perf_counter() - t0) * 1e3 / pairs)
r = es[0].pose_covariance(qts[0], 0.01, 0.01)
print(json.dumps(dict(pairs=pairs, repeats=reps, n_points=100_000, mode="EM", K=4, active_slots=r["active"],
                      ms_per_pair_lone=round(float(np.median(lone)), 3), ms_per_pair_batch=round(float(np.median(batch)), 3),
                      ms_per_align=round(float(np.median(align)), 3),
                      sigma_1cm_std_mm_mrad=[round(float(np.sqrt(v)) * 1e3, 4) for v in np.diag(r["covariance"])])), flush=True)
for e in es:
    e.close()
