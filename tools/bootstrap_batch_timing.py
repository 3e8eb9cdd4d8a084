"""Pairs per second of sicp_bootstrap_batch against sequential sicp_bootstrap calls on 100K x 100K pairs, and the batch's
stage split (keypoints, features, matching = feature k-NN + host draws, scoring).  Evidence for DESIGN.md, not a gate.
usage (GPU box): bootstrap_batch_timing.py [repeats]"""
import importlib, json, os, sys, time
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth
sicp = importlib.import_module("semantic-icp_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
# 8 distinct 100K x 100K pairs, reused round-robin by the handles of a batch
pairs = [synth.lidar_pair(seed=20 + i, n_points=100000, motion=(1.0 + 0.5 * i, 10.0 * i))[:4:2] for i in range(8)]
engines = []
for i in range(64):
    e = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    e.set_source(pairs[i % 8][0]); e.set_target(pairs[i % 8][1])
    engines.append(e)
keys = ("t_keypoints_ms", "t_features_ms", "t_match_ms", "t_score_ms", "t_total_ms")
sicp.bootstrap_batch(engines[:8])  # warm-up: arena blocks, code objects
for e in engines[:8]:
    e.bootstrap()
# 32 sequential lone calls
seq = []
for _ in range(reps):
    t0 = time.perf_counter()
    for e in engines[:32]:
        e.bootstrap()
    seq.append(time.perf_counter() - t0)
print(json.dumps(dict(mode="sequential", n=32, repeats=reps, pairs_per_s=round(32 / float(np.median(seq)), 2),
                      median_s=round(float(np.median(seq)), 4))), flush=True)
for n in (1, 8, 32, 64):
    wall, split = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        res = sicp.bootstrap_batch(engines[:n])
        wall.append(time.perf_counter() - t0)
        assert all(r[0] == sicp.OK for r in res)
        split.append([res[0][2][k] for k in keys])
    med = np.median(np.array(split), axis=0)
    print(json.dumps(dict(mode="batch", n=n, repeats=reps, pairs_per_s=round(n / float(np.median(wall)), 2),
                          median_s=round(float(np.median(wall)), 4), stage_ms={k: round(float(v), 3) for k, v in zip(keys, med)})),
          flush=True)
for e in engines:
    e.close()
