"""Stage times of the initial alignment without a pose prior (sicp_bootstrap, exec/bootstrap.h defaults) on 100K x 100K
pairs: keypoints, features, matching, scoring, total; the keypoint counts and the largest neighbourhood.  Evidence for
DESIGN.md, not a gate.  usage (GPU box): bootstrap_timing.py [repeats]"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth
sicp = importlib.import_module("semantic-icp_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
for seed, motion in ((2, (1.0, 2.0)), (3, (4.0, 120.0))):
    src, _, tgt, _, T, _ = synth.lidar_pair(seed=seed, n_points=100000, motion=motion)
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e:
        e.set_source(src); e.set_target(tgt)
        e.bootstrap()  # warm-up: arena blocks, code objects
        infos = [e.bootstrap()[1] for _ in range(reps)]
    keys = ("t_keypoints_ms", "t_features_ms", "t_match_ms", "t_score_ms", "t_total_ms")
    med = {k: round(float(np.median([i[k] for i in infos])), 3) for k in keys}
    last = infos[-1]
    print(json.dumps(dict(seed=seed, motion=motion, n_points=100000, repeats=reps, median_ms=med,
                          n_source_keypoints=last["n_source_keypoints"], n_target_keypoints=last["n_target_keypoints"],
                          max_neighbours=last["max_neighbours"], best_iteration=last["best_iteration"])), flush=True)
