"""Stage times of the label-aware initial alignment (sicp_bootstrap_semantic) beside the label-blind one (sicp_bootstrap)
on the 100K x 100K pairs of tools/bootstrap_timing.py, with the pairs' own labels: keypoints, features, matching, scoring,
total, and the share of matching + features (what a per-label grouping of the target keypoints could shorten).  Evidence
for DESIGN.md 3.3, not a gate.  usage (GPU box): bootstrap_semantic_timing.py [repeats] [out.json]"""
import importlib, json, os, sys
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth
sicp = importlib.import_module("semantic-icp_amd")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else None
keys = ("t_keypoints_ms", "t_features_ms", "t_match_ms", "t_score_ms", "t_total_ms")


def median_of(infos):
    return {k: round(float(np.median([i[k] for i in infos])), 3) for k in keys}


rows = []
for seed, motion in ((2, (1.0, 2.0)), (3, (4.0, 120.0))):
    src, sl, tgt, tl, T, _ = synth.lidar_pair(seed=seed, n_points=100000, motion=motion)
    moving = int(np.bincount(sl).argmax())  # the most frequent label stands in for a moving class
    calls = {"bootstrap": lambda e: e.bootstrap(),
             "semantic": lambda e: e.bootstrap_semantic(),
             "semantic_flags_off": lambda e: e.bootstrap_semantic(None, sicp.default_bootstrap_label_params(match_same_label=0, score_same_label=0)),
             "semantic_ignore_1": lambda e: e.bootstrap_semantic(None, sicp.default_bootstrap_label_params(ignore=(moving,)))}
    with sicp.Engine(0, sicp.default_params(sicp.MODE_GICP)) as e:
        e.set_source(src, sl); e.set_target(tgt, tl)
        for name, call in calls.items():
            call(e)  # warm-up: arena blocks, code objects
            infos = [call(e)[1] for _ in range(reps)]
            med, last = median_of(infos), infos[-1]
            row = dict(call=name, seed=seed, motion=motion, n_points=100000, repeats=reps, median_ms=med,
                       match_and_features_share=round((med["t_match_ms"] + med["t_features_ms"]) / med["t_total_ms"], 3),
                       n_source_keypoints=last["n_source_keypoints"], n_target_keypoints=last["n_target_keypoints"],
                       max_neighbours=last["max_neighbours"], best_iteration=last["best_iteration"])
            rows.append(row)
            print(json.dumps(row), flush=True)
if out_path:
    with open(out_path, "w") as f:
        json.dump(rows, f, indent=1)
