#!/usr/bin/env python3
"""What an upload costs -- sicp_set_cloud: staging, the copies and the tree build of csrc/build_tree.hip -- and whether two
builds of the library lay a cloud out the same way (evidence for an A/B of the build, not a gate).  Three clouds:
  flat       EM, synth.lidar_pair(seed=2, n_points=100000): one segment, no caller-index array
  semantic   SICP_MODE_SEMANTIC, synth.rgbd_pair(seed=3): 13 label segments in 307 200 points
  one_label  SICP_MODE_SEMANTIC, the flat cloud's points all given label 1: one segment WITH a caller-index array
Per cloud: REPEATS uploads of the source through one handle, host wall clock of the set_source call and of the wait until
synchronize() returns (the upload and the build are queued, not waited for); median and range over the repeats after the
first.  Then a SHA-256 over the bytes of correspondences(POSE) (idx, d2) and accumulate(POSE) (out28): no API reads a tree
back, but every sum is taken in the device order that the build lays down.  SICP_LIB selects another build of the library, as
for every tool.
usage (GPU box): tools/upload_timing.py [--out FILE]     (the driver)
                 tools/upload_timing.py --step run       (the measurement, prints one JSON line)"""
import argparse, hashlib, importlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, REPEATS = 100_000, 21


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(n=int(v.size), median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def step_run(args):
    import synth
    from np_ref import mat_to_qt

    sicp = importlib.import_module("semantic-icp_amd")
    pose = mat_to_qt(synth.pose_matrix(2.0, (0.1, 0.2, 1.0), (0.5, -0.1, 0.05)))
    fs, fsl, ft, ftl, _, cm = synth.lidar_pair(seed=2, n_points=N)
    rs, rsl, rt, rtl = synth.rgbd_pair(seed=3)[:4]
    one = lambda a: np.ones(len(a), dtype=np.uint32)
    clouds = (("flat", sicp.MODE_EM, fs, fsl, ft, ftl), ("semantic", sicp.MODE_SEMANTIC, rs, rsl, rt, rtl),
              ("one_label", sicp.MODE_SEMANTIC, fs, one(fs), ft, one(ft)))
    res = dict(lib=os.environ.get("SICP_LIB", "product"), repeats=REPEATS)
    for name, mode, src, sl, tgt, tl in clouds:
        p = sicp.default_params(mode)
        if mode == sicp.MODE_EM:
            p.num_classes = cm.shape[0]
        with sicp.Engine(0, p) as e:
            if mode == sicp.MODE_EM:
                e.set_confusion(cm)
            e.set_target(tgt, tl)
            call, wait = [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                e.set_source(src, sl)
                t1 = time.perf_counter()
                e.synchronize()
                t2 = time.perf_counter()
                call.append((t1 - t0) * 1e3)
                wait.append((t2 - t1) * 1e3)
            idx, d2, _ = e.correspondences(pose)
            out28 = e.accumulate(pose)
        sha = hashlib.sha256(idx.tobytes() + d2.tobytes() + out28.tobytes()).hexdigest()
        res[name] = dict(points=len(src), segments=int(len(np.unique(sl))) if mode == sicp.MODE_SEMANTIC else 1, matched=int((idx >= 0).sum()),
                         set_source_call_ms=spread(call[1:]), wait_ms=spread(wait[1:]), sha256=sha)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_run(args)), flush=True)
        return 0
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", "run"], capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1
    res = json.loads(lines[-1])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"))
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
