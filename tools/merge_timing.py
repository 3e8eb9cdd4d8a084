#!/usr/bin/env python3
"""What sicp_merge_clouds costs at the size of a local map (evidence for DESIGN.md 3.8, not a gate).  Two shapes, measured
alternately in one loop of one child process under a time limit:
  map    8 parts x 100K LiDAR-like labelled points at poses along a track, leaf 0.2, crop 40 about the last pose
  crop   1 part of 100K points, identity, leaf 0, crop 40: the reference drivers' filterRange on the device
For each: the wall clock of merge_clouds with and without the result's read-back (host clock around a call that ends in a
stream synchronise), the HIP-event time of every stage (the library prints them to stderr when SICP_DEBUG and SICP_MERGE_LOG
are set: events on the call's own stream between its launches), and for context, in the same loop, the wall clock of
Engine.set_cloud on the same number of raw points -- what the host route (transform, crop, voxel grid and label vote in a
host loop, then an upload) pays for the upload alone.  Every figure comes with its spread over the repeats: median, min, max,
10th and 90th percentile.
usage (GPU box): tools/merge_timing.py [--out FILE] [--reps N]      (the driver)
                 tools/merge_timing.py --step run ...               (the measurement, prints one JSON line)"""
import argparse, importlib, json, os, re, subprocess, sys, tempfile, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, PARTS, LEAF, RANGE = 100_000, 8, 0.2, 40.0


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(n=int(v.size), median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4),
                p10=round(float(np.percentile(v, 10)), 4), p90=round(float(np.percentile(v, 90)), 4))


class StageLog:
    """file descriptor 2 into a file while the timed calls run; the library's `sicp_merge: ... name_ms=value` lines out of it"""

    def __init__(self):
        self.f = tempfile.TemporaryFile(mode="w+b")
        self.saved = None

    def __enter__(self):
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)

    def stages(self):
        self.f.seek(0)
        rows = []
        for line in self.f.read().decode(errors="replace").splitlines():
            if line.startswith("sicp_merge:"):
                rows.append({k: float(v) for k, v in re.findall(r"(\w+)=([0-9.eE+-]+)", line)})
        return rows


def step_run(args):
    os.environ["SICP_DEBUG"] = "1"
    os.environ["SICP_MERGE_LOG"] = "1"
    import np_ref, synth
    sicp = importlib.import_module("semantic-icp_amd")
    scans, poses = [], []
    for i in range(PARTS):
        p, l, pose = synth.lidar_sequence_scan(seed=9, i=i, n_points=N)
        scans.append((p, l))
        poses.append(np_ref.mat_to_qt(pose))
    qts = np.stack(poses)
    es = []
    for p, l in scans:
        e = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
        e.set_target(p, l)
        es.append(e)
    up = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    raw = (np.concatenate([p for p, _ in scans]), np.concatenate([l for _, l in scans]))
    parts = [(e, sicp.TARGET) for e in es]
    p_map = sicp.default_merge_params(leaf_size=LEAF, crop_center=tuple(qts[-1, 4:7]), crop_range=RANGE)
    p_crop = sicp.default_merge_params(leaf_size=0.0, crop_range=RANGE)
    shapes = {"map": (parts, qts, p_map), "crop": (parts[:1], None, p_crop)}
    info = {}
    for name, (ps, q, pp) in shapes.items():  # warm-up: arena blocks, code objects, pinned buffers
        for _ in range(3):
            info[name] = sicp.merge_clouds(ps, q, pp)["info"]
            sicp.merge_clouds(ps, q, pp, want_points=False)
    for _ in range(2):
        up.set_target(*raw)
        up.set_source(*scans[0])
    wall = {k: [] for k in ("map", "map_counts_only", "crop", "crop_counts_only", "set_cloud_800k", "set_cloud_100k")}
    with StageLog() as log:
        for _ in range(args.reps):
            for name, (ps, q, pp) in shapes.items():
                t0 = time.perf_counter(); sicp.merge_clouds(ps, q, pp); wall[name].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter(); sicp.merge_clouds(ps, q, pp, want_points=False)
                wall[name + "_counts_only"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); up.set_target(*raw); up.synchronize(); wall["set_cloud_800k"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); up.set_source(*scans[0]); up.synchronize(); wall["set_cloud_100k"].append((time.perf_counter() - t0) * 1e3)
    rows = log.stages()
    stages = {}
    for name, n_in in (("map", info["map"]["n_in"]), ("crop", info["crop"]["n_in"])):
        mine = [r for r in rows if int(r["n_in"]) == n_in and "result_ms" in r]  # (the calls that read the result back)
        keys = [k for k in mine[0] if k.endswith("_ms")] if mine else []
        stages[name] = {k[:-3] + "_event_ms": spread([r[k] for r in mine]) for k in keys}
        stages[name]["all_stages_event_ms"] = spread([sum(r[k] for k in keys) for r in mine]) if mine else None
    for e in es + [up]:
        e.close()
    return dict(points_per_part=N, parts=PARTS, leaf=LEAF, crop_range=RANGE,
                info={k: {f: v[f] for f in ("n_in", "n_kept", "n_out", "max_voxel_points")} for k, v in info.items()},
                wall_ms={k: spread(v) for k, v in wall.items()}, stages=stages)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge", "timing.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_run(args)), flush=True)
        return 0
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step", "run"],
                       capture_output=True, text=True)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1
    res = json.loads(lines[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
