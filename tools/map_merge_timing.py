#!/usr/bin/env python3
"""What fusing a submap into a global map costs with sicp_map_merge, and with the only route there was before it (evidence for
DESIGN.md 3.9, not a gate).  The submap is the 50 scans of tools/map_timing.py -- 100K points each along a straight track,
leaf 0.2, crop 40 m about the vehicle -- integrated into one map with 19 classes, in the submap's own frame.  Two global maps:
one empty, and one that holds ten such submaps at poses 50 m apart (a small yaw and offset each, as a pose graph leaves them);
the timed call adds the submap at the next pose.
  merge  VoxelMap.merge(submap, pose)                                              (this checkout)
  lossy  submap.extract(dst=handle) + VoxelMap.integrate(handle, pose): every voxel becomes one point, the counts, the
         centroids' weights and the histograms are lost, and the handle's cloud goes through the upload path
         (--lossy-root DIR: import the package from that checkout instead, e.g. the parent commit built in place)
Host wall clock around calls that end in a stream synchronise; before every timed call the global map is rebuilt, untimed.
Warm-up calls of the same shapes first; the median, minimum and maximum of --reps calls.  A second run of the merge child
with SICP_DEBUG and SICP_MAP_LOG set collects the library's own HIP-event stage times of the timed calls.
usage (GPU box): tools/map_merge_timing.py [--out FILE] [--lossy-root DIR] [--reps N]     (the driver)
                 tools/map_merge_timing.py --step merge|lossy [--root DIR]                (a measurement: one JSON line)"""
import argparse, datetime, importlib, json, os, re, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import map_timing
import np_ref
import synth

SCANS, LEAF, RANGE, CLASSES = map_timing.SCANS, map_timing.LEAF, map_timing.RANGE, 19
SUBMAPS, WARMUP = 10, 3


def pose(j):
    """submap j in the global frame: 50 m further up the track, with the small correction a pose graph leaves"""
    return np_ref.mat_to_qt(synth.pose_matrix(0.7 * ((j % 3) - 1) + 0.2, (0.02, -0.01, 1.0), (50.0 * j + 0.13 * (j % 4), 0.21 * ((j % 5) - 2), 0.02 * (j % 3))))


def submap(sicp):
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    e = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    for k in range(SCANS):
        xyz, lab = map_timing.scan(k)
        e.set_source(xyz, lab)
        vm.integrate(e, sicp.SOURCE, np.array([0, 0, 0, 1, 1.0 * k, 0, 0.0]), (1.0 * k, 0.0, 0.0), RANGE)
    e.close()
    return vm


def step(args):
    sys.path.insert(0, args.root or ROOT)
    sicp = importlib.import_module("semantic-icp_amd")
    sub = submap(sicp)
    g = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    handle = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))

    def add(j, timed=None):
        t0 = time.perf_counter()
        if args.step == "merge":
            info = g.merge(sub, pose(j))
            t1 = t2 = time.perf_counter()
            kept = info["n_kept_rows"]
        else:
            out = sub.extract(dst=handle, dst_which=sicp.SOURCE, want_points=False)
            t1 = time.perf_counter()
            info = g.integrate(handle, sicp.SOURCE, pose(j))
            t2 = time.perf_counter()
            kept = info["n_kept"]
        if timed is not None:
            timed.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
        return dict(rows_added=kept, new_voxels=info["n_new_voxels"], voxels_after=info["n_voxels"])

    res = dict(route=args.step, submap_voxels=sub.size()[0], submap_points=sub.size()[1], cases={})
    for name, held in (("empty", 0), ("ten_submaps", SUBMAPS)):
        times, sizes = [], None
        for rep in range(WARMUP + args.reps):
            g.clear()
            for j in range(held):
                add(j)
            before = g.size()
            sys.stderr.write(f"TIMED {name} {rep}\n")
            sys.stderr.flush()
            sizes = dict(global_voxels_before=before[0], global_points_before=before[1], **add(held, times if rep >= WARMUP else None))
            sizes["global_points_after"] = g.size()[1]
        t = np.array(times)
        res["cases"][name] = dict(sizes=sizes, total_ms=map_timing.spread(t[:, 0]))
        if args.step == "lossy":
            res["cases"][name].update(extract_to_handle_ms=map_timing.spread(t[:, 1]), integrate_ms=map_timing.spread(t[:, 2]))
        res["cases"][name]["per_call_ms"] = [round(float(v), 4) for v in t[:, 0]]
    for o in (g, sub, handle):
        o.close()
    return res


def child(step_name, root, reps, log):
    env = dict(os.environ)
    if log:
        env.update(SICP_DEBUG="1", SICP_MAP_LOG="1")
    cmd = ["timeout", "-k", "10", "420", sys.executable, os.path.abspath(__file__), "--step", step_name, "--reps", str(reps)]
    if root:
        cmd += ["--root", os.path.abspath(root)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(r.returncode or 1)
    return json.loads(lines[-1]), r.stderr


def timed_stages(stderr):
    """{case: [{stage: ms}]}: the stage line of the merge that follows every TIMED marker (warm-ups dropped)"""
    out, want = {}, None
    for line in stderr.splitlines():
        m = re.match(r"TIMED (\w+) (\d+)", line)
        if m:
            want = m.group(1) if int(m.group(2)) >= WARMUP else None
        elif line.startswith("sicp_map_merge: ") and want:
            out.setdefault(want, []).append({k: float(v) for k, v in re.findall(r"(\w+)_ms=([0-9.eE+-]+)", line)})
            want = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["merge", "lossy"])
    ap.add_argument("--root")
    ap.add_argument("--lossy-root")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_merge", "timing.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args)), flush=True)
        return 0
    # the two routes alternate, so that a drift of the box shows in both
    merge_a, _ = child("merge", None, args.reps, False)
    lossy_a, _ = child("lossy", args.lossy_root, args.reps, False)
    merge_b, _ = child("merge", None, args.reps, False)
    lossy_b, _ = child("lossy", args.lossy_root, args.reps, False)
    _, log = child("merge", None, args.reps, True)
    stages = timed_stages(log)
    res = dict(date=datetime.date.today().isoformat(), scans_per_submap=SCANS, points_per_scan=map_timing.N, leaf=LEAF, crop_range=RANGE,
               num_classes=CLASSES, submaps_held=SUBMAPS, warmup=WARMUP, reps=args.reps,
               clock="host wall clock around calls that end in a stream synchronise; stages_ms: HIP events on dst's stream (the library's stage log), a run of their own",
               lossy_route="extract(dst=handle) + integrate(handle)" + (" from the package under --lossy-root (the parent commit, built in place)" if args.lossy_root else " from this checkout"),
               runs=dict(merge=[merge_a, merge_b], lossy=[lossy_a, lossy_b]), summary={})
    for name in merge_a["cases"]:
        m = np.concatenate([r["cases"][name]["per_call_ms"] for r in (merge_a, merge_b)])
        l = np.concatenate([r["cases"][name]["per_call_ms"] for r in (lossy_a, lossy_b)])
        st = stages.get(name, [])
        res["summary"][name] = dict(
            merge_ms=map_timing.spread(m), lossy_ms=map_timing.spread(l), merge_over_lossy=round(float(np.median(m) / np.median(l)), 4),
            merge_sizes=merge_a["cases"][name]["sizes"], lossy_sizes=lossy_a["cases"][name]["sizes"],
            stages_ms={k: map_timing.spread([s[k] for s in st]) for k in (st[0] if st else {})},
            stages_sum_ms=map_timing.spread([sum(s.values()) for s in st]) if st else None)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res["summary"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
