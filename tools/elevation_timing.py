#!/usr/bin/env python3
"""What the elevation grid of a voxel map costs next to the host route it replaces (evidence for DESIGN.md 3.19, not a gate).
The map is the 50-scan submap of tools/map_merge_timing.py (100K-point scans along a straight track, leaf 0.2, 19 classes;
597 K voxels).  Four rows, each timed on both routes:
  512 x 512 at cell_voxels = 1 and 256 x 256 at cell_voxels = 2, about the middle of the track, without points and with the
  heights of a 100K-point scan (the 26th, at its pose)
  library    VoxelMap.elevation: the whole call's host wall clock, every array asked for
  host       VoxelMap.get_state() plus tests/elevation_ref.elevation on its rows: what a caller had to do before
Five runs (child processes under a time limit) of `--reps` library calls each after `--warmup`, and of `--host-reps` passes of
the host route after one that is not timed (the first get_state() of a process also allocates its pinned buffer); a run reports
the spread over its calls, the summary the spread of the runs' medians.  The library's answer is compared with the host
route's, byte for byte, once per row and run.
usage (GPU box): tools/elevation_timing.py [--out FILE]     (the driver)
                 tools/elevation_timing.py --step run        (one run: one JSON line on stdout)
                 tools/elevation_timing.py --step profile    (a few calls of every row, for rocprofv3 --kernel-trace --stats)"""
import argparse, datetime, importlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import map_merge_timing
import map_timing

RUNS = 5
SCAN = 25
CENTRE = (25.0, 1.0)
ROWS = {"512x512_b1": dict(width=512, height=512, cell_voxels=1), "256x256_b2": dict(width=256, height=256, cell_voxels=2)}
PARAMS = dict(clearance_voxels=8, ignore=(4,), max_step=0.3, min_clearance=2.0, min_neighbors=3)


def step(args):
    import elevation_ref as ref
    sicp = importlib.import_module("semantic-icp_amd")
    vm = map_merge_timing.submap(sicp)
    xyz, lab = map_timing.scan(SCAN)
    qt = np.array([0, 0, 0, 1, 1.0 * SCAN, 0, 0.0])
    e = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    e.set_source(xyz, lab)
    e.synchronize()
    res = dict(map_voxels=vm.size()[0], map_points=vm.size()[1], scan_points=len(xyz), rows={})
    for name, win in ROWS.items():
        for with_points in (False, True):
            kw = dict(PARAMS, **win)
            p = sicp.default_map_elevation_params(ignore=kw["ignore"], **{k: v for k, v in kw.items() if k != "ignore"})
            call = lambda: vm.elevation(CENTRE, win["width"], win["height"], p, e if with_points else None, sicp.SOURCE, qt)
            got = None
            for _ in range(args.warmup):
                got = call()
            t_lib = []
            for _ in range(args.reps):
                t = time.perf_counter()
                got = call()
                t_lib.append(1e3 * (time.perf_counter() - t))
            row = dict(library_ms=map_timing.spread(t_lib), library_inside_ms=got["info"]["t_total_ms"], n_class=got["info"]["n_class"])
            if args.step == "run":
                t_state, t_ref, want = [], [], None
                for k in range(args.host_reps + 1):  # (the first pass is not timed)
                    t = time.perf_counter()
                    state = vm.get_state()
                    t1 = time.perf_counter()
                    want = ref.elevation(state, ref.defaults(**kw), CENTRE, xyz if with_points else None, qt if with_points else None)
                    t2 = time.perf_counter()
                    if k > 0:
                        t_state.append(1e3 * (t1 - t))
                        t_ref.append(1e3 * (t2 - t1))
                same = all(got[k].tobytes() == want[k].tobytes() for k in want if k != "info")
                row.update(host_get_state_ms=map_timing.spread(t_state), host_restatement_ms=map_timing.spread(t_ref),
                           host_ms=map_timing.spread(np.add(t_state, t_ref)), same_bytes=bool(same),
                           points_in_a_surface_cell=int(np.isfinite(want["point_height"]).sum()) if with_points else 0)
            res["rows"][name + ("_points" if with_points else "")] = row
    e.close()
    vm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run", "profile"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elevation", "timing.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step(args)), flush=True)
        return 0
    runs = []
    for _ in range(RUNS):
        r = subprocess.run(["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "--step", "run", "--warmup", str(args.warmup),
                            "--reps", str(args.reps), "--host-reps", str(args.host_reps)], capture_output=True, text=True)
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            return r.returncode or 1
        runs.append(json.loads(lines[-1]))
    summary = {}
    for name in runs[0]["rows"]:
        lib = [q["rows"][name]["library_ms"]["median"] for q in runs]
        host = [q["rows"][name]["host_ms"]["median"] for q in runs]
        summary[name] = dict(library_ms=map_timing.spread(lib), host_ms=map_timing.spread(host),
                             host_get_state_ms=map_timing.spread([q["rows"][name]["host_get_state_ms"]["median"] for q in runs]),
                             host_restatement_ms=map_timing.spread([q["rows"][name]["host_restatement_ms"]["median"] for q in runs]),
                             library_over_host=round(float(np.median(lib) / np.median(host)), 4),
                             same_bytes=all(q["rows"][name]["same_bytes"] for q in runs))
    res = dict(date=datetime.date.today().isoformat(), scans=map_timing.SCANS, points_per_scan=map_timing.N, leaf=map_timing.LEAF,
               num_classes=map_merge_timing.CLASSES, centre=CENTRE, params=PARAMS, windows=ROWS, runs_n=RUNS, warmup=args.warmup, reps=args.reps,
               host_reps=args.host_reps, clock="host wall clock around calls that end in a stream synchronise; spreads of the runs' medians",
               summary=summary, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(dict(summary=summary, map_voxels=runs[0]["map_voxels"]), indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
