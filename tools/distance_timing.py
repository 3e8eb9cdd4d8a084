#!/usr/bin/env python3
"""What the distance field of a voxel map costs next to the host route it replaces (evidence for DESIGN.md 3.20, not a gate).
The map is the 50-scan submap of tools/map_merge_timing.py (100K-point scans along a straight track, leaf 0.2, 19 classes;
597 K voxels).  Three rows about the middle of the track, each timed on both routes, warm and in the same process:
  512x512x32_r10          the 3-D field at R = 10, every cell array
  512x512x32_r10_points   the same window, only the point outputs of a 100K-point scan (the 26th, at its pose)
  1024x1024x1_planar_r16  obstacle inflation of the band 0.2 .. 2.0 m at R = 16, every cell array
  library    VoxelMap.distance: the whole call's host wall clock
  host       VoxelMap.get_state(), the window's occupancy grid from its keys, and scipy.ndimage.distance_transform_edt(...,
             return_indices=True) on it (and, for the point row, the look-up of the points' cells): what a caller had to do before
Five runs (child processes under a time limit) of `--reps` library calls each after `--warmup`, and of `--host-reps` passes of
the host route after one that is not timed; a run reports the spread over its calls, the summary the spread of the runs' medians
and the library's slowest and the host's fastest single call over all runs.  Once per row and run dist_sq is compared: the
library's against scipy's squared distance truncated at R^2 (for the point row, the points' values).
usage (GPU box): tools/distance_timing.py [--out FILE]     (the driver)
                 tools/distance_timing.py --step run        (one run: one JSON line on stdout)
                 tools/distance_timing.py --step profile [--row NAME]   (a few calls of every row and of a 256 x 256 x 128
                                                             window at R = 64, or of one of them, for rocprofv3 --kernel-trace
                                                             --stats)"""
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
CENTRE = (25.0, 1.0, 1.0)
BIAS = 1 << 20
ROWS = {
    "512x512x32_r10": dict(shape=(512, 512, 32), params=dict(max_dist_voxels=10), points=False, want=("dist_sq", "nearest", "label")),
    "512x512x32_r10_points": dict(shape=(512, 512, 32), params=dict(max_dist_voxels=10), points=True,
                                  want=("point_cell", "point_dist_sq", "point_nearest", "point_range_sq")),
    "1024x1024x1_planar_r16": dict(shape=(1024, 1024, 1), params=dict(max_dist_voxels=16, planar=1, z_min=0.2, z_max=2.0), points=False,
                                   want=("dist_sq", "nearest", "label")),
}
PROFILE_ONLY = {"256x256x128_r64": dict(shape=(256, 256, 128), params=dict(max_dist_voxels=64), points=False, want=("dist_sq",))}


def host_route(vm, row, info, xyz, qt):
    """get_state(), the occupancy grid of the window, scipy's exact transform with the nearest cell's indices; -> (dist_sq
    [nz, ny, nx] truncated as the call truncates it, the points' dist_sq or None, ms of get_state, ms of the rest)"""
    from scipy import ndimage
    import distance_ref as ref
    import np_ref
    nx, ny, nz = row["shape"]
    p = ref.defaults(nx=nx, ny=ny, nz=nz, **row["params"])
    R = p["max_dist_voxels"]
    t0 = time.perf_counter()
    state = vm.get_state()
    t1 = time.perf_counter()
    key = state["key"].astype(np.int64)
    i, j, k = (key & 0x1FFFFF) - BIAS - info["x0"], ((key >> 21) & 0x1FFFFF) - BIAS - info["y0"], (key >> 42) - BIAS
    inv = ref.inv_leaf(state["leaf_size"])
    if p["planar"]:
        lo, hi = ref.level_of(p["z_min"], inv, -(BIAS - 1), BIAS - 1), ref.level_of(p["z_max"], inv, -(BIAS - 1), BIAS - 1)
        keep = (k >= lo) & (k <= hi)
        k = np.zeros_like(k)
    else:
        k = k - info["z0"]
        keep = (k >= 0) & (k < nz)
    keep &= (i >= 0) & (i < nx) & (j >= 0) & (j < ny)
    free = np.ones((nz, ny, nx), bool)
    free[k[keep], j[keep], i[keep]] = False
    if free.all():
        sq = np.full(free.shape, -1, np.int64)
    else:
        edt, idx = ndimage.distance_transform_edt(free, return_indices=True)
        sq = np.rint(edt * edt).astype(np.int64)
        sq = np.where(sq <= R * R, sq, -1)
    pd = None
    if row["points"]:
        q = np_ref.transform_points(np_ref.qt_to_mat(qt), xyz)
        v = np.floor((q * inv).astype(np.float32)).astype(np.int64) - np.array([info["x0"], info["y0"], info["z0"]])
        inside = ((v >= 0) & (v < np.array([nx, ny, nz]))).all(axis=1)
        pd = np.full(len(xyz), -1, np.int64)
        pd[inside] = sq[v[inside, 2], v[inside, 1], v[inside, 0]]
    t2 = time.perf_counter()
    return sq, pd, 1e3 * (t1 - t0), 1e3 * (t2 - t1)


def step(args):
    sicp = importlib.import_module("semantic-icp_amd")
    vm = map_merge_timing.submap(sicp)
    xyz, lab = map_timing.scan(SCAN)
    qt = np.array([0, 0, 0, 1, 1.0 * SCAN, 0, 0.0])
    e = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    e.set_source(xyz, lab)
    e.synchronize()
    res = dict(map_voxels=vm.size()[0], map_points=vm.size()[1], scan_points=len(xyz), rows={})
    rows = dict(ROWS, **PROFILE_ONLY) if args.step == "profile" else ROWS
    if args.row:
        rows = {args.row: rows[args.row]}
    for name, row in rows.items():
        p = sicp.default_map_distance_params(**row["params"])
        call = lambda: vm.distance(CENTRE, row["shape"], p, e if row["points"] else None, sicp.SOURCE, qt, want=row["want"])
        got = None
        for _ in range(args.warmup):
            got = call()
        t_lib = []
        for _ in range(args.reps):
            t = time.perf_counter()
            got = call()
            t_lib.append(1e3 * (time.perf_counter() - t))
        info = got["info"]
        out = dict(library_ms=map_timing.spread(t_lib), library_slowest_ms=max(t_lib), library_inside_ms=info["t_total_ms"],
                   n_obstacles=info["n_obstacles"], n_reached=info["n_reached"], max_dist_sq=info["max_dist_sq"],
                   n_points_inside=info["n_points_inside"])
        if args.step == "run":
            t_state, t_rest, sq, pd = [], [], None, None
            for k in range(args.host_reps + 1):  # (the first pass is not timed)
                sq, pd, a, b = host_route(vm, row, info, xyz, qt)
                if k > 0:
                    t_state.append(a)
                    t_rest.append(b)
            same = np.array_equal(got["point_dist_sq"], pd) if row["points"] else np.array_equal(got["dist_sq"], sq)
            total = np.add(t_state, t_rest)
            out.update(host_get_state_ms=map_timing.spread(t_state), host_transform_ms=map_timing.spread(t_rest), host_ms=map_timing.spread(total),
                       host_fastest_ms=float(total.min()), same_dist_sq=bool(same))
        res["rows"][name] = out
    e.close()
    vm.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run", "profile"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance", "timing.json"))
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--row", help="with --step: this row alone (a profile then holds one window's kernels)")
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
        sys.stderr.write(f"run {len(runs)} of {RUNS} done\n")
    summary = {}
    for name in runs[0]["rows"]:
        lib = [q["rows"][name]["library_ms"]["median"] for q in runs]
        host = [q["rows"][name]["host_ms"]["median"] for q in runs]
        slowest, fastest = max(q["rows"][name]["library_slowest_ms"] for q in runs), min(q["rows"][name]["host_fastest_ms"] for q in runs)
        summary[name] = dict(library_ms=map_timing.spread(lib), host_ms=map_timing.spread(host),
                             host_get_state_ms=map_timing.spread([q["rows"][name]["host_get_state_ms"]["median"] for q in runs]),
                             host_transform_ms=map_timing.spread([q["rows"][name]["host_transform_ms"]["median"] for q in runs]),
                             library_slowest_ms=slowest, host_fastest_ms=fastest, library_slowest_below_host_fastest=bool(slowest < fastest),
                             library_over_host=round(float(np.median(lib) / np.median(host)), 5),
                             same_dist_sq=all(q["rows"][name]["same_dist_sq"] for q in runs))
    res = dict(date=datetime.date.today().isoformat(), scans=map_timing.SCANS, points_per_scan=map_timing.N, leaf=map_timing.LEAF,
               num_classes=map_merge_timing.CLASSES, centre=CENTRE, rows={k: dict(v, shape=list(v["shape"])) for k, v in ROWS.items()}, runs_n=RUNS,
               warmup=args.warmup, reps=args.reps, host_reps=args.host_reps,
               clock="host wall clock around calls that end in a stream synchronise; spreads of the runs' medians", summary=summary, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(dict(summary=summary, map_voxels=runs[0]["map_voxels"]), indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
