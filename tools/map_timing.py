#!/usr/bin/env python3
"""What a step of a rolling map costs with the persistent voxel map and with the chained merge it replaces (evidence for
DESIGN.md 3.9, not a gate).  50 synthetic labelled scans of 100K points along a straight track (1 m a scan; ground, two walls
and clutter within 40 m of the sensor), leaf 0.2, crop 40 m about the vehicle.  Every step, in one loop of one child process
under a time limit, both routes take the same scan from the same handle:
  map    VoxelMap.integrate(scan at its pose, crop 40) + VoxelMap.extract(crop 40) to arrays
  merge  merge_clouds([map_engine, scan_engine], dst=map_engine) with the same leaf and crop: the recipe of sicp_merge_clouds'
         documentation, whose map is a cloud
Host wall clock around the calls (both end in a stream synchronise).  Reported at the map sizes reached after 10, 25 and 50
scans: the spread over the five steps that end there, with the sizes of both maps.
usage (GPU box): tools/map_timing.py [--out FILE]       (the driver)
                 tools/map_timing.py --step run         (the measurement, prints one JSON line)"""
import argparse, importlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, SCANS, LEAF, RANGE, CLASSES = 100_000, 50, 0.2, 40.0, 4
CHECKPOINTS, WINDOW = (10, 25, 50), 5


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(n=int(v.size), median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def scan(i):
    """100K points in the sensor frame: ground (label 1), two walls along the track (2, 3), clutter (4); 1 cm noise"""
    rng = np.random.default_rng([77, i])
    n_g, n_w = N // 2, N // 5
    r, a = 40.0 * np.sqrt(rng.uniform(0, 1, n_g)), rng.uniform(0, 2 * np.pi, n_g)
    ground = np.stack([r * np.cos(a), r * np.sin(a), np.full(n_g, -1.7)], axis=1)
    walls = [np.stack([rng.uniform(-38, 38, n_w), np.full(n_w, y), rng.uniform(-1.7, 4, n_w)], axis=1) for y in (-9.0, 11.0)]
    n_c = N - n_g - 2 * n_w
    clutter = np.stack([rng.uniform(-30, 30, n_c), rng.uniform(-8, 10, n_c), rng.uniform(-1.7, 1.0, n_c)], axis=1)
    xyz = np.concatenate([ground] + walls + [clutter]) + rng.normal(0, 0.01, (N, 3))
    lab = np.concatenate([np.full(n_g, 1), np.full(n_w, 2), np.full(n_w, 3), np.full(n_c, 4)]).astype(np.uint32)
    order = rng.permutation(N)
    return xyz[order].astype(np.float32), lab[order]


def step_run(args):
    sicp = importlib.import_module("semantic-icp_amd")
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    scan_engine = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    map_engine = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    t_map, t_int, t_ext, t_merge, rows = [], [], [], [], []
    for k in range(SCANS):
        xyz, lab = scan(k)
        centre = (1.0 * k, 0.0, 0.0)
        qt = np.array([0, 0, 0, 1, centre[0], 0, 0.0])
        scan_engine.set_source(xyz, lab)
        scan_engine.synchronize()
        t0 = time.perf_counter()
        info = vm.integrate(scan_engine, sicp.SOURCE, qt, centre, RANGE)
        t1 = time.perf_counter()
        out = vm.extract(crop_center=centre, crop_range=RANGE)
        t2 = time.perf_counter()
        mp = sicp.default_merge_params(leaf_size=LEAF, crop_center=centre, crop_range=RANGE)
        if k == 0:
            merged = sicp.merge_clouds([(scan_engine, sicp.SOURCE)], qt[None], mp, dst=(map_engine, sicp.TARGET))
            t3 = time.perf_counter()
        else:
            merged = sicp.merge_clouds([(map_engine, sicp.TARGET), (scan_engine, sicp.SOURCE)], np.stack([ident, qt]), mp,
                                       dst=(map_engine, sicp.TARGET))
            t3 = time.perf_counter()
        t_int.append((t1 - t0) * 1e3); t_ext.append((t2 - t1) * 1e3); t_map.append((t2 - t0) * 1e3); t_merge.append((t3 - t2) * 1e3)
        rows.append(dict(map_voxels=info["n_voxels"], map_new_voxels=info["n_new_voxels"], map_extracted=out["info"]["n_out"],
                         merge_points_in=merged["info"]["n_in"], merge_points_out=merged["info"]["n_out"]))
    res = dict(points_per_scan=N, scans=SCANS, leaf=LEAF, crop_range=RANGE, num_classes=CLASSES, window=WINDOW, after={})
    for c in CHECKPOINTS:
        w = slice(c - WINDOW, c)
        res["after"][str(c)] = dict(sizes=rows[c - 1], integrate_plus_extract_ms=spread(t_map[w]), integrate_ms=spread(t_int[w]),
                                    extract_ms=spread(t_ext[w]), chained_merge_ms=spread(t_merge[w]))
    res["per_step_ms"] = dict(integrate_plus_extract=[round(v, 3) for v in t_map], chained_merge=[round(v, 3) for v in t_merge])
    vm.close()
    scan_engine.close()
    map_engine.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_map", "timing.json"))
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
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_step_ms"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
