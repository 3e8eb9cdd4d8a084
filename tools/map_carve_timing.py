#!/usr/bin/env python3
"""What free-space carving costs next to the integrate it stands beside (evidence for DESIGN.md 3.9, not a gate).  The 50-scan
loop of tools/map_timing.py -- 100K-point scans along a straight track, leaf 0.2, range 40 m about the vehicle, 4 classes --
in the order the loop is meant to run.  Every step, in one child process under a time limit:
  carve      VoxelMap.carve of the new scan at its pose, sensor at the scan's origin, max_range 40, the defaults otherwise,
             before the scan is integrated
  integrate  the scan into the map (crop 40)
The times are the library's own HIP-event stage times (SICP_DEBUG + SICP_MAP_LOG, one line a call on stderr), on the map's
stream: carve's kernels (hit marking, the walk, the select, and prune's compaction when rows go) and its whole call;
sicp_map_integrate of the same scan in the same run is the yardstick.  Reported at the map sizes reached after 10, 25 and 50
scans: the spread over the calls of the five steps that end there.
usage (GPU box): tools/map_carve_timing.py [--out FILE]       (the driver)
                 tools/map_carve_timing.py --step run         (the measurement: one JSON line on stdout, the stage lines on stderr)"""
import argparse, importlib, json, os, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import map_fusion_timing
import map_timing

N, SCANS, LEAF, RANGE, CLASSES = map_timing.N, map_timing.SCANS, map_timing.LEAF, map_timing.RANGE, map_timing.CLASSES
CHECKPOINTS, WINDOW = map_timing.CHECKPOINTS, map_timing.WINDOW
KERNELS = ("hits", "walk", "select", "compact")


def step_run(args):
    sicp = importlib.import_module("semantic-icp_amd")
    engine = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    params = sicp.default_map_carve_params(max_range=RANGE)
    rows = []
    for k in range(SCANS):
        xyz, lab = map_timing.scan(k)
        centre = (1.0 * k, 0.0, 0.0)
        qt = np.array([0, 0, 0, 1, centre[0], 0, 0.0])
        engine.set_source(xyz, lab)
        engine.synchronize()
        carved = vm.carve(engine, sicp.SOURCE, qt, None, params)["info"]
        info = vm.integrate(engine, sicp.SOURCE, qt, centre, RANGE)
        rows.append(dict(map_voxels_before=carved["n_voxels"] + carved["n_removed"], rays=carved["n_rays"], steps=carved["n_steps"],
                         touched=carved["n_touched"], hit=carved["n_hit"], removed=carved["n_removed"],
                         spared_hit=carved["n_spared_hit"], map_voxels_after_integrate=info["n_voxels"]))
    vm.close()
    engine.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_carve", "timing.json"))
    args = ap.parse_args()
    if args.step:
        print(json.dumps(step_run(args)), flush=True)
        return 0
    env = dict(os.environ, SICP_DEBUG="1", SICP_MAP_LOG="1")
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--step", "run"], capture_output=True,
                       text=True, env=env)
    lines = [l for l in r.stdout.splitlines() if l.startswith("[")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        return r.returncode or 1
    rows = json.loads(lines[-1])
    carve, integrate = (map_fusion_timing.stage_lines(r.stderr, c) for c in ("sicp_map_carve", "sicp_map_integrate"))
    assert len(carve) == len(integrate) == SCANS, (len(carve), len(integrate))
    spread = map_timing.spread

    def kernels(s):
        return sum(s.get(k, 0.0) for k in KERNELS)

    res = dict(points_per_scan=N, scans=SCANS, leaf=LEAF, max_range=RANGE, num_classes=CLASSES, window=WINDOW,
               clock="HIP events on the map's stream (the library's stage log)", after={})
    for c in CHECKPOINTS:
        v, g = carve[c - WINDOW:c], integrate[c - WINDOW:c]
        res["after"][str(c)] = dict(
            sizes=rows[c - 1],
            carve_walk_ms=spread([s["walk"] for s in v]),
            carve_kernels_ms=spread([kernels(s) for s in v]),
            carve_total_ms=spread([sum(s.values()) for s in v]),
            integrate_kernels_ms=spread([sum(s.values()) for s in g]))
    res["per_call_ms"] = dict(carve_walk=[round(s["walk"], 4) for s in carve], carve=[round(sum(s.values()), 4) for s in carve],
                              integrate=[round(sum(s.values()), 4) for s in integrate])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_call_ms"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
