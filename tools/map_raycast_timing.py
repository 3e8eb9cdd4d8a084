#!/usr/bin/env python3
"""What a ray cast of the voxel map costs next to the carve walk it shares its lookup with (evidence for DESIGN.md 3.9, not a
gate).  The 50-scan loop of tools/map_timing.py -- 100K-point scans along a straight track, leaf 0.2, range 40 m about the
vehicle, 4 classes.  Every step, in one loop of one child process under a time limit, before the scan is integrated:
  carve (dry)     VoxelMap.carve(dry_run=1) of the new scan at its pose, max_range 40: the yardstick, its walk visits every
                  candidate of every ray
  own ends        VoxelMap.raycast with the scan's own points as ends, max_range 40: the same rays, stopped at the first hit
  pattern         VoxelMap.raycast of a 64 x 1800 lidar_ray_ends pattern (elevations -25 .. 3 degrees, 40 m) from the vehicle's
                  pose, without dst and with dst (the visible rows into an Engine's target slot)
The times are the library's own HIP-event stage times (SICP_DEBUG + SICP_MAP_LOG, one line a call on stderr) on the map's
stream; for the two pattern calls also the call's host wall clock (info.t_total_ms), which holds the copies and dst's upload.
Reported at the map sizes reached after 10, 25 and 50 scans: the spread over the calls of the five steps that end there, and
the walk's ns per voxel tested beside carve's ns per candidate.
usage (GPU box): tools/map_raycast_timing.py [--out FILE]       (the driver)
                 tools/map_raycast_timing.py --step run         (the measurement: one JSON line on stdout, the stage lines on stderr)"""
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
RINGS, AZIMUTHS, ELEV = 64, 1800, (-25.0, 3.0)


def step_run(args):
    sicp = importlib.import_module("semantic-icp_amd")
    engine = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    target = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    carve_params = sicp.default_map_carve_params(max_range=RANGE, dry_run=1)
    own_params = sicp.default_map_raycast_params(max_range=RANGE)
    pattern = sicp.lidar_ray_ends(RINGS, AZIMUTHS, ELEV[0], ELEV[1], RANGE)
    rows = []
    for k in range(SCANS):
        xyz, lab = map_timing.scan(k)
        centre = (1.0 * k, 0.0, 0.0)
        qt = np.array([0, 0, 0, 1, centre[0], 0, 0.0])
        engine.set_source(xyz, lab)
        engine.synchronize()
        carved = vm.carve(engine, sicp.SOURCE, qt, None, carve_params)["info"]
        own = vm.raycast(xyz, qt, None, own_params)["info"]
        plain = vm.raycast(pattern, qt)["info"]
        with_dst = dict(t_total_ms=0.0, n_visible=0)
        if plain["n_visible"] > 0:  # (the first step's map is empty: a dst would be refused)
            with_dst = vm.raycast(pattern, qt, dst=target, dst_which=sicp.TARGET)["info"]
        vm.integrate(engine, sicp.SOURCE, qt, centre, RANGE)
        rows.append(dict(map_voxels=carved["n_voxels"], carve_rays=carved["n_rays"], carve_candidates=carved["n_steps"],
                         own_rays=own["n_rays"], own_tested=own["n_steps"], own_hits=own["n_hits"], own_visible=own["n_visible"],
                         pattern_rays=plain["n_rays"], pattern_tested=plain["n_steps"], pattern_hits=plain["n_hits"],
                         pattern_visible=plain["n_visible"], dst=int(plain["n_visible"] > 0),
                         pattern_wall_ms=plain["t_total_ms"], pattern_dst_wall_ms=with_dst["t_total_ms"]))
    vm.close()
    engine.close()
    target.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_raycast", "timing.json"))
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
    carve = map_fusion_timing.stage_lines(r.stderr, "sicp_map_carve")
    casts = map_fusion_timing.stage_lines(r.stderr, "sicp_map_raycast")
    gathers = map_fusion_timing.stage_lines(r.stderr, "sicp_map_raycast (visible rows)")
    n_dst = sum(row["dst"] for row in rows)
    assert len(carve) == SCANS and len(casts) == 2 * SCANS + n_dst and len(gathers) == n_dst, (len(carve), len(casts), len(gathers))
    own, plain, with_dst, gather = [], [], [], []
    it, ig = iter(casts), iter(gathers)
    for row in rows:  # the calls of a step in the order they were made
        own.append(next(it))
        plain.append(next(it))
        with_dst.append(next(it) if row["dst"] else {})
        gather.append(next(ig) if row["dst"] else {})
    spread = map_timing.spread

    def per(ms, counts):
        return spread([1e6 * t / max(c, 1) for t, c in zip(ms, counts)])

    res = dict(points_per_scan=N, scans=SCANS, leaf=LEAF, max_range=RANGE, num_classes=CLASSES, window=WINDOW,
               pattern=dict(rings=RINGS, azimuths=AZIMUTHS, elev_deg=ELEV, rays=RINGS * AZIMUTHS),
               rays_per_wave=128, clock="HIP events on the map's stream (the library's stage log); *_wall_ms: the call's host clock",
               after={})
    for c in CHECKPOINTS:
        w = slice(c - WINDOW, c)
        rw = rows[w]
        res["after"][str(c)] = dict(
            sizes={k: v for k, v in rows[c - 1].items() if not k.endswith("_ms")},
            carve_walk_ms=spread([s["walk"] for s in carve[w]]),
            carve_ns_per_candidate=per([s["walk"] for s in carve[w]], [q["carve_candidates"] for q in rw]),
            own_ends_walk_ms=spread([s["walk"] for s in own[w]]),
            own_ends_stages_ms=spread([sum(s.values()) for s in own[w]]),
            own_ends_ns_per_tested=per([s["walk"] for s in own[w]], [q["own_tested"] for q in rw]),
            pattern_walk_ms=spread([s["walk"] for s in plain[w]]),
            pattern_stages_ms=spread([sum(s.values()) for s in plain[w]]),
            pattern_ns_per_tested=per([s["walk"] for s in plain[w]], [q["pattern_tested"] for q in rw]),
            pattern_dst_stages_ms=spread([sum(s.values()) + sum(g.values()) for s, g in zip(with_dst[w], gather[w])]),
            pattern_wall_ms=spread([q["pattern_wall_ms"] for q in rw]),
            pattern_dst_wall_ms=spread([q["pattern_dst_wall_ms"] for q in rw]))
    res["per_call_ms"] = dict(carve_walk=[round(s["walk"], 4) for s in carve], own_ends_walk=[round(s["walk"], 4) for s in own],
                              pattern_walk=[round(s["walk"], 4) for s in plain])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_call_ms"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
