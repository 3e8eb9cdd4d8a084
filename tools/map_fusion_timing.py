#!/usr/bin/env python3
"""What the map's label fusion costs next to the majority vote it stands beside (evidence for DESIGN.md 3.9, not a gate).  The
50-scan loop of tools/map_timing.py -- 100K-point scans along a straight track, leaf 0.2, crop 40 m about the vehicle -- with
19 classes: the scans' four surfaces are spread over 16 labels and a tenth of the points get a label drawn from all 19, so a
voxel holds one to three non-zero bins.  Every step, in one child process under a time limit:
  fused_labels   VoxelMap.fused_labels of the new 100K-point scan at its pose, before it is integrated
  integrate      the scan into the map
  extract        VoxelMap.extract(crop 40) and VoxelMap.extract_fused(crop 40) to arrays, twice each, alternating
The times are the library's own HIP-event stage times (SICP_DEBUG + SICP_MAP_LOG, one line a call on stderr): the kernels of a
call and its read-back apart, on the map's stream.  sicp_map_extract in the same run is the yardstick.  Reported at the map
sizes reached after 10, 25 and 50 scans: the spread over the calls of the five steps that end there.
usage (GPU box): tools/map_fusion_timing.py [--out FILE]       (the driver)
                 tools/map_fusion_timing.py --step run         (the measurement: one JSON line on stdout, the stage lines on stderr)"""
import argparse, importlib, json, os, re, subprocess, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import map_timing

N, SCANS, LEAF, RANGE, CLASSES = map_timing.N, map_timing.SCANS, map_timing.LEAF, map_timing.RANGE, 19
CHECKPOINTS, WINDOW, REPEATS = map_timing.CHECKPOINTS, map_timing.WINDOW, 2


def scan(i):
    xyz, lab = map_timing.scan(i)
    rng = np.random.default_rng([78, i])
    fine = (lab - 1) * 4 + rng.integers(1, 5, N)  # 1..16: four labels a surface
    noisy = rng.uniform(0, 1, N) < 0.1
    fine[noisy] = rng.integers(1, CLASSES + 1, int(noisy.sum()))
    return xyz, fine.astype(np.uint32)


def confusion():
    rng = np.random.default_rng(79)
    cm = rng.uniform(0.05, 1.0, (CLASSES, CLASSES)) + 2.0 * CLASSES * np.eye(CLASSES)
    return cm / cm.sum(axis=0, keepdims=True)


def step_run(args):
    sicp = importlib.import_module("semantic-icp_amd")
    engine = sicp.Engine(0, sicp.default_params(sicp.MODE_GICP))
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=LEAF, num_classes=CLASSES))
    vm.set_confusion(confusion())
    rows = []
    for k in range(SCANS):
        xyz, lab = scan(k)
        centre = (1.0 * k, 0.0, 0.0)
        qt = np.array([0, 0, 0, 1, centre[0], 0, 0.0])
        engine.set_source(xyz, lab)
        engine.synchronize()
        labels, conf = vm.fused_labels(engine, sicp.SOURCE, qt)
        info = vm.integrate(engine, sicp.SOURCE, qt, centre, RANGE)
        for _ in range(REPEATS):
            vote = vm.extract(crop_center=centre, crop_range=RANGE)
            fused = vm.extract_fused(crop_center=centre, crop_range=RANGE)
        assert vote["xyz"].tobytes() == fused["xyz"].tobytes() and vote["count"].tobytes() == fused["count"].tobytes()
        rows.append(dict(map_voxels=info["n_voxels"], extracted=fused["info"]["n_out"],
                         fused_differs_from_vote=int((vote["labels"] != fused["labels"]).sum()),
                         scan_relabelled=int((labels != lab).sum()), scan_with_evidence=int((conf > 0).sum())))
    vm.close()
    engine.close()
    return rows


def spread(v):
    return map_timing.spread(v)


def stage_lines(stderr, call):
    """[{stage: ms}] of every logged call of that name, in order"""
    out = []
    for line in stderr.splitlines():
        if line.startswith(call + ": "):
            out.append({k: float(v) for k, v in re.findall(r"(\w+)_ms=([0-9.eE+-]+)", line)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["run"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_fusion", "timing.json"))
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
    vote, fused, relabel = (stage_lines(r.stderr, c) for c in ("sicp_map_extract", "sicp_map_extract_fused", "sicp_map_fused_labels"))
    assert len(vote) == len(fused) == SCANS * REPEATS and len(relabel) == SCANS, (len(vote), len(fused), len(relabel))
    res = dict(points_per_scan=N, scans=SCANS, leaf=LEAF, crop_range=RANGE, num_classes=CLASSES, window=WINDOW, repeats=REPEATS,
               clock="HIP events on the map's stream (the library's stage log)", after={})
    for c in CHECKPOINTS:
        w = slice((c - WINDOW) * REPEATS, c * REPEATS)
        v, f, l = vote[w], fused[w], relabel[c - WINDOW:c]
        res["after"][str(c)] = dict(
            sizes=rows[c - 1],
            extract_kernels_ms=spread([s["select_gather"] for s in v]),
            extract_total_ms=spread([s["select_gather"] + s["result"] for s in v]),
            extract_fused_kernels_ms=spread([s["select_gather"] + s["posterior"] for s in f]),
            extract_fused_posterior_ms=spread([s["posterior"] for s in f]),
            extract_fused_total_ms=spread([s["select_gather"] + s["posterior"] + s["result"] for s in f]),
            fused_labels_kernel_ms=spread([s["relabel"] for s in l]),
            fused_labels_total_ms=spread([s["relabel"] + s["result"] for s in l]))
    res["per_call_ms"] = dict(extract=[round(s["select_gather"] + s["result"], 4) for s in vote],
                              extract_fused=[round(s["select_gather"] + s["posterior"] + s["result"], 4) for s in fused],
                              fused_labels=[round(s["relabel"] + s["result"], 4) for s in relabel])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "per_call_ms"}, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
