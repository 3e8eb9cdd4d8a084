#!/usr/bin/env python3
"""What a handle's life costs with the handle pool and without it (evidence for DESIGN.md's handle-pool row, not a gate).
One cycle is what the reference's drivers do per pair: sicp_create, set_params, set_confusion, both clouds of
synth.lidar_pair(seed=2, n_points=100000), one EM align() from the identity, sicp_destroy.  20 cycles as they come (the
second cycle on finds the first one's handle parked) and 20 with sicp_release_pool between the cycles (every handle is made
from nothing and really freed; the release itself is outside the cycle and timed on its own).  Host wall clock around calls
that end synchronised: create, the align (the first use of the handle's buffers), destroy, and the whole cycle; medians
with their spread.  SICP_LIB selects another build of the library, as for every tool.
usage (GPU box): tools/handle_lifetime_timing.py [--out FILE]     (the driver)
                 tools/handle_lifetime_timing.py --step run       (the measurement, prints one JSON line)"""
import argparse, importlib, json, os, subprocess, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N, CYCLES = 100_000, 20


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(n=int(v.size), median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def step_run(args):
    import synth

    sicp = importlib.import_module("semantic-icp_amd")
    src, sl, tgt, tl, _, cm = synth.lidar_pair(seed=2, n_points=N)
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = cm.shape[0]
    ident = np.array([0, 0, 0, 1, 0, 0, 0.0])
    release = lambda: sicp.lib().sicp_release_pool(0)

    def cycle(t):
        t0 = time.perf_counter()
        e = sicp.Engine(0)
        t1 = time.perf_counter()
        e.set_params(p)
        e.set_confusion(cm)
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        t2 = time.perf_counter()
        qt, st = e.align(ident)
        t3 = time.perf_counter()
        e.close()
        t4 = time.perf_counter()
        for k, v in (("create_ms", t1 - t0), ("first_align_ms", t3 - t2), ("destroy_ms", t4 - t3), ("cycle_ms", t4 - t0)):
            t.setdefault(k, []).append(v * 1e3)
        return qt.tobytes(), st["outer_iters"]

    with sicp.Engine(0) as warm:  # the runtime's own first-use costs (context, code objects) belong to neither leg
        warm.set_params(p)
        warm.set_confusion(cm)
        warm.set_source(src, sl)
        warm.set_target(tgt, tl)
        want = warm.align(ident)
        want = (want[0].tobytes(), want[1]["outer_iters"])
    release()
    res = dict(points=N, cycles=CYCLES, lib=os.environ.get("SICP_LIB", "product"), same_result_every_cycle=True)
    for leg in ("pool", "release_between"):
        t = {}
        for _ in range(CYCLES):
            res["same_result_every_cycle"] &= cycle(t) == want
            if leg == "release_between":
                t0 = time.perf_counter()
                release()
                t.setdefault("release_pool_ms", []).append((time.perf_counter() - t0) * 1e3)
        res[leg] = {k: spread(v) for k, v in t.items()}
        release()
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
        json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
