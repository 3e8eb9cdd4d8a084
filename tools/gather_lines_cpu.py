"""Count, on the CPU, the cache lines the accumulate kernel's target gathers touch under two layouts of the target records
("dense gathers"): the 48-byte records `rec`, and the dense arrays `rec_dense` = [n] x 16 | [n] x 16 | [n] x 4.

Recipe: synth.lidar_pair(seed, points); both clouds in Morton order (a stand-in for the engine's Hilbert order); K = 4 nearest
targets of every source point by scipy.spatial.cKDTree, at the identity and at the planted pose; a wave step is 64 consecutive
source points x 4 slots x 3 pieces = 12 gather instructions; the quantity is the number of distinct lines an instruction
touches, summed over the 12 -- for lanes coalesced 64 / 16 / 8 / 4 at a time and for 64- and 128-byte lines.

usage: gather_lines_cpu.py [points] [seed ...]      (numpy and scipy only; prints one JSON document)"""
import json
import os
import sys

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import synth  # noqa: E402

K, WAVE = 4, 64


def morton_order(p):
    lo, ext = p.min(axis=0), float((p.max(axis=0) - p.min(axis=0)).max())
    q = np.minimum(((p - lo) / ext * 2097151.0).astype(np.uint64), np.uint64(2097151))
    code = np.zeros(len(p), dtype=np.uint64)
    for b in range(21):
        for d in range(3):
            code |= ((q[:, d] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + d)
    return np.argsort(code, kind="stable")


def distinct_per_group(v, g):
    """v: [steps, 64] line numbers of one instruction; distinct values inside every group of g consecutive lanes, summed"""
    s = np.sort(v.reshape(v.shape[0], WAVE // g, g), axis=2)
    return int((1 + (np.diff(s, axis=2) != 0).sum(axis=2)).sum())


def piece_addresses(j, n, layout):
    """byte addresses of the three pieces of target j (array bases at 0: the engine's buffers are 256-byte aligned)"""
    j = j.astype(np.int64)
    if layout == "rec":
        return [48 * j, 48 * j + 16, 48 * j + 32]
    return [16 * j, 16 * n + 16 * j, 32 * n + 4 * j]


def count(idx, n_t):
    steps = len(idx) // WAVE
    j = idx[: steps * WAVE].reshape(steps, WAVE, K)
    out = {"wave_steps": steps,
           "distinct_targets_per_wave_step": float(np.mean([len(np.unique(j[s])) for s in range(steps)]))}
    for layout in ("rec", "rec_dense"):
        row = {}
        for line in (64, 128):
            addr = [a // line for c in range(K) for a in piece_addresses(j[:, :, c], n_t, layout)]  # the 12 instructions
            for g in (64, 16, 8, 4):
                row[f"lines_per_wave_step_{g}_lanes_{line}B"] = sum(distinct_per_group(a, g) for a in addr) / steps
            whole = np.stack(addr, axis=2).reshape(steps, -1)
            row[f"distinct_lines_per_whole_step_{line}B"] = float(np.mean([len(np.unique(whole[s])) for s in range(steps)]))
        out[layout] = row
    out["dense_relative_to_rec"] = {k: out["rec_dense"][k] / out["rec"][k] for k in out["rec"] if k.startswith("lines_per_wave_step")}
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    seeds = [int(a) for a in sys.argv[2:]] or [2, 7]
    doc = {"points": n, "K": K, "order": "Morton, 21 bits per axis", "cases": []}
    for seed in seeds:
        ps, _, pt, _, T, _ = synth.lidar_pair(seed, n)
        ps, pt = ps[morton_order(ps)].astype(np.float64), pt[morton_order(pt)].astype(np.float64)
        tree = cKDTree(pt)
        for pose_name, M in (("identity", np.eye(4)), ("planted pose", T)):
            _, idx = tree.query(ps @ M[:3, :3].T + M[:3, 3], k=K)
            doc["cases"].append({"seed": seed, "pose": pose_name, **count(idx, len(pt))})
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
