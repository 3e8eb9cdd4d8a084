"""Inputs of the place-recognition tests (tests/test_place_cpu.py, tests/test_gpu_place.py): boundary points with their expected
cells, seeded clouds and descriptors, and the street scene of 17 keyframes and 4 revisits."""
from __future__ import annotations

import functools
import math

import numpy as np

import place_ref as PR
import synth

# ---- boundary points at R = 20, S = 60, max_range = 40 (rings 2 m wide, sectors 6 degrees), min_range = 1 -------------------
# (x, y, z), kept, ring, sector -- each value follows from rules 1 and 3 by hand:
#   +x axis: dy == 0 and dx > 0 -> upper half, no boundary j >= 1 passed (cos*0 - sin*x < 0) -> sector 0
#   +y axis: upper; boundaries j = 1..15 (angles 6..90 degrees) are passed, cos(90 deg) is 6e-17 > 0 so j = 15 counts -> sector 15
#   -x axis: dy == 0 and dx < 0 -> lower, mirrored to +x -> sector 0 + 30
#   -y axis: lower, mirrored to +y -> 15 + 30
#   the origin: dy == 0, dx == 0 -> lower; every predicate is 0 - 0 >= 0 -> 29 + 30 = 59; d2 = 0 < min_range^2 -> dropped
#     (kept, ring 0, with min_range = 0: BOUNDARY_ORIGIN_CELL)
#   d2 exactly on edge2[1] = 4: (2, 0, 0) -> ring 1 (>= counts); edge2[3] = 36: (0, 6, 0) -> ring 3
#   at max_range: (40, 0, 0) has d2 = 1600 = edge2[20] -> out; (39.99, 0, 0) -> ring 19
#   at min_range = 1: (1, 0, 0) has d2 = 1 >= 1 -> kept, ring 0; (0.999, 0, 0) -> dropped
BOUNDARY_PARAMS = dict(R=20, S=60, max_range=40.0, min_range=1.0)
BOUNDARY_POINTS = [
    ((5.0, 0.0, 0.0), True, 2, 0),
    ((0.0, 5.0, 0.0), True, 2, 15),
    ((-5.0, 0.0, 0.0), True, 2, 30),
    ((0.0, -5.0, 0.0), True, 2, 45),
    ((0.0, 0.0, 0.0), False, 0, 59),
    ((2.0, 0.0, 0.0), True, 1, 0),
    ((0.0, 6.0, 0.0), True, 3, 15),
    ((40.0, 0.0, 0.0), False, 19, 0),
    ((39.99, 0.0, 0.0), True, 19, 0),
    ((1.0, 0.0, 0.0), True, 0, 0),
    ((0.999, 0.0, 0.0), False, 0, 0),
]
BOUNDARY_ORIGIN_CELL = (0, 59)


def boundary_xyz():
    return np.array([p for p, _, _, _ in BOUNDARY_POINTS], dtype=np.float32)


def cloud(seed: int, n: int, max_range: float, C: int, with_specials: bool = True):
    """A seeded cloud about the origin: points out to 1.2 * max_range, labels 0..C, the boundary points scaled to max_range,
    and (with_specials) NaN / Inf points mixed in.  Returns xyz float32 [m, 3], labels uint32 [m]."""
    rng = np.random.default_rng(seed)
    r = max_range * 1.2 * np.sqrt(rng.uniform(0, 1, n))
    a = rng.uniform(-np.pi, np.pi, n)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-4.0, 140.0, n)], axis=1).astype(np.float32)
    xyz[: n // 8, 2] = rng.uniform(-3.0, 4.0, n // 8).astype(np.float32)
    extra = boundary_xyz() * np.float32(max_range / 40.0)
    # the diagonals (a sector boundary when S is a multiple of 8) and a point straight above the origin
    diag = np.array([(3, 3, 1), (-3, 3, 1), (-3, -3, 1), (3, -3, 1), (0, 0, 1)], dtype=np.float32) * np.float32(max_range / 40.0)
    parts = [xyz, extra, diag]
    if with_specials:
        bad = np.array([(np.nan, 1, 1), (1, np.inf, 1), (1, 1, -np.inf), (np.nan, np.nan, np.nan)], dtype=np.float32)
        parts.append(bad)
    xyz = np.concatenate(parts).astype(np.float32)
    order = rng.permutation(xyz.shape[0])
    xyz = np.ascontiguousarray(xyz[order])
    labels = rng.integers(0, C + 1, xyz.shape[0]).astype(np.uint32)
    return xyz, labels


def descriptors(seed: int, n: int, R: int, S: int, codes: int, fill: float = 0.6):
    """n seeded descriptors [n, R, S] uint8 with codes 1..codes in about `fill` of the cells"""
    rng = np.random.default_rng(seed)
    d = rng.integers(1, codes + 1, (n, R, S)).astype(np.uint8)
    d[rng.uniform(0, 1, (n, R, S)) >= fill] = 0
    return d


def search_database(seed: int, n: int, R: int, S: int, codes: int = 6):
    """A database that exercises the ranking: random entries, then -- where n allows -- duplicates (ties between ids), a
    descriptor periodic in the sector (ties between shifts), all-empty entries, and rolled copies of entry 0.  Returns
    (entries [n, R, S], queries [4, R, S]): entry 0 rolled, a fresh random one, the periodic one, an all-empty one."""
    d = descriptors(seed, n, R, S, codes)
    period = np.tile(descriptors(seed + 1, 1, R, 2, codes, fill=1.0)[0], (1, S // 2))
    if n >= 8:
        d[5] = d[2]
        d[n - 1] = d[2]
        d[3] = period
        d[4] = 0
        d[6] = 0
        d[7] = np.roll(d[0], 1, axis=1)
    q = np.stack([np.roll(d[0], -(S // 3), axis=1), descriptors(seed + 2, 1, R, S, codes)[0], period, np.zeros((R, S), np.uint8)])
    return d, q


# ---- the street scene --------------------------------------------------------------------------------------------------
SCENE_SEED = 11
SCENE_RAYS = 600          # azimuth steps of the 64-ring scan
SCENE_RANGE = 40.0
SCENE_CLASSES = 11
SCENE_HEIGHT = 1.73
# (entry revisited, offset from it in the world (m, at most 0.4 long), yaw in degrees)
SCENE_REVISITS = [(3, (0.0, 0.0), 183.0), (8, (0.25, -0.1), 90.0), (11, (-0.3, 0.2), -47.0), (14, (0.1, 0.38), 12.0)]


def _pose(x, y, yaw_deg):
    T = synth.pose_matrix(yaw_deg, (0, 0, 1), (x, y, SCENE_HEIGHT))
    return T


@functools.lru_cache(maxsize=1)
def scene():
    """{"entries": [(xyz, labels)] * 17, "entry_poses", "queries": [(xyz, labels)] * 4, "query_poses", "revisits"}: 17 keyframes
    5 m apart along the street with heading 0, and 4 revisits (sensor frames, 64 x 600 rays, range 40 m, seeded)"""
    rng = np.random.default_rng(SCENE_SEED)
    boxes, poles = synth._street(rng)
    entries, entry_poses = [], []
    for i in range(17):
        T = _pose(-40.0 + 5.0 * i, 0.3, 0.0)
        p, l = synth._lidar_scan(rng, T, boxes, poles, SCENE_RAYS, SCENE_RANGE, 0.01)
        entries.append((p.astype(np.float32), l.astype(np.uint32)))
        entry_poses.append(T)
    queries, query_poses = [], []
    for e, (ox, oy), yaw in SCENE_REVISITS:
        T = _pose(-40.0 + 5.0 * e + ox, 0.3 + oy, yaw)
        p, l = synth._lidar_scan(rng, T, boxes, poles, SCENE_RAYS, SCENE_RANGE, 0.01)
        queries.append((p.astype(np.float32), l.astype(np.uint32)))
        query_poses.append(T)
    return {"entries": entries, "entry_poses": entry_poses, "queries": queries, "query_poses": query_poses, "revisits": SCENE_REVISITS}


def scene_params(channel: int):
    return PR.params(R=20, S=60, max_range=SCENE_RANGE, channel=channel, num_classes=SCENE_CLASSES if channel == PR.LABEL else 0)


def expected_shift(yaw_deg: float, S: int) -> int:
    return int(round(math.radians(yaw_deg) / (PR.TWO_PI / S))) % S


def cyclic_distance(a: int, b: int, S: int) -> int:
    d = (a - b) % S
    return min(d, S - d)


def pose_distance(a, b):
    """(rotation angle in rad, translation distance in m) between two 4x4 poses"""
    D = np.linalg.inv(a) @ b
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1.0) / 2.0))
    return math.acos(c), float(np.linalg.norm(D[:3, 3]))


def loop_closure_figures(db, sc, k):
    """Revisit k of the scene (needs a GPU): the query's candidates, then sicp_align (EM, C = 11) of the query onto the entry found, once from
    place_init_qt(yaw) and once from the true relative pose.  Returns the figures the test asserts on."""
    (xyz, lab), (entry, _, yaw_deg) = sc["queries"][k], sc["revisits"][k]
    truth = np.linalg.inv(sc["entry_poses"][entry]) @ sc["query_poses"][k]
    import importlib

    import np_ref

    sicp = importlib.import_module("semantic-icp_amd")
    cm = synth.confusion_matrix(SCENE_CLASSES)
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = SCENE_CLASSES
    with sicp.Engine(0, p) as e:
        e.set_confusion(cm)
        e.set_source(xyz, lab)
        cands = db.query(e, top_k=3)
        e.set_target(*sc["entries"][cands[0]["id"]])
        from_place, _ = e.align(sicp.place_init_qt(cands[0]["yaw"]))
        from_truth, _ = e.align(np_ref.mat_to_qt(truth))
    A, B = np_ref.qt_to_mat(from_place), np_ref.qt_to_mat(from_truth)
    return {"entry": entry, "candidates": cands, "yaw_true_deg": yaw_deg, "yaw_found_deg": math.degrees(cands[0]["yaw"]),
            "place_vs_truth_start": pose_distance(A, B), "place_vs_ground_truth": pose_distance(A, truth),
            "truth_start_vs_ground_truth": pose_distance(B, truth)}
