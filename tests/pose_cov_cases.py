"""Inputs of the pose-covariance path tests (tests/test_pose_cov_cases_cpu.py on the oracle and the restatement alone,
tests/test_gpu_pose_cov_paths.py through the library): crafted pairs whose sorted slot layout is known in advance, a model
of the tile and owner rule of csrc/pose_cov_kernels.hip, the case list and the bar.

What the cases are about: the target pass sorts a pair's n_s K slots by (target, slot), gated-out slots last, cuts them
into tiles of kPoseCovTile = 8 with 256 tiles (2048 slots) per workgroup, sums a run (the slots of one target) that lies
inside a tile at once, and chains the pieces of a run that crosses tile edges to the tile where it starts (its owner).

Crafted pairs.  The device orders the targets along a curve of its own, so a test cannot know which target's run comes
first.  It does not have to when every run has the same length L: run r then starts at slot r L whatever the order.  The
target is T groups of K points (a group within about 0.5 m, groups 100 m apart on a grid), the source L points within
0.1 m of every group's centre -- each finds exactly its group's K points -- and g points 70 m from every target, beyond the
gate (gate_sq = 250) in every mode.  Under the identity pose there are T K runs of L slots and g K gated slots behind them.
Both clouds carry one label, so EM weights exist and label segments play no part.

The grid is flat (z = 0, every point within 4 mm of it; 64 groups are 8 x 8 cells, so coordinates stay below 1 km): every
neighbourhood -- 20 points of one group or of groups 100 m apart -- then has the normal z, every slot has the same
M ~ diag(1/2, 1/2, 1 / (2 epsilon)), and no slot's share of S_tgt is dwarfed by another's.  With normals at random (a 3-D
grid) the few slots whose two normals happen to agree carry S_tgt, and a lost piece of any other run would hide under the
bar: tests/test_pose_cov_cases_cpu.py checks on the reference alone that none can."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import accumulate_cases as A
import pose_cov_ref as ref

TILE = 8            # kPoseCovTile (tests/test_pose_cov_cases_cpu.py reads it from csrc/kernels.h)
LANES = 256         # tiles per workgroup of the tile and the owner kernel
GATE_SQ = 250.0     # sicp_default_params
SPACING = 100.0     # between group centres
FLAT = 0.004        # half thickness of the sheet all points lie in
C = 11              # classes of the confusion matrix; every point has label 1
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
BAR_FLOOR = 1e-8    # tests/test_gpu_pose_covariance.py
BAR_MARGIN = 4.0    # tests/test_gpu_accumulate_paths.py: the margin over the reference's own float64 error


# ---- the tile and owner rule ------------------------------------------------------------------------------------------------------------
def tile_geometry(run_lengths, gated, tile=TILE, lanes=LANES):
    """What pose_cov_tile_jobs / pose_cov_owner_jobs meet on sorted slots made of runs of these lengths (in order) followed
    by `gated` gated-out slots, from the runs' intervals alone.  A run over the tiles ft .. lt (lt > ft) makes ft its owner
    (kOwnsLast), every tile between a pass-through (kFirstContinues | kPassThrough) and lt the end of the chain
    (kFirstContinues alone); the owner walks lt - ft + 1 tiles.  Counts:
      inside              runs that lie in one tile (summed and squared by the tile kernel)
      owns_last           tiles with kOwnsLast = runs that cross a tile edge = owner chains
      first_continues     tiles with kFirstContinues (pass-through tiles included)
      pass_through        tiles with kPassThrough
      crossing_workgroup  chains whose owner and last tile lie in different workgroups
      through_workgroup   chains that pass through a whole workgroup (owner and last tile two or more workgroups apart)
      longest_chain       tiles of the longest chain (1 when no run crosses an edge, 0 without runs)
      ends_on_edge        runs that end exactly on a tile edge (the next run, or the gated tail, starts a tile)
      start_phases        distinct offsets of a run's start within its tile
      gated_on_edge       1 when the gated tail exists and starts exactly on a tile edge
      gated_beside_edge   1 when it starts one slot before or after a tile edge
      tiles, workgroups   of the whole job"""
    out = dict(inside=0, owns_last=0, first_continues=0, pass_through=0, crossing_workgroup=0, through_workgroup=0, longest_chain=0,
               ends_on_edge=0, start_phases=0, gated_on_edge=0, gated_beside_edge=0)
    phases = set()
    s = 0
    for n in run_lengths:
        assert n >= 1
        e = s + n
        ft, lt = s // tile, (e - 1) // tile
        phases.add(s % tile)
        out["ends_on_edge"] += e % tile == 0
        out["longest_chain"] = max(out["longest_chain"], lt - ft + 1)
        if ft == lt:
            out["inside"] += 1
        else:
            out["owns_last"] += 1
            out["pass_through"] += lt - ft - 1
            out["first_continues"] += lt - ft
            out["crossing_workgroup"] += ft // lanes != lt // lanes
            out["through_workgroup"] += lt // lanes - ft // lanes >= 2
        s = e
    out["start_phases"] = len(phases)
    if gated > 0:
        out["gated_on_edge"] = int(s % tile == 0)
        out["gated_beside_edge"] = int(s % tile in (1, tile - 1))
    total = s + gated
    out["tiles"] = (total + tile - 1) // tile
    out["workgroups"] = (out["tiles"] + lanes - 1) // lanes
    return {k: int(v) for k, v in out.items()}


def run_lengths_of(idx, n_t):
    """(slots per target that has any, in target order; gated slots) of correspondences idx [n_s, K]"""
    idx = np.asarray(idx)
    counts = np.bincount(idx[idx >= 0], minlength=n_t)
    return counts[counts > 0], int((idx < 0).sum())


# ---- crafted pairs ----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name T K L g claims")


def _case(T, K, L, g=0, **claims):
    return Case(f"T{T}_K{K}_L{L}_g{g}", T, K, L, g, claims)


def _ge(v):
    return ("ge", v)


# claims: key of tile_geometry -> exact value, or ("ge", v)
GEOMETRY_CASES = [
    # K = 1, 37 runs: inside a tile, on a tile edge, every phase of a tile, chains of 2, 3 and 9 tiles, two workgroups
    _case(37, 1, 1, inside=37, owns_last=0, start_phases=8),
    _case(37, 1, 2, inside=37, owns_last=0),
    _case(37, 1, 7, owns_last=_ge(20), inside=_ge(4), longest_chain=2, start_phases=8),
    _case(37, 1, 8, inside=37, owns_last=0, ends_on_edge=37),
    _case(37, 1, 9, inside=0, owns_last=37, longest_chain=2, start_phases=8, pass_through=0),
    _case(37, 1, 15, owns_last=37, longest_chain=3, pass_through=_ge(20), start_phases=8),
    _case(37, 1, 16, owns_last=37, longest_chain=2, pass_through=0, ends_on_edge=37),
    _case(37, 1, 17, owns_last=37, longest_chain=3, pass_through=37, start_phases=8),
    _case(37, 1, 63, owns_last=37, longest_chain=9, start_phases=8, workgroups=2, crossing_workgroup=1),
    _case(37, 1, 64, owns_last=37, longest_chain=8, ends_on_edge=37, workgroups=2, crossing_workgroup=0),
    _case(37, 1, 65, owns_last=37, longest_chain=9, start_phases=8, workgroups=2, crossing_workgroup=1),
    # runs that end before, on and after a workgroup edge; owner chains of 256 tiles and more
    _case(3, 1, 2047, owns_last=3, longest_chain=257, crossing_workgroup=2, workgroups=3),
    _case(3, 1, 2048, owns_last=3, longest_chain=256, crossing_workgroup=0, ends_on_edge=3, workgroups=3),
    _case(3, 1, 2049, owns_last=3, longest_chain=257, crossing_workgroup=3, workgroups=4),
    # a list that passes through a whole workgroup
    _case(2, 1, 4104, owns_last=2, longest_chain=513, through_workgroup=2, ends_on_edge=2, workgroups=5),
    # K = 4 and K = 20: T K runs, a source point's slots K runs apart
    _case(37, 4, 7, owns_last=_ge(80), longest_chain=2, start_phases=8),
    _case(37, 4, 8, inside=148, owns_last=0, ends_on_edge=148),
    _case(37, 4, 9, owns_last=148, longest_chain=2, start_phases=8, workgroups=1),
    _case(37, 20, 7, owns_last=_ge(400), longest_chain=2, start_phases=8, workgroups=3),
    _case(37, 20, 8, inside=740, owns_last=0, workgroups=3),
    _case(37, 20, 9, owns_last=740, longest_chain=2, start_phases=8, workgroups=4, crossing_workgroup=_ge(1)),
    # the gated tail on a tile edge (L = 8: 296 live slots) and inside a tile (L = 9: 333)
    _case(37, 1, 8, 1, gated_on_edge=1, tiles=38),
    _case(37, 1, 8, 7, gated_on_edge=1, tiles=38),
    _case(37, 1, 8, 8, gated_on_edge=1, tiles=38),
    _case(37, 1, 8, 9, gated_on_edge=1, tiles=39),
    _case(37, 1, 9, 1, gated_on_edge=0, tiles=42),
    _case(37, 1, 9, 7, gated_on_edge=0, tiles=43),
    _case(37, 1, 9, 8, gated_on_edge=0, tiles=43),
    _case(37, 1, 9, 9, gated_on_edge=0, tiles=43),
    # ... and beside one: 33 x 9 = 297 live slots (one past an edge), 39 x 9 = 351 (one before); K = 4 with a gated tail
    _case(33, 1, 9, 1, gated_beside_edge=1),
    _case(33, 1, 9, 8, gated_beside_edge=1),
    _case(39, 1, 9, 1, gated_beside_edge=1, tiles=44),
    _case(39, 1, 9, 8, gated_beside_edge=1),
    _case(37, 4, 8, 1, gated_on_edge=1, inside=148),
    _case(37, 20, 9, 7, owns_last=740),
    # n_t = 2^6 (the key's sentinel is n_t itself), and n_s K = 2048 = 2^11 exactly (the slot field is full, the tiles
    # fill one workgroup exactly), with n_t = 2^8 and with n_t = 2^6
    _case(64, 1, 9, owns_last=64, workgroups=1),
    _case(64, 4, 8, inside=256, tiles=256, workgroups=1),
    _case(64, 1, 32, owns_last=64, longest_chain=4, tiles=256, workgroups=1),
    # ... and the same two with a gated tail: the sentinel 64 needs a bit more than the targets 0 .. 63 do, and the gated
    # slots' numbers reach 2047 (63 x 8 + 8 = 512 source points at K = 4)
    _case(64, 1, 9, 3, owns_last=64, gated_on_edge=1, tiles=73),
    _case(63, 4, 8, 8, inside=252, gated_on_edge=1, tiles=256, workgroups=1),
]
GEOMETRY = {c.name: c for c in GEOMETRY_CASES}
assert len(GEOMETRY) == len(GEOMETRY_CASES)

# the source kernel's last column: pose_cov_blocks(n_s) = 1, 1, 1, 2, 3 with the last workgroup 20, 255, 256, 1 and 1 lanes full
SOURCE_SIZES = (20, 255, 256, 257, 513)


def holds(claim, value):
    return value >= claim[1] if isinstance(claim, tuple) else value == claim


def check_claims(case, geo):
    bad = {k: (v, geo[k]) for k, v in case.claims.items() if not holds(v, geo[k])}
    assert not bad, (case.name, bad)


def slots_of_case(case):
    """(n_s, n_t, live slots, gated slots)"""
    n_s = case.T * case.L + case.g
    return n_s, case.T * case.K, case.T * case.L * case.K, case.g * case.K


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def crafted_pair(T, K, L, g, seed=71):
    """(src, source labels, tgt, target labels), float32 / uint32, the source in a seeded random order (a run's slots are
    then no block of consecutive slot numbers)"""
    rng = np.random.default_rng([seed, T, K, L, g])
    side = int(np.ceil(np.sqrt(T) - 1e-9))
    assert side * SPACING < 1000.0
    cells = np.stack(np.unravel_index(np.arange(T), (side, side)) + (np.zeros(T, dtype=int),), 1).astype(np.float64)
    centres = 50.0 + SPACING * cells
    centres[:, 2] = 0.0

    def jitter(n, xy):
        return rng.uniform(-1.0, 1.0, (n, 3)) * (xy, xy, FLAT)

    tgt = np.repeat(centres, K, axis=0) + jitter(T * K, 0.15)
    near = np.repeat(centres, L, axis=0) + jitter(T * L, 0.05)
    far = centres[rng.integers(0, T, g)] + (0.5 * SPACING, 0.5 * SPACING, 0.0) + jitter(g, 1.0)
    src = np.concatenate([near, far])[rng.permutation(T * L + g)]
    src, tgt = np.ascontiguousarray(src, dtype=np.float32), np.ascontiguousarray(tgt, dtype=np.float32)
    return _frozen(src, np.ones(len(src), dtype=np.uint32), tgt, np.ones(len(tgt), dtype=np.uint32))


def case_pair(case):
    return crafted_pair(case.T, case.K, case.L, case.g)


def source_pair(n_s):
    """the first n_s source points of the accumulate tests' mid-size lidar pair (3000 target points) and its true pose"""
    return A.mid_pair(n_s)


# ---- the bar ------------------------------------------------------------------------------------------------------------------------------
def rotation(qt):
    x, y, z, w = np.asarray(qt, dtype=np.float64)[:4]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def reference(qt, src, sn, tgt, tn, idx, w, eps, use_sqloss, cauchy_a, weights_always=False):
    """((S_src, S_tgt) in float64, the restatement's own gap per sum): the gap is |float64 - longdouble| of the restatement
    on the same inputs, in units of max |diag| of the sum"""
    R, t = rotation(qt), np.asarray(qt, dtype=np.float64)[4:]
    args = (R, t, np.asarray(src, dtype=np.float64), sn, np.asarray(tgt, dtype=np.float64), tn, idx, w, eps, None, cauchy_a)
    want = ref.cross_sums(*args, use_sqloss=use_sqloss, weights_always=weights_always)
    exact = ref.cross_sums(*args, use_sqloss=use_sqloss, weights_always=weights_always, dtype=np.longdouble)
    gaps = []
    for a, b in zip(want, exact):
        scale = np.abs(np.diag(b)).max()
        gaps.append(float(np.abs(a.astype(np.longdouble) - b).max() / scale) if scale > 0 else 0.0)
    return want, gaps


def bar_of(gap):
    """the bar: |got - want|_max <= bar x max |diag(want)|"""
    return max(BAR_FLOOR, BAR_MARGIN * gap)


def distance(got, want):
    """|got - want|_max in units of max |diag(want)| (inf when want is all zero and got is not)"""
    scale = np.abs(np.diag(want)).max()
    err = np.abs(np.asarray(got) - want).max()
    if scale == 0:
        return 0.0 if err == 0 else np.inf
    return float(err / scale)


# ---- would the bar hide a lost piece? -------------------------------------------------------------------------------------------------
def lost_pieces(case, tile=TILE):
    """the distinct slot counts a run of the case has beyond its first tile edge; {L} (a whole run) where no run crosses one"""
    sizes = set()
    for r in range(case.T * case.K):
        s, e = r * case.L, (r + 1) * case.L
        edge = (s // tile + 1) * tile
        if e > edge:
            sizes.add(e - edge)
    return sorted(sizes) if sizes else [case.L]


def least_movement(qt, src, sn, tgt, tn, idx, eps, use_sqloss, cauchy_a, pieces):
    """S_tgt with the last m slots (in slot order) of ONE target's list missing, for every target and every m in `pieces`:
    the smallest |S_tgt' - S_tgt|_max / max |diag S_tgt|.  The device's target order is its own, so every target may be the
    one whose run lies at a given place."""
    R, t = rotation(qt), np.asarray(qt, dtype=np.float64)[4:]
    n_s, K = idx.shape
    ii, cc = np.nonzero(idx >= 0)          # (row-major: in slot order)
    jj = idx[ii, cc]
    _, _, _, Bq = ref.slot_terms(R, t, np.asarray(src, dtype=np.float64)[ii], sn[ii], np.asarray(tgt, dtype=np.float64)[jj], tn[jj], eps, None,
                                 cauchy_a, np.ones(len(ii)), use_sqloss)
    G = np.zeros((len(tgt), 6, 3))
    np.add.at(G, jj, Bq)
    S = np.einsum("nij,nkj->ik", G, G)
    scale = np.abs(np.diag(S)).max()
    least = np.inf
    for k in np.unique(jj):
        mine = np.nonzero(jj == k)[0]
        full = G[k] @ G[k].T
        for m in pieces:
            m = min(m, len(mine))
            Gk = G[k] - Bq[mine[len(mine) - m:]].sum(0)
            least = min(least, np.abs(Gk @ Gk.T - full).max() / scale)
    return float(least)
