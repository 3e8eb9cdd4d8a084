"""CPU tests of the sicp_segment_ground restatement (tests/ground_ref.py): against a second, deliberately naive implementation
-- per point and per cell Python loops in the order the header states, members outside a set left out of the lane sums -- on
the tiny cases; the tables against place_ref's; what the named cases are meant to hit; and the conditions the sloped street
was built to meet, by the references alone: one global plane loses the ramp, the polar grid keeps it, and only without the
ground do the objects come apart."""
import math
import struct

import numpy as np
import pytest

import cluster_ref
import ground_cases
import ground_ref
import place_ref
import plane_cases
import plane_ref

G = ground_ref


# ---- the naive twin -----------------------------------------------------------------------------------------------------------
def _ordered(z32):
    b = struct.unpack("<I", struct.pack("<f", z32))[0]
    return (~b & 0xFFFFFFFF) if b & 0x80000000 else b ^ 0x80000000


def _lane_tree_sum(terms):
    """rule 5: terms = [(j, value)] of the set's members; lane j mod 64 adds in ascending j from +0.0, six pairwise steps"""
    lanes = [0.0] * 64
    for j, v in sorted(terms):
        lanes[j % 64] = lanes[j % 64] + v
    for k in range(6):
        lanes = [lanes[l] + lanes[l ^ (1 << k)] for l in range(64)]
    return lanes[0]


def naive(xyz, labels, mask, origin, ring_edge, P):
    xyz = np.asarray(xyz, np.float32)
    n = len(xyz)
    R, S = P["n_rings"], P["n_sectors"]
    o = [0.0, 0.0, 0.0] if origin is None else [float(v) for v in origin]
    T = G.make_tables(R, S, P["min_range"], P["max_range"], ring_edge)
    e2, ch, sh = (T[k].tolist() for k in ("edge2", "cos_half", "sin_half"))
    bound = -(float(P["sensor_height"]) + float(P["max_below"]))
    d, cell, cand = [None] * n, [-1] * n, [False] * n
    n_below = 0
    for i in range(n):
        p = [float(v) for v in xyz[i]]
        if not all(math.isfinite(v) for v in p):
            continue
        dx, dy, dz = p[0] - o[0], p[1] - o[1], p[2] - o[2]
        d[i] = (dx, dy, dz)
        r2 = dx * dx + dy * dy
        if not (e2[0] <= r2 < e2[R]):
            continue
        ring = sum(1 for k in range(1, R) if r2 >= e2[k])
        lower = not (dy > 0 or (dy == 0 and dx > 0))
        xp, yp = (-dx, -dy) if lower else (dx, dy)
        sector = sum(1 for j in range(1, S // 2) if ch[j] * yp - sh[j] * xp >= 0.0) + (S // 2 if lower else 0)
        cell[i] = ring * S + sector
        ok = (mask is None or mask[i] != 0) and (labels is None or int(labels[i]) not in P["ignore"])
        cand[i] = ok and dz >= bound
        n_below += ok and not cand[i]
    out = {"ground": [0] * n, "cell": cell, "height": [float("nan")] * n, "status": [G.EMPTY] * (R * S), "n_members": [0] * (R * S),
           "n_ground": [0] * (R * S), "n_fit": [0] * (R * S), "model": {}, "lpr": {}, "lambda_min": {}, "n_below": n_below, "n_candidates": sum(cand)}
    order = sorted((i for i in range(n) if cand[i]), key=lambda i: (cell[i], _ordered(xyz[i, 2]), i))
    for c in sorted(set(cell[i] for i in order)):
        seg = [i for i in order if cell[i] == c]
        m = len(seg)
        out["n_members"][c] = m
        L = min(P["n_lpr"], m)
        s = 0.0
        for k in range(L):
            s = s + d[seg[k]][2]
        lpr = s / float(L)
        out["lpr"][c] = lpr
        ts = lpr + float(P["th_seeds"])
        cur = [j for j in range(m) if d[seg[j]][2] < ts]
        status = None
        for _ in range(P["n_iter"]):
            if len(cur) < P["min_points"]:
                status = G.TOO_FEW
                break
            cnt = float(len(cur))
            g = [_lane_tree_sum([(j, d[seg[j]][a]) for j in cur]) / cnt for a in range(3)]
            e = {j: tuple(d[seg[j]][a] - g[a] for a in range(3)) for j in range(m)}
            Q = [_lane_tree_sum([(j, e[j][a] * e[j][b]) for j in cur]) for a, b in ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))]
            u, lam = G.smallest_eigenpair(Q)
            if u[2] < 0.0:
                u = [-u[0], -u[1], -u[2]]
            n_fit = len(cur)
            cur = [j for j in range(m) if (u[0] * e[j][0] + u[1] * e[j][1]) + u[2] * e[j][2] < float(P["th_dist"])]
        if status is None:
            mt = float(P["max_thickness"])
            if not u[2] >= float(P["min_cos"]):
                status = G.NOT_UPRIGHT
            elif c // S < P["elevation_rings"] and g[2] >= -float(P["sensor_height"]) + float(P["max_elevation"]):
                status = G.TOO_HIGH
            elif mt > 0.0 and lam > (mt * mt) * float(n_fit):
                status = G.TOO_THICK
            else:
                status = G.GROUND
        out["status"][c] = status
        if status == G.GROUND:
            for j in cur:
                out["ground"][seg[j]] = 1
            out["n_ground"][c], out["n_fit"][c] = len(cur), n_fit
            out["model"][c], out["lambda_min"][c] = (u, g), lam
    for i in range(n):
        if cell[i] < 0:
            continue
        ring, sector = divmod(cell[i], S)
        for r in range(ring, -1, -1):
            if r * S + sector in out["model"]:
                u, g = out["model"][r * S + sector]
                e = [d[i][a] - g[a] for a in range(3)]
                out["height"][i] = (u[0] * e[0] + u[1] * e[1]) + u[2] * e[2]
                break
    return out


def _bits(a):
    return np.asarray(a, np.float64).tobytes()


@pytest.mark.parametrize("name", ground_cases.TINY)
def test_the_restatement_equals_the_naive_twin(name):
    c = ground_cases.case(name)
    ref = ground_cases.reference(name)
    got = naive(c["xyz"], c["labels"], c["mask"], c["origin"], c["ring_edge"], c["params"])
    o = np.zeros(3) if c["origin"] is None else c["origin"]
    assert (got["n_candidates"], got["n_below"]) == (ref["n_candidates"], ref["n_below"])
    for k in ("ground", "cell", "status", "n_members", "n_ground", "n_fit"):
        assert list(got[k]) == ref[k].tolist(), k
    assert _bits(got["height"]) == _bits(ref["height"])
    for cell in range(len(ref["status"])):
        if ref["status"][cell] == G.GROUND:
            u, g = got["model"][cell]
            assert _bits(u) == _bits(ref["normal"][cell]) and _bits([g[a] + float(o[a]) for a in range(3)]) == _bits(ref["centroid"][cell])
            assert _bits(got["lambda_min"][cell]) == _bits(ref["lambda_min"][cell])
        else:
            assert np.isnan(ref["normal"][cell]).all() and np.isnan(ref["centroid"][cell]).all() and np.isnan(ref["lambda_min"][cell])
        if ref["status"][cell] != G.EMPTY:
            assert _bits(got["lpr"][cell]) == _bits(ref["lpr"][cell])
        else:
            assert np.isnan(ref["lpr"][cell])


# ---- tables -------------------------------------------------------------------------------------------------------------------
def test_the_tables_are_the_place_tables():
    """with min_range = 0 the uniform rings and the half-plane tables are sicp_place's, bit for bit; a caller's ring table is squared
    entry by entry"""
    for R, S, mx in ((20, 60, 40.0), (16, 32, 80.0), (1, 4, 7.3), (64, 256, 123.456)):
        a, b = G.make_tables(R, S, 0.0, mx), place_ref.make_tables(R, S, mx)
        for k in ("edge2", "cos_half", "sin_half"):
            assert a[k].tobytes() == b[k].tobytes(), (R, S, k)
    t = G.make_tables(3, 6, 0.5, 30.0, ground_cases.RING_EDGE)
    assert t["edge2"].tolist() == [e * e for e in ground_cases.RING_EDGE]
    u = G.make_tables(16, 32, 2.7, 80.0)["edge2"]
    assert u[0] == 2.7 * 2.7 and (np.diff(u) > 0).all()


def test_ordered_bits_sorts_floats_and_puts_minus_zero_first():
    z = np.array([-np.inf, -3.5, -1e-30, -0.0, 0.0, 1e-30, 2.0, np.inf], np.float32)
    k = G.ordered_bits(z).astype(np.int64)
    assert (np.diff(k) > 0).all()


# ---- what the cases hit -------------------------------------------------------------------------------------------------------
def test_the_cases_hit_what_they_are_named_for():
    ref = ground_cases.reference
    r = ref("cell_sizes")
    assert sorted(v for v in r["n_members"].tolist() if v) == list(ground_cases.CELL_SIZES)
    assert sorted(r["status"][r["n_members"] > 0].tolist()) == [G.GROUND] * 7 + [G.TOO_FEW] * 3
    r, S = ref("statuses"), ground_cases.STATUS_GRID["n_sectors"]
    for (ring, sector), want in ground_cases.STATUS_CELLS.items():
        assert r["status"][ring * S + sector] == want, (ring, sector)
    assert set(r["status"].tolist()) == {0, 1, 2, 3, 4, 5}
    one = ground_cases.run_reference(ground_cases.case("statuses"), n_iter=1)  # (2, 0) fails at the second set only
    assert one["status"][1 * S + 0] == G.TOO_FEW and one["status"][2 * S + 0] == G.TOO_THICK and one["n_members"][2 * S + 0] == 12
    r = ref("th_dist_edge")
    assert r["normal"][0].tolist() == [0.0, 0.0, 1.0] and r["centroid"][0].tolist() == [6.5, 4.5, -2.0]
    assert r["ground"][-3:].tolist() == [0, 1, 0] and r["height"][-3] == 0.25
    assert ref("th_seeds_edge")["n_fit"][0] == 65
    r = ref("below_edge")
    assert r["n_below"] == 3 and r["ground"][-5] == 1 and r["cell"][-4] == 0 and r["ground"][-4] == 0
    r = ref("equal_heights")
    assert r["status"][:5].tolist() == [G.GROUND, G.TOO_HIGH, G.GROUND, G.GROUND, G.NOT_UPRIGHT]
    z = ground_cases.case("equal_heights")["xyz"][:, 2]
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any()
    r, c = ref("height_fallback"), ground_cases.case("height_fallback")
    assert r["status"][[0, 4, 8]].tolist() == [G.GROUND, G.EMPTY, G.TOO_FEW] and np.isfinite(r["height"][r["cell"] == 8]).all()
    assert r["status"][5] == G.TOO_FEW and np.isnan(r["height"][r["cell"] == 5]).all()
    assert np.isfinite(r["height"][c["mask"] == 0]).all() and not r["ground"][c["mask"] == 0].any()
    r = ref("boundaries")
    assert set(r["cell"].tolist()) == set(range(-1, 16)) and r["n_points"] - r["n_candidates"] == int((r["cell"] < 0).sum())
    r = ref("no_candidates")
    assert r["n_candidates"] == 0 and r["cells"] == [16, 0, 0, 0, 0, 0] and r["n_below"] == 100
    r = ref("grid_64x256")
    assert r["cells"][G.EMPTY] > 0.7 * 64 * 256
    r = ref("big")
    assert r["n_points"] == 262145 + 4097 and r["n_members"].max() > 4097
    assert ref("n_lpr_1")["lpr"].tobytes() != ref("n_lpr_64")["lpr"].tobytes()
    assert ref("n_iter_1")["n_ground_total"] != ref("n_iter_8")["n_ground_total"]


def test_refusals_of_the_restatement():
    c = ground_cases.case("no_labels")
    for over in (dict(n_sectors=5), dict(n_sectors=2), dict(n_rings=65), dict(n_lpr=0), dict(n_lpr=65), dict(n_iter=9), dict(min_points=2),
                 dict(min_cos=0.0), dict(th_dist=0.0), dict(th_seeds=-1.0), dict(elevation_rings=5), dict(ignore=(1,)), dict(select=3),
                 dict(min_range=-1.0), dict(max_range=1.0), dict(max_thickness=-0.1), dict(sensor_height=float("nan"))):
        with pytest.raises(ValueError):
            ground_cases.run_reference(c, **over)


# ---- the sloped street ----------------------------------------------------------------------------------------------------------
def test_the_sloped_street_needs_the_polar_grid():
    """(a) the one plane of the planes recipe recalls < 0.7 of the true ground; (b) the polar grid with its defaults reaches
    recall and precision >= 0.95; (c) with only the plane removed one component still holds more than half of what is left; with
    the ground removed the largest holds < 0.4 and there are several"""
    xyz, truth = ground_cases.sloped_street()
    assert len(xyz) == 20000
    plane = plane_ref.segment_planes(xyz, None, None, **dict(plane_ref.DEFAULTS, **plane_cases.RECIPE_PLANE))["plane_id"] == 0
    ground = ground_cases.reference("street")["ground"] != 0
    plane_recall = (plane & truth).sum() / truth.sum()
    recall, precision = (ground & truth).sum() / truth.sum(), (ground & truth).sum() / ground.sum()
    print("plane recall", plane_recall, "ground recall", recall, "precision", precision)
    assert plane_recall < 0.7
    assert recall >= 0.95 and precision >= 0.95
    a = cluster_ref.cluster(xyz[~plane], None, **plane_cases.RECIPE_CLUSTER)
    b = cluster_ref.cluster(xyz[~ground], None, **plane_cases.RECIPE_CLUSTER)
    print("plane removed:", a["n_clusters"], a["max_cluster_points"], int((~plane).sum()), "ground removed:", b["n_clusters"],
          b["max_cluster_points"], int((~ground).sum()))
    assert a["max_cluster_points"] > 0.5 * (~plane).sum()
    assert b["n_clusters"] > 1 and b["max_cluster_points"] < 0.4 * (~ground).sum()
