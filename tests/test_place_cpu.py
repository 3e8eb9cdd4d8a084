"""CPU tests of the place-recognition rules (include/sicp.h, "a database of scan descriptors"): the numpy restatement
tests/place_ref.py against closed forms and hand-stated boundary cases, the scene's condition on the inputs, and the ABI."""
import ctypes
import importlib
import math
import os
import subprocess
import textwrap

import numpy as np
import pytest

import place_cases as PC
import place_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


# ---- cells -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 60, 64, 256])
def test_sector_count_is_the_floor_of_the_azimuth(S):
    rng = np.random.default_rng(100 + S)
    n = 20000
    a = rng.uniform(-np.pi, np.pi, n)
    r = rng.uniform(0.5, 39.0, n)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], axis=1).astype(np.float32)
    T = PR.make_tables(7, S, 40.0)
    keep, ring, sector, d = PR.cells(xyz, None, T, 7, S, 0.0)
    step = 2 * np.pi / S
    az = np.arctan2(d[:, 1].astype(np.float64), d[:, 0].astype(np.float64)) % (2 * np.pi)
    frac = az / step
    far = np.abs(frac - np.round(frac)) * step >= 1e-9  # at least 1e-9 rad from every boundary
    assert far.sum() > n - 10
    assert np.array_equal(sector[far], np.floor(frac[far]).astype(np.int64) % S)
    assert sector.min() >= 0 and sector.max() < S


def test_ring_count_is_the_floor_of_the_range():
    rng = np.random.default_rng(7)
    R, max_range = 13, 37.0
    n = 20000
    xyz = np.stack([rng.uniform(-40, 40, n), rng.uniform(-40, 40, n), rng.uniform(-2, 2, n)], axis=1).astype(np.float32)
    T = PR.make_tables(R, 8, max_range)
    keep, ring, sector, d = PR.cells(xyz, None, T, R, 8, 0.0)
    rho = np.sqrt(d[:, 0].astype(np.float64) ** 2 + d[:, 1].astype(np.float64) ** 2)
    f = rho / (max_range / R)
    away = (np.abs(f - np.round(f)) > 1e-5) & (rho < max_range * (1 - 1e-6))
    assert np.array_equal(keep[away], np.ones(away.sum(), bool))
    assert np.array_equal(ring[away], np.floor(f[away]).astype(np.int64))
    assert not keep[rho > max_range * (1 + 1e-6)].any()


def test_boundary_points_fall_where_the_rules_say():
    B = PC.BOUNDARY_PARAMS
    T = PR.make_tables(B["R"], B["S"], B["max_range"])
    keep, ring, sector, _ = PR.cells(PC.boundary_xyz(), None, T, B["R"], B["S"], B["min_range"])
    for i, (p, k, r, s) in enumerate(PC.BOUNDARY_POINTS):
        assert (bool(keep[i]), int(ring[i]), int(sector[i])) == (k, r, s), p
    # the origin with min_range = 0: kept, in the last sector of ring 0
    keep, ring, sector, _ = PR.cells(np.zeros((1, 3), np.float32), None, T, B["R"], B["S"], 0.0)
    assert bool(keep[0]) and (int(ring[0]), int(sector[0])) == PC.BOUNDARY_ORIGIN_CELL
    # a sensor origin is subtracted in float
    keep, ring, sector, _ = PR.cells(np.array([[15.0, -3.0, 2.0]], np.float32), (10.0, -3.0, 0.5), T, B["R"], B["S"], B["min_range"])
    assert (bool(keep[0]), int(ring[0]), int(sector[0])) == (True, 2, 0)


# ---- voting ------------------------------------------------------------------------------------------------------------
def _one_cell(labels, z=None, **kw):
    """points in cell (ring 1, sector 0) of a 2 x 4 descriptor with 10 m rings"""
    n = len(labels)
    xyz = np.tile(np.array([[9.0, 12.0, 0.0]], np.float32), (n, 1))
    if z is not None:
        xyz[:, 2] = z
    P = PR.params(R=2, S=4, max_range=20.0, **kw)
    T = PR.make_tables(2, 4, 20.0)
    desc, info = PR.describe(xyz, np.array(labels, np.uint32), P, T)
    assert (desc != 0).sum() <= 1 and desc[1, 0] == desc.max()
    return int(desc[1, 0]), info


def test_label_votes():
    assert _one_cell([3, 5, 5, 3, 2], num_classes=6)[0] == 3            # tie 3:5 -> the smallest
    assert _one_cell([0, 0, 0, 4], num_classes=6)[0] == 4               # label 0 takes no part
    assert _one_cell([5, 5, 5, 2], num_classes=6, ignore=(5,))[0] == 2  # nor does an ignored label
    assert _one_cell([0, 0], num_classes=6)[0] == 0
    code, info = _one_cell([5, 5, 0], num_classes=6, ignore=(5,))
    assert code == 0 and info == {"n_in": 3, "n_kept": 3, "n_cells": 0}
    assert _one_cell([0, 4], num_classes=6, min_cell_points=2)[0] == 0  # one remaining point is too few
    assert _one_cell([4, 2], num_classes=6, min_cell_points=2)[0] == 2
    with pytest.raises(PR.BadLabel):
        _one_cell([1, 7], num_classes=6)


def test_height_levels_clamp():
    H = dict(channel=PR.HEIGHT, z_min=-2.0, z_step=0.5)
    assert _one_cell([0], z=[-50.0], **H)[0] == 1                  # below z_min: level 0
    assert _one_cell([0, 0], z=[-1.9, 0.3], **H)[0] == 1 + 4       # (0.3 + 2) / 0.5 = 4.6
    assert _one_cell([0], z=[-2.0 + 0.5 * 253.5], **H)[0] == 254
    assert _one_cell([0], z=[1e6], **H)[0] == 255                  # level 254 is the last
    assert _one_cell([0], z=[0.0], min_cell_points=2, **H)[0] == 0
    assert _one_cell([0, 0], z=[0.0, -5.0], min_cell_points=2, **H)[0] == 5


# ---- scoring -----------------------------------------------------------------------------------------------------------
def test_a_rolled_descriptor_scores_one_at_its_shift():
    d = PC.descriptors(3, 1, 5, 12, 4)[0]
    for k in range(12):
        q = np.roll(d, -k, axis=1)  # q[c] = d[c + k]
        s, m, e = PR.best_shift(q, d)
        assert (s, m) == (k, e) and e == (d != 0).sum()


def test_shift_and_entry_ties():
    period = np.tile(np.array([[1, 2, 0, 3]], np.uint8), (3, 4))  # period 4 in 16 sectors
    s, m, e = PR.best_shift(period, period)
    assert (s, m, e) == (0, 36, 36)
    s, m, e = PR.best_shift(np.roll(period, -2, axis=1), period)
    assert (s, m, e) == (2, 36, 36)  # 2, 6, 10 and 14 tie: the smallest
    other = PC.descriptors(4, 1, 3, 16, 3)[0]
    got = PR.query(period, [other, period, other, period], top_k=4)
    assert [c["id"] for c in got] == [1, 3, 0, 2]
    empty = np.zeros((3, 16), np.uint8)
    assert PR.best_shift(empty, empty) == (0, 0, 0)
    got = PR.query(empty, [empty, empty], top_k=5)
    assert [(c["id"], c["shift"], c["score"]) for c in got] == [(0, 0, 0.0), (1, 0, 0.0)]
    assert PR.query(empty, [empty], top_k=5, min_score=0.1) == []
    assert PR.query(period, [other, period], first=1, count=0) == []


def test_the_integer_key_orders_as_fractions_do():
    rng = np.random.default_rng(9)
    either = rng.integers(0, 16385, 10000)
    match = (rng.uniform(0, 1, 10000) * (either + 1)).astype(np.int64)
    match = np.minimum(match, either)
    either[:50] = 0
    match[:50] = 0
    keys = [PR.key30(m, e) for m, e in zip(match, either)]
    fr = [PR.fraction(m, e) for m, e in zip(match, either)]
    by_key = sorted(range(10000), key=lambda i: (-keys[i], i))
    by_fraction = sorted(range(10000), key=lambda i: (-fr[i], i))
    assert by_key == by_fraction
    assert PR.key30(16384, 16384) == 1 << 30 and PR.key30(0, 0) == 0


# ---- the scene: a condition on the inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel", [PR.LABEL, PR.HEIGHT])
def test_scene_revisits_find_their_keyframe(channel):
    sc = PC.scene()
    P = PC.scene_params(channel)
    T = PR.make_tables(P["R"], P["S"], P["max_range"])
    entries = [PR.describe(p, l, P, T)[0] for p, l in sc["entries"]]
    for (xyz, lab), (e, _, yaw) in zip(sc["queries"], sc["revisits"]):
        q = PR.describe(xyz, lab, P, T)[0]
        got = PR.query(q, entries, top_k=2)
        assert got[0]["id"] == e, (got, e)
        assert PC.cyclic_distance(got[0]["shift"], PC.expected_shift(yaw, P["S"]), P["S"]) <= 1, (got[0], yaw)
        assert got[0]["score"] > got[1]["score"]


# ---- ABI ---------------------------------------------------------------------------------------------------------------
PLACE_SYMBOLS = ["sicp_default_place_params", "sicp_place_create", "sicp_place_destroy", "sicp_place_clear", "sicp_place_size",
                 "sicp_place_last_error", "sicp_place_describe", "sicp_place_add", "sicp_place_add_descriptors", "sicp_place_get",
                 "sicp_place_query", "sicp_place_query_descriptors", "sicp_place_tables"]


def test_place_abi(tmp_path):
    lib = ctypes.CDLL(sicp.build())
    for name in PLACE_SYMBOLS:
        assert hasattr(lib, name), name
    code = textwrap.dedent(
        """
        #include <stdio.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %zu %d %d %d\\n", sizeof(sicp_place_params), sizeof(sicp_place_candidate), sizeof(sicp_place_describe_info),
                 SICP_PLACE_LABEL, SICP_PLACE_HEIGHT, SICP_PLACE_MAX_IGNORE);
          return 0;
        }
        """
    )
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    sizes = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert sizes == [ctypes.sizeof(sicp.SicpPlaceParams), ctypes.sizeof(sicp.SicpPlaceCandidate), ctypes.sizeof(sicp.SicpPlaceDescribeInfo),
                     sicp.PLACE_LABEL, sicp.PLACE_HEIGHT, sicp.PLACE_MAX_IGNORE]
    p = sicp.default_place_params()
    assert (p.n_rings, p.n_sectors, p.max_range, p.min_range, p.channel, p.num_classes) == (20, 60, 40.0, 0.0, sicp.PLACE_LABEL, 0)
    assert (p.z_min, p.z_step, p.min_cell_points, p.n_ignore) == (-2.0, 0.5, 1, 0)
    assert list(p.ignore) == [0] * sicp.PLACE_MAX_IGNORE
    q = sicp.default_place_params(num_classes=11, ignore=(3, 4))
    assert (q.num_classes, q.n_ignore, list(q.ignore)[:3]) == (11, 2, [3, 4, 0])
    assert sicp.lib().sicp_default_place_params(None) == sicp.ERR_INVALID_ARGUMENT
    qt = sicp.place_init_qt(math.pi / 3)
    assert np.allclose(qt, [0, 0, 0.5, math.sqrt(3) / 2, 0, 0, 0], atol=1e-15)
