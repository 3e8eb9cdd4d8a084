"""CPU tests of ray casting (sicp_map_raycast): the library exports it, the ctypes structs have the header's layout, the defaults
are the header's, lidar_ray_ends is ring-major, and the numpy restatement the GPU tests compare against
(tests/map_raycast_ref.py) is itself checked -- its hit is the opaque voxel a segment enters first by an independent rule in
exact rational arithmetic, it hits the hand cases' k-th voxel at start_margin = k, and the cases of the GPU tests are not
trivial ones (their counts are pinned)."""
import ctypes
import fractions
import importlib
import os
import subprocess

import numpy as np
import pytest

import map_carve_cases
import map_carve_ref
import map_cases
import map_raycast_cases as cases
import map_raycast_ref as ref
import map_ref
import merge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_raycast_params", "sicp_map_raycast")


def test_library_exports_the_raycast_entry_points():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header(tmp_path):
    probes = [
        ("sicp_map_raycast_params", sicp.SicpMapRaycastParams, ("max_range", "min_count", "start_margin", "n_ignore", "ignore")),
        ("sicp_map_raycast_info", sicp.SicpMapRaycastInfo, ("n_in", "n_rays", "n_steps", "n_hits", "n_voxels", "n_visible", "t_total_ms")),
    ]
    prints = "".join(
        f'  printf("%zu", sizeof({c}));' + "".join(f' printf(" %zu", offsetof({c}, {f}));' for f in fields) + ' printf("\\n");\n'
        for c, _, fields in probes)
    code = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sicp.h\"\nint main(void) {\n" + prints +
            '  printf("%d\\n", SICP_MAP_RAYCAST_MAX_IGNORE);\n  return 0;\n}\n')
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(rows) == len(probes) + 1
    for row, (cname, struct, fields) in zip(rows, probes):
        size, *offsets = map(int, row.split())
        assert ctypes.sizeof(struct) == size, cname
        assert [getattr(struct, f).offset for f in fields] == offsets, cname
    assert int(rows[-1]) == sicp.MAP_RAYCAST_MAX_IGNORE == ref.MAX_IGNORE


def test_default_params_are_the_headers():
    p = sicp.default_map_raycast_params()
    assert (p.max_range, p.min_count, p.start_margin, p.n_ignore, p.reserved_) == (0.0, 1, 1, 0, 0)
    assert list(p.ignore) == [0] * sicp.MAP_RAYCAST_MAX_IGNORE
    d = ref.defaults()
    assert (d["max_range"], d["min_count"], d["start_margin"], tuple(d["ignore"])) == (0.0, 1, 1, ())
    q = sicp.default_map_raycast_params(ignore=(2, 7), max_range=40.0, min_count=3, start_margin=0)
    assert (q.max_range, q.min_count, q.start_margin, q.n_ignore, list(q.ignore)[:3]) == (40.0, 3, 0, 2, [2, 7, 0])
    with pytest.raises(AttributeError):
        sicp.default_map_raycast_params(end_margin=1)
    with pytest.raises(AttributeError):
        ref.defaults(end_margin=1)
    with pytest.raises(ValueError):
        sicp.default_map_raycast_params(ignore=range(sicp.MAP_RAYCAST_MAX_IGNORE + 1))
    assert sicp.lib().sicp_default_map_raycast_params(None) == sicp.ERR_INVALID_ARGUMENT


def test_a_null_map_is_refused_not_dereferenced():
    lib = sicp.lib()
    p = sicp.default_map_raycast_params()
    info = sicp.SicpMapRaycastInfo()
    e = np.zeros(4, np.float32)
    fp = e.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    none = (None,) * 9
    assert lib.sicp_map_raycast(None, None, None, 0, None, None, None, None, None, 0, *none, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_raycast(None, None, None, 4, fp, fp, fp, ctypes.byref(p), None, 1, *none, ctypes.byref(info)) == sicp.ERR_INVALID_ARGUMENT
    assert info.n_in == 0 and info.n_voxels == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_gpu_means_loud_failure_not_fallback():
    assert callable(sicp.VoxelMap.raycast)
    with pytest.raises(sicp.SicpError) as e:
        sicp.VoxelMap(0)
    assert e.value.status == sicp.ERR_NO_DEVICE


def test_lidar_ray_ends_are_ring_major_and_max_range_long():
    o = np.array([0.5, -1.0, 2.0])
    ends = sicp.lidar_ray_ends(5, 8, -30.0, 10.0, 20.0, origin=o)
    assert ends.dtype == np.float32 and ends.shape == (40, 3) and ends.flags.c_contiguous
    d = ends.astype(np.float64) - o
    assert np.allclose(np.linalg.norm(d, axis=1), 20.0, atol=1e-4)
    elev = np.degrees(np.arcsin(d[:, 2] / 20.0)).reshape(5, 8)
    assert np.allclose(elev, np.linspace(-30, 10, 5)[:, None], atol=1e-4)  # a ring is a run of n_azimuth consecutive rays
    azim = np.degrees(np.arctan2(d[:, 1], d[:, 0])).reshape(5, 8) % 360.0
    assert np.allclose(azim, np.arange(8) * 45.0, atol=1e-3)
    assert np.array_equal(sicp.lidar_ray_ends(1, 1, 0.0, 0.0, 2.0), np.array([[2.0, 0.0, 0.0]], np.float32))
    with pytest.raises(ValueError):
        sicp.lidar_ray_ends(0, 8, -1.0, 1.0, 2.0)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _coords(key):
    B = map_ref.BIAS
    return int(key & 0x1fffff) - B, int((key >> 21) & 0x1fffff) - B, int((key >> 42) & 0x1fffff) - B


def _entry(o, p, inv, v):
    """the exact parameter t at which the segment from o to p enters the open box of voxel v (a voxel of segment_voxels)"""
    F = fractions.Fraction
    t_in = F(0)
    for a in range(3):
        u, w = F(float(o[a])) * F(float(inv)), F(float(p[a])) * F(float(inv))
        if w != u:
            t_in = max(t_in, min((v[a] - u) / (w - u), (v[a] + 1 - u) / (w - u)))
    return t_in


def test_the_hit_is_the_opaque_voxel_the_segment_enters_first():
    """seeded rays in general position on sparse maps: the restatement's hit lies on the segment by the exact rule, and no opaque
    voxel the segment meets is entered strictly earlier (equal entry parameters are left out); a ray without a hit meets no
    opaque voxel at all.  start_margin = 0, so the rule has no exception; min_count = 2 makes part of the map transparent."""
    rays = hits = transparent_passed = 0
    for leaf, origins, returns in map_carve_cases.general_rays():
        half = float(np.abs(np.concatenate([origins, returns])).max())
        rng = np.random.default_rng(7)
        pts = rng.uniform(-half, half, (int(0.6 * (2 * half / leaf) ** 3), 3)).astype(np.float32)
        m = map_ref.Map(leaf, 0)
        m.integrate(pts)
        P = ref.defaults(start_margin=0, min_count=2)
        opaque = {_coords(k) for k in m.key[ref.opaque_rows(m, P)]}
        held = {_coords(k) for k in m.key}
        assert 20 < len(opaque) < len(held)
        inv = map_carve_ref.inv_leaf(leaf)
        for g in range(len(origins)):
            out = ref.raycast(m, returns[g][None], None, origins[g], P)
            seg = map_carve_ref.segment_voxels(origins[g], returns[g], inv)
            rays += 1
            assert out["length"][0] >= 0
            if out["row"][0] < 0:
                assert not (seg & opaque)
                continue
            hits += 1
            v = _coords(m.key[out["row"][0]])
            assert v in seg and v in opaque
            t_hit = _entry(origins[g], returns[g], inv, v)
            assert all(_entry(origins[g], returns[g], inv, c) >= t_hit for c in seg & opaque)
            transparent_passed += any(_entry(origins[g], returns[g], inv, c) < t_hit for c in seg & (held - opaque))
    print(f"{rays} rays, {hits} hits, {transparent_passed} of them behind a transparent voxel of the map")
    assert rays == 400 and hits >= 100 and rays - hits >= 20 and transparent_passed >= 20


def _box():
    m = map_ref.Map(map_carve_cases.LEAF, map_carve_cases.CLASSES)
    m.integrate(*map_carve_cases.box_map())
    return m


@pytest.fixture(scope="module")
def box():
    return _box()


@pytest.mark.parametrize("name", sorted(map_carve_cases.HAND))
def test_hand_cases(box, name):
    """every voxel of the box map is occupied: with start_margin = k the hit is the walk's k-th voxel, written out by hand"""
    o, p, _, want = map_carve_cases.HAND[name]
    end = np.asarray(p, np.float32)[None]
    n = len(want) - 1
    for k in range(n + 2):
        out = ref.raycast(box, end, None, o, ref.defaults(start_margin=k))
        assert out["length"][0] == n and out["info"]["n_rays"] == 1
        if k <= n:
            assert out["step"][0] == k and _coords(box.key[out["row"][0]]) == want[k], (name, k)
            assert out["info"]["n_steps"] == 1 and out["info"]["n_hits"] == 1 and out["info"]["n_visible"] == 1
            assert out["xyz"][0].tobytes() == box.centroids()[out["row"][0]].tobytes() and out["count"][0] == 1
            assert out["labels"][0] == np.argmax(box.hist[out["row"][0]]) and out["range_sq"][0] >= 0.0
        else:
            assert (out["row"][0], out["step"][0], out["range_sq"][0]) == (-1, -1, -1.0) and out["info"]["n_steps"] == 0
            assert not out["xyz"].any() and out["labels"][0] == 0 and out["count"][0] == 0


def test_zero_length_hits_v0_at_margin_0_and_nothing_at_1(box):
    o, p, _, want = map_carve_cases.HAND["zero_length"]
    assert want == [(0, 0, 0)]
    end = np.asarray(p, np.float32)[None]
    at0 = ref.raycast(box, end, None, o, ref.defaults(start_margin=0))
    assert at0["step"][0] == 0 and at0["length"][0] == 0 and _coords(box.key[at0["row"][0]]) == (0, 0, 0)
    at1 = ref.raycast(box, end, None, o)
    assert at1["row"][0] == -1 and at1["length"][0] == 0 and at1["info"] == dict(n_in=1, n_rays=1, n_steps=0, n_hits=0, n_voxels=len(box.key), n_visible=0)


def test_ends_that_cast_no_ray_keep_their_index():
    """NaN and infinite ends, and one beyond the key's range: length -1 at their own index, the others unmoved"""
    ends = cases.sparse_ends()[:50].copy()
    ends[3, 1] = np.nan
    ends[17, 0] = np.inf
    ends[30] = (3e6, 0.0, 0.0)
    m = cases.sparse_map()
    out = ref.raycast(m, ends, None, cases.ORIGIN)
    full = cases.parity_reference("defaults")
    bad = np.zeros(50, bool)
    bad[[3, 17, 30]] = True
    assert (out["length"][bad] == -1).all() and (out["row"][bad] == -1).all() and (out["range_sq"][bad] == -1.0).all()
    for k in ref.ARRAYS:
        assert np.array_equal(out[k][~bad], full[k][:50][~bad]), k
    assert out["info"]["n_in"] == 50 and out["info"]["n_rays"] == 47


# ---- the cases of the GPU tests --------------------------------------------------------------------------------------------------
PINNED = {  # name: (rays cast, with a hit, voxels tested, distinct rows hit)
    "defaults": (1500, 953, 16428, 209),
    "margin0": (1500, 953, 17928, 209),
    "margin3": (1500, 936, 13648, 210),
    "min_count2": (1500, 32, 27124, 12),
    "min_count2_two_scans": (1500, 150, 25925, 39),
    "ignore": (1500, 562, 22122, 156),
    "ignore_bin0_range": (61, 18, 313, 9),
    "ignore_bin0_range_two_scans": (61, 28, 284, 13),
    "range4": (220, 92, 1609, 39),
}


def test_the_sparse_map_is_sparse():
    assert len(cases.sparse_map().key) == 780 and len(cases.sparse_map(2).key) == 1516
    assert int((cases.sparse_map(2).cnt >= 2).sum()) >= 40
    assert sorted(PINNED) == sorted(cases.PARITY)


@pytest.mark.parametrize("name", sorted(cases.PARITY))
def test_parity_cases_have_hits_and_misses(name):
    """the condition on a parity case: at least 20 rays with a hit and at least 20 cast rays without one"""
    out = cases.parity_reference(name)
    i = out["info"]
    cast_without = int(((out["row"] < 0) & (out["length"] >= 0)).sum())
    print(name, i, cast_without)
    assert (i["n_rays"], i["n_hits"], i["n_steps"], i["n_visible"]) == PINNED[name]
    assert i["n_hits"] + cast_without == i["n_rays"] and i["n_in"] == 1500
    if name in cases.BELOW_CONDITION:
        assert name + "_two_scans" in cases.PARITY  # (18 hits on the one-scan map: its twin carries the condition)
    else:
        assert i["n_hits"] >= 20 and cast_without >= 20


def test_the_dense_map_would_not_do():
    """on map_cases.four() every ray of map_carve_cases.fifth() hits within a step or two: that map cannot test a ray cast"""
    out = ref.raycast(map_carve_cases.four_map(), map_carve_cases.fifth()[0], None, cases.ORIGIN)
    assert out["info"]["n_hits"] == 1500 and int(out["step"].max()) <= 2 and out["info"]["n_visible"] < 10


def test_the_scene_sees_the_car_or_through_it():
    CAR = map_carve_cases.CAR
    seen = cases.scene_reference()
    through = cases.scene_reference((CAR,))
    assert seen["info"]["n_rays"] == through["info"]["n_rays"] == 2880
    on_car = (seen["row"] >= 0) & (seen["labels"] == CAR)
    assert seen["info"]["n_hits"] > 1000 and int(on_car.sum()) >= 50
    assert through["info"]["n_hits"] == seen["info"]["n_hits"] and not (through["labels"][through["row"] >= 0] == CAR).any()
    # every ray that met the car now ends on ground or wall, further away; the others are unchanged
    assert (through["row"][on_car] >= 0).all()
    assert set(np.unique(through["labels"][on_car])) <= {map_carve_cases.GROUND, map_carve_cases.WALL}
    assert (through["step"][on_car] > seen["step"][on_car]).all() and (through["range_sq"][on_car] > seen["range_sq"][on_car]).all()
    for k in ref.ARRAYS:
        assert np.array_equal(through[k][~on_car], seen[k][~on_car]), k


def test_scan_points_that_the_map_contradicts():
    """scan 3's own points as ends against the map of scans 1 - 2: the rays that meet a CAR voxel before their end are the
    returns from behind where the car stood"""
    CAR = map_carve_cases.CAR
    scan3 = map_carve_cases.scene()["scans"][2][0]
    out = ref.raycast(map_carve_cases.scene_map(), scan3, None, map_carve_cases.SENSOR)
    blocked = (out["row"] >= 0) & (out["labels"] == CAR) & (out["step"] < out["length"])
    assert 0 < int(blocked.sum()) < len(scan3) // 4
    assert (scan3[blocked][:, 0] > 3.0).all() and (np.abs(scan3[blocked][:, 1]) < 2.5).all()  # behind the box [2, 3] x [-0.5, 0.5]


def test_refusals_of_the_restatement():
    m = cases.sparse_map()
    ends = cases.sparse_ends()[:10]
    for bad in (dict(min_count=0), dict(start_margin=-1), dict(max_range=-1.0), dict(max_range=float("nan")),
                dict(ignore=(cases.CLASSES + 1,)), dict(ignore=range(65))):
        with pytest.raises(ValueError):
            ref.raycast(m, ends, None, None, ref.defaults(**bad))
    with pytest.raises(merge_ref.GridOverflow):
        ref.raycast(m, ends, None, (1e6, 0.0, 0.0))
    with pytest.raises(ValueError):
        ref.raycast(map_ref.Map(cases.LEAF, 0), ends, None, None, ref.defaults(ignore=(1,)))
    assert ref.raycast(m, ends, None, None, ref.defaults(max_range=float("inf")))["info"]["n_rays"] == 10
