"""CPU tests of free-space carving (sicp_map_carve): the library exports it, the ctypes structs have the header's layout, there
is no fallback without a device, and the numpy restatement the GPU tests compare against (tests/map_carve_ref.py) is itself
checked -- its walk visits exactly the voxels a segment meets by an independent rule in exact rational arithmetic, it walks
the hand cases as worked out by hand, and on a scene with a car that drove off it removes the car and keeps wall and ground."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import map_carve_cases as cases
import map_carve_ref as ref
import map_ref
import merge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_carve_params", "sicp_map_carve")


def test_library_exports_the_carve_entry_points():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header(tmp_path):
    probes = [
        ("sicp_map_carve_params", sicp.SicpMapCarveParams, ("max_range", "min_rays", "end_margin", "dry_run", "n_protect", "protect")),
        ("sicp_map_carve_info", sicp.SicpMapCarveInfo, ("n_in", "n_rays", "n_steps", "n_voxels", "n_touched", "n_hit", "n_removed",
                                                        "n_spared_hit", "n_spared_label", "t_total_ms")),
    ]
    prints = "".join(
        f'  printf("%zu", sizeof({c}));' + "".join(f' printf(" %zu", offsetof({c}, {f}));' for f in fields) + ' printf("\\n");\n'
        for c, _, fields in probes)
    code = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sicp.h\"\nint main(void) {\n" + prints +
            '  printf("%d\\n", SICP_MAP_MAX_PROTECT);\n  return 0;\n}\n')
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
    assert int(rows[-1]) == sicp.MAP_MAX_PROTECT == ref.MAX_PROTECT


def test_defaults_and_unknown_overrides():
    p = sicp.default_map_carve_params()
    assert (p.max_range, p.min_rays, p.end_margin, p.dry_run, p.n_protect) == (0.0, 3, 1, 0, 0)
    assert list(p.protect) == [0] * sicp.MAP_MAX_PROTECT
    d = ref.defaults()
    assert (d["max_range"], d["min_rays"], d["end_margin"], d["dry_run"], tuple(d["protect"])) == (0.0, 3, 1, 0, ())
    q = sicp.default_map_carve_params(max_range=40.0, min_rays=5, end_margin=0, dry_run=1, protect=(2, 7))
    assert (q.max_range, q.min_rays, q.end_margin, q.dry_run, q.n_protect, list(q.protect)[:3]) == (40.0, 5, 0, 1, 2, [2, 7, 0])
    with pytest.raises(AttributeError):
        sicp.default_map_carve_params(crop_range=3.0)
    with pytest.raises(AttributeError):
        ref.defaults(crop_range=3.0)
    with pytest.raises(ValueError):
        sicp.default_map_carve_params(protect=range(sicp.MAP_MAX_PROTECT + 1))
    assert sicp.lib().sicp_default_map_carve_params(None) == sicp.ERR_INVALID_ARGUMENT


def test_a_null_map_is_refused_not_dereferenced():
    lib = sicp.lib()
    p = sicp.default_map_carve_params()
    info = sicp.SicpMapCarveInfo()
    assert lib.sicp_map_carve(None, None, 0, None, None, None, 0, None, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_carve(None, None, 0, None, None, ctypes.byref(p), 0, None, ctypes.byref(info)) == sicp.ERR_INVALID_ARGUMENT
    assert info.n_in == 0 and info.n_voxels == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_gpu_means_loud_failure_not_fallback():
    assert callable(sicp.VoxelMap.carve)
    with pytest.raises(sicp.SicpError) as e:
        sicp.VoxelMap(0)
    assert e.value.status == sicp.ERR_NO_DEVICE


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_the_walk_visits_the_voxels_the_segment_meets():
    """seeded rays in general position: the walk's voxels are exactly those whose open box the segment meets, and consecutive
    ones share a face.  The condition is zero mismatches."""
    mismatches, rays, longest = 0, 0, 0
    for leaf, origins, returns in cases.general_rays():
        inv = ref.inv_leaf(leaf)
        vo, ok_o = ref.voxels_of(origins, leaf)
        vp, ok_p = ref.voxels_of(returns, leaf)
        assert ok_o.all() and ok_p.all()
        for g in range(len(origins)):
            cells = ref.walk(origins[g], returns[g], vo[g], vp[g], inv)
            assert cells[0] == tuple(vo[g]) and cells[-1] == tuple(vp[g]) and len(set(cells)) == len(cells)
            assert all(sum(abs(a - b) for a, b in zip(c, d)) == 1 for c, d in zip(cells, cells[1:]))
            mismatches += set(cells) != ref.segment_voxels(origins[g], returns[g], inv)
            rays += 1
            longest = max(longest, len(cells) - 1)
    print(f"{rays} rays, the longest {longest} steps, {mismatches} mismatches")
    assert rays == 400 and longest >= 15
    assert mismatches == 0


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_cases(name):
    o, p, end_margin, want = cases.HAND[name]
    o32, p32 = np.asarray(o, np.float32), np.asarray(p, np.float32)
    vo, _ = ref.voxels_of(o32[None], cases.LEAF)
    vp, _ = ref.voxels_of(p32[None], cases.LEAF)
    assert ref.walk(o32, p32, vo[0], vp[0], ref.inv_leaf(cases.LEAF)) == want
    # through carve: on the box map the candidates are the voxels with miss = 1
    m = map_ref.Map(cases.LEAF, cases.CLASSES)
    m.integrate(*cases.box_map())
    out = ref.carve(m, p32[None], None, o, ref.defaults(min_rays=1, end_margin=end_margin, dry_run=1))
    n = len(want) - 1
    cand = want[:max(n - end_margin, 0)]
    assert cases.visited_on_box(m, out["miss"]) == set(cand) and int(out["miss"].sum()) == len(cand)
    assert out["info"]["n_rays"] == 1 and out["info"]["n_steps"] == len(cand) and out["info"]["n_hit"] == 1
    assert out["info"]["n_voxels"] == len(m.key) == (2 * cases.BOX + 1) ** 3  # a dry run


def test_parity_map_is_crossed_by_the_fifth_scan():
    """the GPU parity case is not a trivial one: more than half the rows are touched, some are hit, protect and the range test bite"""
    xyz, _ = cases.fifth()
    m = cases.four_map()
    assert len(m.key) == 1676
    base = ref.carve(m, xyz, None, cases.ORIGIN, ref.defaults(dry_run=1))["info"]
    assert base["n_rays"] == base["n_in"] == 1500 and base["n_touched"] > len(m.key) // 2 and 300 < base["n_hit"] < 1500
    assert base["n_removed"] > 100 and base["n_spared_hit"] > 50 and base["n_spared_label"] == 0 and base["n_voxels"] == 1676
    prot = ref.carve(m, xyz, None, cases.ORIGIN, ref.defaults(dry_run=1, protect=(1, 3)))["info"]
    assert 0 < prot["n_spared_label"] < base["n_removed"] and prot["n_removed"] + prot["n_spared_label"] == base["n_removed"]
    near = ref.carve(m, xyz, None, cases.ORIGIN, ref.defaults(dry_run=1, max_range=2.5))["info"]
    assert 0 < near["n_rays"] < 1500 and near["n_hit"] == base["n_hit"] and near["n_steps"] < base["n_steps"]
    out = ref.carve(m, xyz, None, cases.ORIGIN)
    assert out["info"]["n_voxels"] == 1676 - base["n_removed"] == len(m.key) and (np.diff(m.key) > 0).all()


def test_refusals_of_the_restatement_change_nothing():
    xyz, _ = cases.fifth()
    m = cases.four_map()
    before = m.extract()
    for bad in (dict(min_rays=0), dict(end_margin=-1), dict(dry_run=2), dict(max_range=-1.0), dict(max_range=float("nan")),
                dict(protect=(cases.CLASSES + 1,)), dict(protect=range(65))):
        with pytest.raises(ValueError):
            ref.carve(m, xyz, None, None, ref.defaults(**bad))
    with pytest.raises(merge_ref.GridOverflow):
        ref.carve(m, xyz, None, (1e6, 0.0, 0.0))
    with pytest.raises(ValueError):
        ref.carve(map_ref.Map(cases.LEAF, 0), xyz, None, None, ref.defaults(protect=(1,)))
    after = m.extract()
    assert after["xyz"].tobytes() == before["xyz"].tobytes() and after["hist"].tobytes() == before["hist"].tobytes()


def test_the_car_that_drove_off_goes_and_wall_and_ground_stay():
    s = cases.scene()
    scan3 = s["scans"][2][0]
    car = s["car_voxels"]
    assert len(car) >= 8

    def voxel_set(m, rows=None):
        k = m.key if rows is None else m.key[rows]
        B = map_ref.BIAS
        return {(int(a & 0x1fffff) - B, int((a >> 21) & 0x1fffff) - B, int((a >> 42) & 0x1fffff) - B) for a in k}

    m = cases.scene_map()
    labels = ref.fullest_bin(m.hist)
    rows_before = voxel_set(m)
    assert car <= rows_before
    # with wall and ground protected only the car goes
    dry = ref.carve(m, scan3, None, cases.SENSOR, ref.defaults(dry_run=1, protect=(cases.GROUND, cases.WALL)))
    assert voxel_set(m) == rows_before
    out = ref.carve(m, scan3, None, cases.SENSOR, ref.defaults(protect=(cases.GROUND, cases.WALL)))
    assert out["info"] == dict(dry["info"], n_voxels=len(m.key)) and np.array_equal(out["miss"], dry["miss"])
    gone = rows_before - voxel_set(m)
    assert gone == car, (sorted(car - gone), sorted(gone - car))
    assert out["info"]["n_removed"] == len(car) and out["info"]["n_spared_hit"] > 0 and out["info"]["n_spared_label"] > 0
    assert (ref.fullest_bin(m.hist) != cases.CAR).all() and (labels == cases.CAR).sum() == len(car)
    # without protect the unseen ground strip that the low wall rays graze goes too: the hit rule alone keeps the rest
    m2 = cases.scene_map()
    out2 = ref.carve(m2, scan3, None, cases.SENSOR)
    gone2 = rows_before - voxel_set(m2)
    assert car < gone2 and all(v[2] == 0 for v in gone2 - car)
    assert out2["info"]["n_spared_label"] == 0 and out2["info"]["n_removed"] == len(gone2)
    assert (ref.fullest_bin(m2.hist) == cases.WALL).sum() == (labels == cases.WALL).sum()
    # min_rays above the car's ray count: nothing goes
    car_rows = labels == cases.CAR
    assert int(dry["miss"][car_rows].min()) >= 3
    m3 = cases.scene_map()
    out3 = ref.carve(m3, scan3, None, cases.SENSOR, ref.defaults(min_rays=int(dry["miss"][car_rows].max()) + 1,
                                                                  protect=(cases.GROUND, cases.WALL)))
    assert out3["info"]["n_removed"] == 0 and voxel_set(m3) == rows_before
