"""CPU tests of sicp_map_merge and the map's state calls: the library exports them, the ctypes structs have the header's layout,
NULL maps are refused, and the numpy restatement the GPU tests compare against (tests/map_merge_ref.py) is itself checked -- it
equals the slow row-by-row restatement byte for byte on every case, the identity merge into an empty map reproduces src, every
merged row's own float centroid keys to its row, the fold's order shows in the bytes of the long run, and the exact scene equals
direct integration in map_ref."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import map_cases
import map_merge_cases as cases
import map_merge_ref as ref
import map_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_merge_params", "sicp_map_merge", "sicp_map_get_state", "sicp_map_set_state")


def test_library_exports_the_new_entry_points():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header(tmp_path):
    probes = [
        ("sicp_map_merge_params", sicp.SicpMapMergeParams, ("min_count", "crop_center", "crop_range")),
        ("sicp_map_merge_info", sicp.SicpMapMergeInfo, ("n_src_rows", "n_kept_rows", "n_kept_points", "n_touched", "n_new_voxels", "max_run",
                                                        "n_voxels", "t_total_ms")),
    ]
    prints = "".join(
        f'  printf("%zu", sizeof({c}));' + "".join(f' printf(" %zu", offsetof({c}, {f}));' for f in fields) + ' printf("\\n");\n'
        for c, _, fields in probes)
    code = "#include <stdio.h>\n#include <stddef.h>\n#include \"sicp.h\"\nint main(void) {\n" + prints + "  return 0;\n}\n"
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    rows = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(rows) == len(probes)
    for row, (cname, struct, fields) in zip(rows, probes):
        size, *offsets = map(int, row.split())
        assert ctypes.sizeof(struct) == size, cname
        assert [getattr(struct, f).offset for f in fields] == offsets, cname


def test_null_maps_are_refused_not_dereferenced():
    lib = sicp.lib()
    assert lib.sicp_map_merge(None, None, None, None, None) == sicp.ERR_INVALID_ARGUMENT
    n = ctypes.c_int64(-1)
    assert lib.sicp_map_get_state(None, 0, None, None, None, None, ctypes.byref(n)) == sicp.ERR_INVALID_ARGUMENT and n.value == -1
    assert lib.sicp_map_set_state(None, 0, None, None, None, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_default_map_merge_params(None) == sicp.ERR_INVALID_ARGUMENT


def test_defaults_and_unknown_overrides():
    p = sicp.default_map_merge_params()
    assert (p.min_count, list(p.crop_center), p.crop_range) == (1, [0.0, 0.0, 0.0], 0.0)
    q = sicp.default_map_merge_params(min_count=3, crop_center=(1, 2, 3), crop_range=40.0)
    assert (q.min_count, list(q.crop_center), q.crop_range) == (3, [1.0, 2.0, 3.0], 40.0)
    with pytest.raises(AttributeError):
        sicp.default_map_merge_params(leaf_size=0.1)
    assert set(sicp.SicpMapMergeInfo().as_dict()) == set(ref.INFO_KEYS) | {"t_total_ms"}


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.ALL)
def test_restatement_equals_the_slow_one(name):
    src, dst, kw = cases.case(name)
    slow = ref.merge_slow(dst, src, **kw)
    got, info = cases.reference(name)
    assert ref.state_bytes(got) == ref.state_bytes(slow)
    assert info["n_voxels"] == len(got["key"]) and info["n_src_rows"] == len(src.key)
    assert int(got["count"].astype(np.int64).sum()) == int(dst.cnt.sum()) + info["n_kept_points"]
    assert info["n_new_voxels"] == len(got["key"]) - len(dst.key) and info["n_new_voxels"] <= info["n_touched"] <= info["n_kept_rows"]


def test_the_cases_are_what_their_names_say():
    info = {name: cases.reference(name)[1] for name in cases.ALL}
    for name in ("below", "above", "between"):
        assert info[name]["n_new_voxels"] == info[name]["n_touched"] == 30, name
    fresh = {}
    for name in ("below", "above", "between"):
        old = cases.case(name)[1].key
        fresh[name] = (np.setdiff1d(np.asarray(cases.reference(name)[0]["key"], np.uint64).astype(np.int64), old), old)
    assert fresh["below"][0].max() < fresh["below"][1][0] and fresh["above"][0].min() > fresh["above"][1][-1]
    assert fresh["between"][1][0] < fresh["between"][0].min() and fresh["between"][0].max() < fresh["between"][1][-1]
    assert info["none_new"]["n_new_voxels"] == 0 and info["none_new"]["n_touched"] == 25
    assert (info["one_row"]["n_src_rows"], info["one_row"]["n_touched"], info["one_row"]["n_new_voxels"]) == (1, 1, 0)
    for n in cases.EDGE_COUNTS:
        i = info[f"n{n}"]
        assert i["n_kept_rows"] == i["n_touched"] == n and 0 < i["n_new_voxels"] < n, n
    i = info["long_run"]
    assert i["n_touched"] == 1 and i["n_new_voxels"] == 0 and i["max_run"] == i["n_kept_rows"] > 280
    assert info["g_0.1_0.4_full"]["max_run"] >= 5 and info["g_0.4_0.1_full"]["max_run"] <= 2
    for name in cases.GENERAL:
        if name.endswith("full"):
            assert 0 < info[name]["n_new_voxels"] < info[name]["n_touched"], name  # overlapping and new voxels
    assert 0 < info["crop_min"]["n_kept_rows"] < info["g_0.2_0.2_full"]["n_kept_rows"]
    for name in ("all_dropped_min", "all_dropped_crop"):
        assert info[name]["n_kept_rows"] == info[name]["n_touched"] == info[name]["max_run"] == 0, name


def test_the_fold_order_shows_in_the_long_run():
    """the same rows added in descending order give other bytes: a split or reordered fold cannot hide"""
    src, dst, kw = cases.case("long_run")
    ref.merge(dst, src, descending=True, **kw)
    want = cases.reference("long_run")[0]
    other = ref.state(dst)
    assert other["key"].tobytes() == want["key"].tobytes() and other["count"].tobytes() == want["count"].tobytes()
    assert other["sums"].tobytes() != want["sums"].tobytes()


@pytest.mark.parametrize("num_classes", [0, 3, 255])
def test_identity_merge_into_an_empty_map_reproduces_src(num_classes):
    scans, qts = map_cases.four_posed()
    parts = [(xyz, (lab % (num_classes + 1)).astype(np.uint32) if num_classes else None) for xyz, lab in scans]
    src = map_cases.build(parts, qts, num_classes=num_classes)
    for qt in (None, np.array([0, 0, 0, 1, 0, 0, 0.0])):
        dst = map_ref.Map(map_cases.LEAF, num_classes)
        info = ref.merge(dst, src, qt)
        assert ref.state_bytes(ref.state(dst)) == ref.state_bytes(ref.state(src))
        assert info["n_kept_rows"] == info["n_touched"] == info["n_new_voxels"] == len(src.key) and info["max_run"] == 1


@pytest.mark.parametrize("name", cases.ALL)
def test_every_merged_rows_centroid_keys_to_its_own_row(name):
    st, _ = cases.reference(name)
    m = ref.from_state(st)
    assert np.array_equal(ref.centroid_keys(m), m.key)


def _exact_maps():
    scans, inner = cases.exact_scans()
    sub = map_cases.build(scans, inner, leaf=cases.EXACT_LEAF, num_classes=cases.EXACT_CLASSES)
    direct = map_cases.build(scans, cases.exact_composed(), leaf=cases.EXACT_LEAF, num_classes=cases.EXACT_CLASSES)
    return sub, direct


def test_exact_scene_equals_direct_integration():
    sub, direct = _exact_maps()
    assert len(sub.key) > 400 and int(sub.cnt.max()) < 300
    dst = map_ref.Map(cases.EXACT_LEAF, cases.EXACT_CLASSES)
    info = ref.merge(dst, sub, cases.HALF_TURN)
    assert info["max_run"] == 1 and info["n_kept_points"] == 4500
    assert ref.state_bytes(ref.state(dst)) == ref.state_bytes(ref.state(direct))
    assert not np.array_equal(dst.key, sub.key)  # (the pose moved every voxel)


def test_state_round_trip_and_its_refusals():
    st, _ = cases.reference("g_0.2_0.2_full")
    m = ref.from_state(st)
    assert ref.state_bytes(ref.state(m)) == ref.state_bytes(st)
    n = len(st["key"])

    def broken(**change):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        for k, (row, value) in change.items():
            bad[k][row] = value
        return bad

    swapped = broken(key=(5, st["key"][6]))
    swapped["key"][6] = st["key"][5]
    for bad, row in ((swapped, 6), (broken(key=(9, st["key"][8])), 9), (broken(key=(4, st["key"][4] & ~np.uint64(0x1fffff))), 4),
                     (broken(key=(n - 1, st["key"][n - 1] | np.uint64(1 << 63))), n - 1), (broken(count=(7, 0)), 7),
                     (broken(sums=((3, 1), np.nan)), 3), (broken(hist=((2, 1), st["hist"][2, 1] + 1)), 2)):
        with pytest.raises(ref.BadState) as e:
            ref.from_state(bad)
        assert e.value.row == row
