"""CPU tests of the persistent voxel map (sicp_map_*): the library exports it, the ctypes structs have the header's layout,
there is no fallback without a device, and the numpy restatement the GPU tests compare against (tests/map_ref.py) is itself
checked -- it equals merge_ref.merge of all scans byte for byte, it equals an independent slow restatement, and the chained
merge it replaces differs from it in the way the documents say."""
import ctypes
import importlib
import os
import subprocess
import textwrap

import numpy as np
import pytest

import map_cases
import map_ref
import merge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_params", "sicp_map_create", "sicp_map_destroy", "sicp_map_clear", "sicp_map_size",
                "sicp_map_last_error", "sicp_map_integrate", "sicp_map_prune", "sicp_default_map_extract_params", "sicp_map_extract")


def test_library_exports_the_map_entry_points():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_struct_layouts_match_the_header(tmp_path):
    probes = [
        ("sicp_map_params", sicp.SicpMapParams, ("leaf_size", "num_classes")),
        ("sicp_map_integrate_info", sicp.SicpMapIntegrateInfo, ("n_in", "n_kept", "n_scan_voxels", "n_new_voxels", "n_voxels", "t_total_ms")),
        ("sicp_map_extract_params", sicp.SicpMapExtractParams, ("min_count", "crop_center", "crop_range")),
        ("sicp_map_extract_info", sicp.SicpMapExtractInfo, ("n_voxels", "n_out", "max_voxel_points", "has_label", "t_total_ms")),
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


def test_defaults_and_unknown_overrides():
    p = sicp.default_map_params()
    assert (p.leaf_size, p.num_classes) == (0.2, 0)
    q = sicp.default_map_params(leaf_size=0.5, num_classes=19)
    assert (q.leaf_size, q.num_classes) == (0.5, 19)
    with pytest.raises(AttributeError):
        sicp.default_map_params(crop_range=3.0)
    e = sicp.default_map_extract_params()
    assert (e.min_count, list(e.crop_center), e.crop_range) == (1, [0.0, 0.0, 0.0], 0.0)
    f = sicp.default_map_extract_params(min_count=3, crop_center=(1, 2, 3), crop_range=40.0)
    assert (f.min_count, list(f.crop_center), f.crop_range) == (3, [1.0, 2.0, 3.0], 40.0)
    with pytest.raises(AttributeError):
        sicp.default_map_extract_params(leaf_size=0.1)
    assert sicp.lib().sicp_default_map_params(None) == sicp.ERR_INVALID_ARGUMENT
    assert sicp.lib().sicp_default_map_extract_params(None) == sicp.ERR_INVALID_ARGUMENT


def test_null_maps_are_refused_not_dereferenced():
    lib = sicp.lib()
    assert lib.sicp_map_destroy(None) == sicp.OK
    assert lib.sicp_map_clear(None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_size(None, None, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_integrate(None, None, 0, None, None, 0.0, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_prune(None, None, 1.0, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_extract(None, None, None, 0, 0, None, None, None, None, None, None, None) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_map_last_error(None) == b""
    out = ctypes.c_void_p()
    assert lib.sicp_map_create(0, None, ctypes.byref(out)) == sicp.ERR_INVALID_ARGUMENT and not out.value
    for bad in (dict(leaf_size=0.0), dict(leaf_size=float("nan")), dict(leaf_size=float("inf")), dict(num_classes=-1), dict(num_classes=256)):
        assert lib.sicp_map_create(0, ctypes.byref(sicp.default_map_params(**bad)), ctypes.byref(out)) == sicp.ERR_INVALID_ARGUMENT, bad
    assert lib.sicp_map_create(0, ctypes.byref(sicp.default_map_params()), None) == sicp.ERR_INVALID_ARGUMENT


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_no_gpu_means_loud_failure_not_fallback():
    with pytest.raises(sicp.SicpError) as e:
        sicp.VoxelMap(0)
    assert e.value.status == sicp.ERR_NO_DEVICE


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def _same_bytes(got, want):
    assert got["n_out"] == want["n_out"] and got["max_voxel_points"] == want["max_voxel_points"]
    assert got["xyz"].dtype == np.float32 and got["xyz"].tobytes() == want["xyz"].tobytes()
    assert np.array_equal(got["count"], want["count"])
    assert (got["labels"] is None) == (want["labels"] is None)
    if want["labels"] is not None:
        assert got["labels"].dtype == np.uint32 and got["labels"].tobytes() == want["labels"].tobytes()


@pytest.mark.parametrize("crop", [False, True], ids=["nocrop", "crop"])
@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("posed", [False, True], ids=["plain", "posed"])
def test_map_equals_the_one_shot_merge(posed, labelled, crop):
    got, want = map_cases.reference(posed, labelled, crop)
    assert want["n_out"] > 1000 and (not crop or want["n_kept"] < want["n_in"])
    if posed:
        assert want["n_in"] < 4 * 1500  # the NaN rows are gone
    _same_bytes(got, want)


def test_map_equals_the_slow_restatement():
    scans, qts = map_cases.four_posed()
    kw = dict(qts=qts, center=map_cases.CENTER, crop_range=map_cases.RANGE)
    a = map_cases.build(scans, **kw).extract()
    b = map_cases.build(scans, cls=map_ref.MapSlow, **kw).extract()
    _same_bytes(a, b)
    for min_count in (2, 3):
        a = map_cases.build(scans, **kw).extract(min_count=min_count)
        b = map_cases.build(scans, cls=map_ref.MapSlow, **kw).extract(min_count=min_count)
        assert 0 < a["n_out"] < map_cases.reference(True, True, True)[0]["n_out"]
        _same_bytes(a, b)


def test_info_counts_and_sizes_follow_the_scans():
    scans = map_cases.four()
    m = map_ref.Map(map_cases.LEAF, map_cases.CLASSES)
    seen = 0
    for xyz, lab in scans:
        before = m.size()[0]
        info = m.integrate(xyz, lab)
        seen += len(xyz)
        assert info["n_in"] == info["n_kept"] == len(xyz) and info["n_voxels"] == before + info["n_new_voxels"] == m.size()[0]
        assert 0 < info["n_scan_voxels"] <= len(xyz) and m.size()[1] == seen
    assert info["n_new_voxels"] < info["n_scan_voxels"]  # the fourth scan mostly lands in voxels the map holds
    ex = m.extract()
    assert (ex["hist"].sum(axis=1) == ex["count"]).all() and (ex["hist"][:, 0] == 0).all()


def test_the_chained_merge_differs_in_centroids_and_labels():
    """the figures of INTEGRATION.md, "A persistent voxel map": the same voxels, but most centroids and a fifth of the labels"""
    scans = map_cases.four()
    got, want = map_cases.reference(False, True, False)
    chain = map_ref.chained_merge(scans, None, map_cases.LEAF)
    assert chain["n_out"] == want["n_out"] == got["n_out"]
    xyz_differ = int((chain["xyz"].view(np.uint32) != want["xyz"].view(np.uint32)).any(axis=1).sum())
    labels_differ = int((chain["labels"] != want["labels"]).sum())
    print(f"voxels {want['n_out']}, max points {want['max_voxel_points']}, chained merge: {xyz_differ} centroids "
          f"({100.0 * xyz_differ / want['n_out']:.0f} %) and {labels_differ} labels ({100.0 * labels_differ / want['n_out']:.0f} %) differ")
    assert xyz_differ > 0 and labels_differ > 0
    assert not np.array_equal(chain["count"], want["count"])  # (its counts are those of the last merge only)


def test_five_road_points_then_two_car_points():
    """a voxel seen five times as label 1, then twice as label 2: the map says 1, the chain -- one map point against two -- says 2"""
    road = map_cases.lattice([[0, 0, 0]], per_cell=5, label=1, seed=1)
    car = map_cases.lattice([[0, 0, 0]], per_cell=2, label=2, seed=2)
    m = map_cases.build([road, car], num_classes=2).extract()
    assert m["n_out"] == 1 and m["labels"].tolist() == [1] and m["count"].tolist() == [7] and m["hist"].tolist() == [[0, 5, 2]]
    chain = map_ref.chained_merge([road, car], None, map_cases.LEAF)
    assert chain["n_out"] == 1 and chain["labels"].tolist() == [2] and chain["count"].tolist() == [3]
    both = merge_ref.merge([road, car], None, map_cases.LEAF)
    assert m["xyz"].tobytes() == both["xyz"].tobytes() and chain["xyz"].tobytes() != both["xyz"].tobytes()


def test_refusals_of_the_restatement_change_nothing():
    scans = map_cases.four()
    m = map_cases.build(scans[:2])
    before = m.extract()
    xyz, lab = scans[2]
    bad = lab.copy()
    bad[7] = map_cases.CLASSES + 1
    far = xyz.copy()
    far[3] = (1e6, 0, 0)
    with pytest.raises(map_ref.BadLabel):
        m.integrate(xyz, bad)
    with pytest.raises(merge_ref.GridOverflow):
        m.integrate(far, lab)
    with pytest.raises(ValueError):
        m.integrate(xyz, None)
    after = m.extract()
    _same_bytes(after, before)
    assert after["hist"].tobytes() == before["hist"].tobytes()


def test_prune_keeps_the_survivors_bits():
    scans, qts = map_cases.four_posed()
    m = map_cases.build(scans, qts)
    full = m.extract()
    removed = m.prune(map_cases.CENTER, 2.5)
    cut = m.extract()
    want = map_cases.build(scans, qts).extract(center=map_cases.CENTER, crop_range=2.5)
    assert 0 < removed == full["n_out"] - cut["n_out"]
    _same_bytes(cut, want)
    assert m.prune(map_cases.CENTER, np.inf) == 0
