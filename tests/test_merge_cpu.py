"""CPU tests of sicp_merge_clouds: the library exports it, the ctypes structs have the header's layout, and the numpy
restatement the GPU tests compare against (tests/merge_ref.py) is itself checked -- against the bootstrap's voxel grid,
against a transcription of exec/filter_range.h, against an independent slow restatement -- on inputs that have the properties
they are meant to have."""
import ctypes
import importlib
import os
import subprocess
import textwrap

import numpy as np
import pytest

import bootstrap_ref
import merge_cases
import merge_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


def test_library_exports_the_merge_entry_points():
    lib = ctypes.CDLL(sicp.build())
    assert hasattr(lib, "sicp_merge_clouds") and hasattr(lib, "sicp_default_merge_params")


def test_struct_layouts_match_the_header(tmp_path):
    code = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu\\n", sizeof(sicp_merge_params), sizeof(sicp_merge_info), offsetof(sicp_merge_params, crop_range),
                 offsetof(sicp_merge_info, n_out), offsetof(sicp_merge_info, t_total_ms));
          return 0;
        }
        """
    )
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    a, b, o1, o2, o3 = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(sicp.SicpMergeParams) == a and ctypes.sizeof(sicp.SicpMergeInfo) == b
    assert sicp.SicpMergeParams.crop_range.offset == o1
    assert sicp.SicpMergeInfo.n_out.offset == o2 and sicp.SicpMergeInfo.t_total_ms.offset == o3


def test_default_merge_params():
    p = sicp.default_merge_params()
    assert (p.leaf_size, list(p.crop_center), p.crop_range) == (0.2, [0.0, 0.0, 0.0], 0.0)
    q = sicp.default_merge_params(leaf_size=0.5, crop_center=(1, 2, 3), crop_range=40.0)
    assert (q.leaf_size, list(q.crop_center), q.crop_range) == (0.5, [1.0, 2.0, 3.0], 40.0)
    with pytest.raises(AttributeError):
        sicp.default_merge_params(min_points=3)
    assert sicp.lib().sicp_default_merge_params(None) == sicp.ERR_INVALID_ARGUMENT


# ---- the restatement against what already exists ----------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", [0.4, 0.07])
def test_one_part_identity_no_crop_is_the_bootstraps_voxel_grid(leaf):
    rng = np.random.default_rng(5)
    xyz = rng.uniform(-4, 4, (3000, 3)).astype(np.float32)
    xyz[::97, 1] = np.nan
    got = merge_ref.merge([(xyz, None)], None, leaf)
    want = bootstrap_ref.voxel_keypoints(xyz, box_max=np.inf, leaf=leaf)
    assert got["xyz"].dtype == np.float32 and got["xyz"].tobytes() == want.tobytes()
    assert got["n_out"] == len(want) and got["count"].sum() == got["n_kept"] == got["n_in"] == 3000 - len(xyz[::97])


def test_leaf_zero_centre_zero_is_filter_range():
    rng = np.random.default_rng(6)
    xyz = rng.uniform(-6, 6, (3000, 3)).astype(np.float32)
    xyz[7] = (3, 4, 0)  # d^2 = range^2 exactly: not erased
    lab = rng.integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32)
    got = merge_ref.merge([(xyz, lab)], None, 0.0, (0, 0, 0), 5.0)
    want = merge_ref.filter_range([(p[0], p[1], p[2], l) for p, l in zip(xyz, lab)], 5.0)
    assert 0 < len(want) < 3000 and got["n_out"] == len(want)
    assert np.array_equal(got["xyz"], np.array([w[:3] for w in want], dtype=np.float32))
    assert np.array_equal(got["labels"], np.array([w[3] for w in want], dtype=np.uint32))
    assert (got["count"] == 1).all() and got["max_voxel_points"] == 1
    assert (got["xyz"] == np.float32([3, 4, 0])).all(axis=1).any()


@pytest.mark.parametrize("name", merge_cases.NAMES)
def test_restatement_equals_the_slow_restatement(name):
    a, b = merge_cases.reference(name), merge_cases.run_ref(merge_cases.case(name), merge_ref.merge_slow)
    for k in ("n_in", "n_kept", "n_out", "max_voxel_points", "has_label"):
        assert a[k] == b[k], k
    assert a["xyz"].tobytes() == b["xyz"].tobytes()
    assert np.array_equal(a["count"], b["count"])
    assert (a["labels"] is None) == (b["labels"] is None)
    if a["labels"] is not None:
        assert np.array_equal(a["labels"], b["labels"])


def test_the_grid_refuses_coordinates_beyond_its_fields():
    xyz = np.array([[100.0, 1.0, 2.0]], dtype=np.float32)
    with pytest.raises(merge_ref.GridOverflow):
        merge_ref.merge([(xyz, None)], None, 1e-6)
    assert merge_ref.merge([(xyz, None)], None, 1e-3)["n_out"] == 1


def test_mixed_labelled_and_unlabelled_parts_are_refused():
    a, b = merge_cases.scan(1, 40), merge_cases.scan(2, 40, labelled=False)
    with pytest.raises(ValueError):
        merge_ref.merge([a, b])


# ---- the cases have the properties they are meant to have ---------------------------------------------------------------------
def _voxel_label_counts(name):
    """per voxel of the case, in the result's order: {label: count}"""
    c = merge_cases.case(name)
    p, lab = merge_ref.gather(c["parts"], c["qts"])
    keep = merge_ref.crop_mask(p, c["center"], c["crop_range"])
    v = merge_ref.voxel_coords(p[keep], c["leaf"])
    cells = {}
    for key, l in zip(map(tuple, v[:, ::-1]), lab[keep]):
        cells.setdefault(key, {}).setdefault(int(l), 0)
        cells[key][int(l)] += 1
    return [cells[k] for k in sorted(cells)]


def test_cases_hold_label_ties_and_the_smallest_label_wins():
    for name in ("five", "blob"):
        r = merge_cases.reference(name)
        ties = 0
        for k, cell in enumerate(_voxel_label_counts(name)):
            top = max(cell.values())
            winners = sorted(l for l, n in cell.items() if n == top)
            assert r["labels"][k] == winners[0]
            ties += len(winners) > 1
        assert ties >= 1, name
    labels = merge_cases.reference("five")["labels"]
    assert (labels == 0).any() and (labels == 0xFFFFFFFF).any()


def test_cases_hold_a_long_voxel_single_point_voxels_and_negative_voxels():
    blob = merge_cases.reference("blob")
    assert blob["max_voxel_points"] >= 5000 and blob["count"].max() == blob["max_voxel_points"]
    k = int(np.argmax(blob["count"]))
    assert blob["labels"][k] == 3  # 2750 of label 3 and 2750 of label 5 (the 500 scattered points may add a few)
    five = merge_cases.reference("five")
    assert (five["count"] == 1).any() and (five["count"] > 1).any()
    assert (five["voxels"] < 0).any(axis=0).all() and (five["voxels"] > 0).any(axis=0).all()


def test_cases_hold_non_finite_points_and_straddle_the_workgroup():
    parts = merge_cases.case("five")["parts"]
    assert sorted(len(x) for x, _ in parts) == sorted(merge_cases.SIZES)
    n_all = sum(len(x) for x, _ in parts)
    n_fin = sum(int(np.isfinite(x).all(axis=1).sum()) for x, _ in parts)
    assert merge_cases.reference("five")["n_in"] == n_fin
    assert 0.02 * n_all < n_all - n_fin < 0.04 * n_all


def test_cases_hold_a_point_on_the_crop_sphere_and_a_part_wholly_cropped():
    c = merge_cases.case("crop_edge")
    r = merge_cases.reference("crop_edge")
    assert r["labels"].tolist() == [0, 3, 5, 6] and r["n_kept"] == 4  # (4,4,0) and (1,0,5) at d^2 = 25 stay; one ulp further goes
    p, _ = merge_ref.gather(c["parts"], c["qts"])
    d = (p - np.float32(c["center"])).astype(np.float32)
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2[0] == np.float32(25) and d2[3] == np.float32(25) and d2[1] > 25 and d2[4] > 25
    for name, far in (("five", merge_cases.FAR), ("five_far_256", 2)):
        c = merge_cases.case(name)
        alone = merge_ref.merge([c["parts"][far]], c["qts"][far:far + 1], c["leaf"], c["center"], c["crop_range"])
        assert alone["n_in"] > 0 and alone["n_kept"] == 0 and alone["n_out"] == 0 and alone["max_voxel_points"] == 0
        assert 0 < merge_cases.reference(name)["n_kept"] < merge_cases.reference(name)["n_in"]
    assert merge_cases.reference("five_inf")["n_kept"] == merge_cases.reference("five_inf")["n_in"]
    assert merge_cases.reference("five_inf")["xyz"].tobytes() == merge_cases.reference("five_nocrop")["xyz"].tobytes()
