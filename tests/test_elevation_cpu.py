"""CPU tests of the elevation grid (sicp_map_elevation): the library exports it, the ctypes structs have the header's layout and
the defaults are the header's; and the numpy restatement the GPU tests compare against (tests/elevation_ref.py) is itself
checked -- it equals the naive twin (tests/elevation_cases.py: plain loops, cell by cell) in every output byte of every case, it
gives the values worked out by hand below for three small cases, every case hits what it is named for, and it refuses what the
header says the call refuses."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import elevation_cases as cases
import elevation_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_elevation_params", "sicp_map_elevation")


def test_library_exports_the_entry_points_with_the_headers_structs_and_defaults(tmp_path):
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    probes = [
        ("sicp_map_elevation_params", sicp.SicpMapElevationParams,
         ("z_min", "z_max", "ref_z", "min_clearance", "max_step", "width", "height", "cell_voxels", "min_count", "clearance_voxels",
          "use_ref_z", "max_extent_voxels", "min_neighbors", "n_ignore", "n_blocked", "n_drivable", "ignore", "blocked", "drivable")),
        ("sicp_map_elevation_out", sicp.SicpMapElevationOut, tuple(n for n, _ in ref.CELL_ARRAYS + ref.POINT_ARRAYS)),
        ("sicp_map_elevation_info", sicp.SicpMapElevationInfo,
         ("n_voxels", "n_points", "x0", "y0", "width", "height", "n_class", "cell_size", "t_total_ms")),
    ]
    prints = "".join(
        f'  printf("%zu", sizeof({c}));' + "".join(f' printf(" %zu", offsetof({c}, {f}));' for f in fields) + ' printf("\\n");\n'
        for c, _, fields in probes)
    code = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sicp.h\"\nint main(void) {\n" + prints +
            '  printf("%d %d %d %d %d %d %d %d\\n", SICP_MAP_ELEVATION_MAX_LABELS, SICP_ELEVATION_UNKNOWN, SICP_ELEVATION_FREE,'
            ' SICP_ELEVATION_BLOCKED_LABEL, SICP_ELEVATION_OBSTACLE, SICP_ELEVATION_LOW_CLEARANCE, SICP_ELEVATION_STEP,'
            ' SICP_ELEVATION_SPARSE);\n  return 0;\n}\n')
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
    assert [int(v) for v in rows[-1].split()] == [sicp.MAP_ELEVATION_MAX_LABELS, sicp.ELEVATION_UNKNOWN, sicp.ELEVATION_FREE,
                                                   sicp.ELEVATION_BLOCKED_LABEL, sicp.ELEVATION_OBSTACLE, sicp.ELEVATION_LOW_CLEARANCE,
                                                   sicp.ELEVATION_STEP, sicp.ELEVATION_SPARSE]
    assert sicp.MAP_ELEVATION_MAX_LABELS == ref.MAX_LABELS == 64
    assert [sicp.ELEVATION_UNKNOWN, sicp.ELEVATION_FREE, sicp.ELEVATION_BLOCKED_LABEL, sicp.ELEVATION_OBSTACLE,
            sicp.ELEVATION_LOW_CLEARANCE, sicp.ELEVATION_STEP, sicp.ELEVATION_SPARSE] == \
        [ref.UNKNOWN, ref.FREE, ref.BLOCKED_LABEL, ref.OBSTACLE, ref.LOW_CLEARANCE, ref.STEP, ref.SPARSE]
    assert tuple((n, np.dtype(d)) for n, d in sicp.ELEVATION_CELL_ARRAYS) == tuple((n, np.dtype(d)) for n, d in ref.CELL_ARRAYS)
    assert tuple((n, np.dtype(d)) for n, d in sicp.ELEVATION_POINT_ARRAYS) == tuple((n, np.dtype(d)) for n, d in ref.POINT_ARRAYS)

    p = sicp.default_map_elevation_params()
    d = ref.defaults()
    for k in ("width", "height", "cell_voxels", "min_count", "z_min", "z_max", "clearance_voxels", "use_ref_z", "ref_z", "max_extent_voxels",
              "min_clearance", "max_step", "min_neighbors"):
        assert getattr(p, k) == d[k], k
    assert (p.width, p.height, p.cell_voxels, p.min_count, p.clearance_voxels, p.use_ref_z, p.max_extent_voxels, p.min_neighbors) == \
        (0, 0, 1, 1, 10, 0, 2, 0)
    assert (p.z_min, p.z_max, p.ref_z, p.min_clearance, p.max_step) == (-math.inf, math.inf, 0.0, 0.0, math.inf)
    assert (p.n_ignore, p.n_blocked, p.n_drivable, p.reserved_) == (0, 0, 0, 0)
    assert not any(p.ignore) and not any(p.blocked) and not any(p.drivable)
    assert lib.sicp_default_map_elevation_params(None) == sicp.ERR_INVALID_ARGUMENT
    q = sicp.default_map_elevation_params(ignore=(3, 1), blocked=(2,), drivable=(1, 2, 4), cell_voxels=4, ref_z=1.5)
    assert (q.n_ignore, q.n_blocked, q.n_drivable, q.cell_voxels, q.ref_z) == (2, 1, 3, 4, 1.5)
    assert list(q.ignore[:3]) == [3, 1, 0] and list(q.drivable[:4]) == [1, 2, 4, 0]
    with pytest.raises(AttributeError):
        sicp.default_map_elevation_params(no_such_field=1)
    with pytest.raises(ValueError):
        sicp.default_map_elevation_params(ignore=range(65))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_restatement_equals_the_naive_twin_in_every_byte(name):
    c = cases.case(name)
    want = cases.naive(c["state"], c["params"], c["center"], c["points"], c["qt"])
    got = cases.reference(name)
    arrays = ref.CELL_ARRAYS + (ref.POINT_ARRAYS if c["points"] is not None else ())
    assert set(got) == {n for n, _ in arrays} | {"info"}
    for k, dt in arrays:
        assert got[k].dtype == want[k].dtype == dt and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))[:5])
    assert got["info"] == want["info"] and tuple(got["info"]) == ref.INFO
    assert sum(got["info"]["n_class"]) == c["width"] * c["height"]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_hits_what_it_is_named_for(name):
    cases.case(name)["expect"](cases.reference(name))


def test_the_segment_cases_hold_the_row_counts_around_a_wave():
    """cells with 0, 1, 2, 63, 64, 65, 128 and 129 counting rows, at one column a cell and at four"""
    for name, B in (("segments_b1", 1), ("segments_b2", 2)):
        st = cases.case(name)["state"]
        vx = (st["key"].astype(np.int64) & 0x1FFFFF) - cases.BIAS
        assert np.bincount(vx // B, minlength=8).tolist() == list(cases.SEGMENT_ROWS)
    st = cases.case("b8_full")["state"]
    key = st["key"].astype(np.int64)
    vx, vz = (key & 0x1FFFFF) - cases.BIAS, (key >> 42) - cases.BIAS
    assert [int(((vx // 8 == 0) & (vz == l)).sum()) for l in (3, 4, 5, 16)] == [64, 64, 64, 64]
    big = cases.case("large_random")
    assert big["params"]["width"] * big["params"]["height"] > 1 << 15 and len(big["state"]["key"]) > 190000  # 21 + 16 sorted bits


def test_hand_derived_values_clearance():
    """leaf 0.5, every voxel 2 points at a mean z of (level + 0.5) / 2.  Column 0 holds the levels 0 and 10: 10 - 0 is not above
    clearance_voxels = 10, one run of two levels, elevation 5.25, bottom 0.25, no ceiling.  Column 1 holds 0 and 11: two runs,
    the surface is level 0 at 0.25 under a ceiling at 5.75.  The two cells are neighbours: |0.25 - 5.25| = 5."""
    out = cases.reference("clearance_exact")
    a, b = (1, 2), (1, 3)
    want = dict(state=(1, 1), elevation=(5.25, 0.25), bottom=(0.25, 0.25), ceiling=(math.inf, 5.75), label=(1, 1), count=(2, 2),
                level_top=(10, 0), level_bottom=(0, 0), n_levels=(2, 1), step=(5.0, 5.0), neighbors=(1, 1), cell_class=(ref.FREE, ref.FREE))
    for k, (va, vb) in want.items():
        assert (out[k][a], out[k][b]) == (va, vb), k
    assert int(out["state"].sum()) == 2 and np.isnan(out["elevation"][0, 0]) and np.isnan(out["step"][0, 0])
    assert out["elevation"][0, 0].tobytes() == np.array([0x7FC00000], np.uint32).tobytes()
    assert out["info"] == dict(n_voxels=4, n_points=0, x0=-2, y0=-1, width=4, height=2, n_class=[6, 2, 0, 0, 0, 0, 0, 0], cell_size=0.5)


def test_hand_derived_values_three_runs():
    """levels 0 1 | 20 21 22 | 40, 3 points a voxel; ref_z = 10.0 is level 20, the second run's bottom: that run is the surface,
    top 22 at 11.25, bottom 20 at 10.25, under the third run's 40 at 20.25.  The neighbour column holds level 20 alone."""
    out = cases.reference("three_runs_ref_on1")
    c = (0, 1)
    want = dict(state=1, elevation=11.25, bottom=10.25, ceiling=20.25, label=2, count=3, level_top=22, level_bottom=20, n_levels=3,
                step=1.0, neighbors=1, cell_class=ref.FREE)
    for k, v in want.items():
        assert out[k][c] == v, k
    assert out["elevation"][0, 2] == 10.25 and np.isinf(out["ceiling"][0, 2]) and out["state"][0, 0] == 0
    below = cases.reference("three_runs_ref_below")
    assert (below["elevation"][c], below["bottom"][c], below["ceiling"][c], below["n_levels"][c]) == (0.75, 0.25, 10.25, 2)
    assert below["cell_class"][c] == ref.FREE and below["step"][c] == 9.5


def test_hand_derived_values_classes():
    """the cell (6, 7) of classes_all: levels 2 and 6 with clearance_voxels = 3 are two runs, so the surface is level 2 at 1.25
    under a ceiling at 3.25 -- 2.0 of head room under min_clearance = 3.0 -- with its two neighbours (6, 6) and (6, 8) at 0.25:
    a step of 1.0 over max_step = 0.6, which the clearance test comes before"""
    out = cases.reference("classes_all")
    c = (7, 6)
    want = dict(state=1, elevation=1.25, bottom=1.25, ceiling=3.25, label=1, count=2, level_top=2, level_bottom=2, n_levels=1, step=1.0,
                neighbors=2, cell_class=ref.LOW_CLEARANCE)
    for k, v in want.items():
        assert out[k][c] == v, k
    tall = (7, 4)  # levels 0..3 | 7: extent 3, elevation 1.75 under 3.75, 1.5 above its neighbours
    assert (out["elevation"][tall], out["ceiling"][tall], out["step"][tall], out["n_levels"][tall], out["cell_class"][tall]) == \
        (1.75, 3.75, 1.5, 4, ref.OBSTACLE)
    assert out["cell_class"][6, 6] == ref.STEP and out["cell_class"][6, 8] == ref.STEP  # the flat cells beside the stepped ones
    assert out["cell_class"][:4, :4].tolist() == [[ref.FREE] * 4] * 4
    assert out["neighbors"][:4, :4].tolist() == [[3, 5, 5, 3], [5, 8, 8, 5], [5, 8, 8, 5], [3, 5, 5, 3]]


def test_window_independence_of_the_restatement():
    """rule 9: a cell's rule-5 arrays do not depend on the window it is seen through"""
    st = cases.patch_state()
    a = ref.elevation(st, ref.defaults(width=9, height=7, clearance_voxels=2), (0.3, 0.3))
    b = ref.elevation(st, ref.defaults(width=6, height=12, clearance_voxels=2), (1.9, -0.8))
    ia, ib = a["info"], b["info"]
    xs = range(max(ia["x0"], ib["x0"]), min(ia["x0"] + 9, ib["x0"] + 6))
    ys = range(max(ia["y0"], ib["y0"]), min(ia["y0"] + 7, ib["y0"] + 12))
    assert len(xs) >= 3 and len(ys) >= 3
    for k in ref.WINDOW_FREE:
        va = a[k][ys[0] - ia["y0"]:ys[-1] + 1 - ia["y0"], xs[0] - ia["x0"]:xs[-1] + 1 - ia["x0"]]
        vb = b[k][ys[0] - ib["y0"]:ys[-1] + 1 - ib["y0"], xs[0] - ib["x0"]:xs[-1] + 1 - ib["x0"]]
        assert va.tobytes() == vb.tobytes(), k


def test_the_restatements_refusals():
    st = cases.patch_state()
    ok = dict(width=4, height=4)
    assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**ok), (0.0, 0.0)) is None
    for what, kw in cases.REFUSED.items():
        assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**{**ok, **kw}), (0.0, 0.0)), what
        with pytest.raises(ref.Refused):
            ref.elevation(st, ref.defaults(**{**ok, **kw}), (0.0, 0.0))
    for what, kw in cases.ACCEPTED.items():
        assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**{**ok, **kw}), (0.0, 0.0)) is None, what
    p = ref.defaults(**ok)
    for name in ("ignore", "blocked", "drivable"):  # a label list on a map without classes; a list too long
        assert ref.refusal(0.5, 0, ref.defaults(**{**ok, name: (0,)}), (0.0, 0.0)) == name
        assert ref.refusal(0.5, 70, ref.defaults(**{**ok, name: tuple(range(65))}), (0.0, 0.0)) == name
        assert ref.refusal(0.5, 70, ref.defaults(**{**ok, name: tuple(range(64))}), (0.0, 0.0)) is None
    assert ref.refusal(0.5, 4, None, (0.0, 0.0)) == "params" and ref.refusal(0.5, 4, p, None) == "center"
    for c in ((math.nan, 0.0), (0.0, math.inf), (0.5 * (1 << 20), 0.0), (0.0, -0.5 * (1 << 20) - 0.5), (1e300, 0.0)):
        assert ref.refusal(0.5, 4, p, c) == "center", c
    assert ref.refusal(0.5, 4, p, (0.5 * (1 << 20) - 0.5, -0.5 * (1 << 20) + 0.5)) is None  # |vc| = 2^20 - 1 on both axes
    assert ref.refusal(0.5, 4, p, (0.0, 0.0), qt=[0, 0, 0, 1, math.nan, 0, 0]) == "pose"
    assert ref.refusal(0.5, 4, p, (0.0, 0.0), want_points=True) == "points"
    assert ref.refusal(0.5, 4, p, (0.0, 0.0), have_handle=True, which=2) == "which"
    assert ref.refusal(0.5, 4, p, (0.0, 0.0), have_handle=True, which=1, want_points=True) is None
