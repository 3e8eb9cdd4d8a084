"""CPU tests of the distance field (sicp_map_distance): the library exports it, the ctypes structs have the header's layout and the
defaults are the header's; and the numpy restatement the GPU tests compare against (tests/distance_ref.py) is itself checked --
it equals the naive twin (tests/distance_cases.py: obstacle by obstacle, no packed keys, no separable passes) in every output
byte of every case, its dist_sq is scipy's exact Euclidean distance transform squared wherever that is within R, it gives the
values worked out by hand below for three small cases, every case hits what it is named for, and it refuses what the header
says the call refuses."""
import ctypes
import importlib
import math
import os
import subprocess

import numpy as np
import pytest
from scipy import ndimage

import distance_cases as cases
import distance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_default_map_distance_params", "sicp_map_distance")


def test_library_exports_the_entry_points_with_the_headers_structs_and_defaults(tmp_path):
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    probes = [
        ("sicp_map_distance_params", sicp.SicpMapDistanceParams,
         ("z_min", "z_max", "nx", "ny", "nz", "max_dist_voxels", "min_count", "planar", "n_ignore", "n_only", "ignore", "only")),
        ("sicp_map_distance_out", sicp.SicpMapDistanceOut, tuple(n for n, _ in ref.CELL_ARRAYS + ref.POINT_ARRAYS)),
        ("sicp_map_distance_info", sicp.SicpMapDistanceInfo, ref.INFO + ("t_total_ms",)),
    ]
    prints = "".join(
        f'  printf("%zu", sizeof({c}));' + "".join(f' printf(" %zu", offsetof({c}, {f}));' for f in fields) + ' printf("\\n");\n'
        for c, _, fields in probes)
    code = ("#include <stdio.h>\n#include <stddef.h>\n#include \"sicp.h\"\nint main(void) {\n" + prints +
            '  printf("%d\\n", SICP_MAP_DISTANCE_MAX_LABELS);\n  return 0;\n}\n')
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
    assert int(rows[-1]) == sicp.MAP_DISTANCE_MAX_LABELS == ref.MAX_LABELS == 64
    assert tuple((n, np.dtype(d)) for n, d in sicp.DISTANCE_CELL_ARRAYS) == tuple((n, np.dtype(d)) for n, d in ref.CELL_ARRAYS)
    assert tuple((n, np.dtype(d)) for n, d in sicp.DISTANCE_POINT_ARRAYS) == tuple((n, np.dtype(d)) for n, d in ref.POINT_ARRAYS)

    p = sicp.default_map_distance_params()
    d = ref.defaults()
    for k in ("nx", "ny", "nz", "max_dist_voxels", "min_count", "planar", "z_min", "z_max"):
        assert getattr(p, k) == d[k], k
    assert (p.nx, p.ny, p.nz, p.max_dist_voxels, p.min_count, p.planar, p.n_ignore, p.n_only) == (0, 0, 0, 10, 1, 0, 0, 0)
    assert (p.z_min, p.z_max) == (-math.inf, math.inf)
    assert not any(p.ignore) and not any(p.only)
    assert lib.sicp_default_map_distance_params(None) == sicp.ERR_INVALID_ARGUMENT
    q = sicp.default_map_distance_params(ignore=(3, 1), only=(2,), max_dist_voxels=4, z_max=1.5)
    assert (q.n_ignore, q.n_only, q.max_dist_voxels, q.z_max) == (2, 1, 4, 1.5)
    assert list(q.ignore[:3]) == [3, 1, 0] and list(q.only[:2]) == [2, 0]
    with pytest.raises(AttributeError):
        sicp.default_map_distance_params(no_such_field=1)
    with pytest.raises(ValueError):
        sicp.default_map_distance_params(only=range(65))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_the_restatement_equals_the_naive_twin_in_every_byte(name):
    c = cases.case(name)
    want = cases.naive(c["state"], c["params"], c["center"], c["points"], c["qt"])
    got = cases.reference(name)
    arrays = ref.CELL_ARRAYS + (ref.point_arrays(c["params"]) if c["points"] is not None else ())
    assert set(got) == set(want) == {n for n, _ in arrays} | {"info"}
    for k, dt in arrays:
        assert got[k].dtype == want[k].dtype == dt and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), (k, np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))[:5])
    assert got["info"] == want["info"] and tuple(got["info"]) == ref.INFO
    assert got["info"]["n_reached"] == int((got["dist_sq"] >= 0).sum()) and got["dist_sq"].shape == c["shape"][::-1]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_hits_what_it_is_named_for(name):
    cases.case(name)["expect"](cases.reference(name))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_dist_sq_is_the_exact_transform_squared_within_r(name):
    """scipy's exact Euclidean distance transform of the window's obstacle cells, with nothing outside the window: equal where its
    square is <= R^2, unreached everywhere else; and the nearest row it names is one at that distance"""
    got = cases.reference(name)
    R = cases.case(name)["params"]["max_dist_voxels"]
    free = got["dist_sq"] != 0
    if not (~free).any():
        assert (got["dist_sq"] == -1).all()
        return
    edt, idx = ndimage.distance_transform_edt(free, return_indices=True)
    sq = np.rint(edt * edt).astype(np.int64)
    assert np.array_equal(got["dist_sq"], np.where(sq <= R * R, sq, -1))
    reached = got["dist_sq"] >= 0
    assert np.array_equal(got["nearest"] >= 0, reached)
    # the cell that scipy names holds an obstacle at the same distance; ours may be another one at that distance, of a smaller row
    seeds = got["nearest"][tuple(idx)]
    assert (seeds[reached] >= got["nearest"][reached]).all()


def test_the_cases_hold_the_shapes_the_kernels_turn_on():
    """one cell; no multiple of a wave or a tile; more than one tile along every axis (130 > 4 x 32, 66 > 64, 35 with R = 6 needs
    the z halo); a line of 1024 > 256 + 2 x 64; R above every dimension; R = 1; about 1 % occupancy"""
    shapes = {n: cases.case(n)["shape"] for n in cases.CASES}
    R = {n: cases.case(n)["params"]["max_dist_voxels"] for n in cases.CASES}
    assert shapes["one_cell_occupied"] == (1, 1, 1) and shapes["shape_67x5x3"] == (67, 5, 3) and shapes["shape_130x66x35"] == (130, 66, 35)
    assert shapes["long_line_r64"] == (1024, 4, 2) and R["long_line_r64"] == 64
    assert R["r_larger_than_window"] > max(shapes["r_larger_than_window"]) and R["r1"] == 1
    dense = cases.case("dense")
    assert dense["shape"] == (96, 80, 40) and R["dense"] == 8 and len(dense["state"]["key"]) == 96 * 80 * 40 // 100


def test_hand_derived_values_the_ball():
    """R = 5, two lone obstacles 15 cells apart in a 30 x 12 x 3 window whose cell (0, 0, 0) is voxel (0, 0, 0).  A = (5, 5, 1) is row
    0 with label 2, B = (20, 5, 1) row 1 with label 3.  A + (3, 4, 0): 9 + 16 = 25 = R^2, reached.  B + (5, 1, 0): 25 + 1 = 26, not
    reached although each offset is <= R.  B + (4, 1, 1): 16 + 1 + 1 = 18.  Each ball holds the cells with di^2 + dj^2 + dk^2 <=
    25 and |dk| <= 1 that lie in the window: 81 in the obstacle's plane and 69 in each of the two others, and no cell is in both."""
    out = cases.reference("ball_not_cube")
    assert (out["dist_sq"][1, 9, 8], out["nearest"][1, 9, 8], out["label"][1, 9, 8]) == (25, 0, 2)
    assert (out["dist_sq"][1, 6, 25], out["nearest"][1, 6, 25], out["label"][1, 6, 25]) == (-1, -1, 0)
    assert (out["dist_sq"][2, 6, 24], out["nearest"][2, 6, 24], out["label"][2, 6, 24]) == (18, 1, 3)
    assert (out["dist_sq"][1, 5, 5], out["dist_sq"][1, 5, 20], out["dist_sq"][0, 5, 5]) == (0, 0, 1)
    assert out["info"] == dict(n_voxels=2, n_points=0, n_points_inside=0, x0=0, y0=0, z0=0, nx=30, ny=12, nz=3, n_obstacles=2,
                               n_reached=2 * (81 + 2 * 69), max_dist_sq=25, voxel_size=0.5)


def test_hand_derived_values_the_tie_along_three_axes():
    """from cell (4, 5, 2) the obstacles (7, 5, 2), (4, 2, 2) and (4, 5, 5) are all at d^2 = 9.  Keys ascend by z, then y, then x, so
    (4, 2, 2) is row 0, (7, 5, 2) row 1, (4, 5, 5) row 2: the cell takes row 0 and its label 2.  One cell further along +x, (5, 5,
    2), row 1 is alone at 4; at (4, 5, 3) row 2 is alone at 4."""
    out = cases.reference("tie_axes")
    assert (out["dist_sq"][2, 5, 4], out["nearest"][2, 5, 4], out["label"][2, 5, 4]) == (9, 0, 2)
    assert (out["dist_sq"][2, 5, 5], out["nearest"][2, 5, 5], out["label"][2, 5, 5]) == (4, 1, 1)
    assert (out["dist_sq"][3, 5, 4], out["nearest"][3, 5, 4], out["label"][3, 5, 4]) == (4, 2, 3)
    assert (out["dist_sq"][2, 4, 4], out["nearest"][2, 4, 4]) == (4, 0)
    assert (out["info"]["x0"], out["info"]["y0"], out["info"]["z0"]) == (0, 0, 0)


def test_hand_derived_values_planar():
    """leaf 0.5: z_min = 1.0 is level 2, z_max = 2.9 level 5.  Column (2, 2) holds the levels 0, 3, 7: level 3 is its row.  Column
    (6, 2) holds 3 and 4: level 3, the smaller row.  Column (10, 2) holds 0 and 9: no obstacle, and with R = 4 it is reached from
    (6, 2) at exactly 16.  Column (2, 6) holds 5 and 2: level 2.  The rows in ascending key (z, y, x): (2,2,0) 0, (10,2,0) 1,
    (2,6,2) 2, (2,2,3) 3, (6,2,3) 4, (6,2,4) 5, (2,6,5) 6, (2,2,7) 7, (10,2,9) 8."""
    out = cases.reference("planar_band")
    d, near, lab = out["dist_sq"][0], out["nearest"][0], out["label"][0]
    assert (d[2, 2], near[2, 2], lab[2, 2]) == (0, 3, 2)
    assert (d[2, 6], near[2, 6], lab[2, 6]) == (0, 4, 4)
    assert (d[6, 2], near[6, 2], lab[6, 2]) == (0, 2, 1)
    assert (d[2, 10], near[2, 10], lab[2, 10]) == (16, 4, 4)
    assert (d[2, 11], near[2, 11]) == (-1, -1)
    assert (d[4, 2], near[4, 2]) == (4, 2) and (d[2, 4], near[2, 4]) == (4, 3)
    assert out["info"]["n_obstacles"] == 3 and out["info"]["z0"] == 0 and out["info"]["n_voxels"] == 9


def test_window_independence_of_the_restatement():
    """rule 6: a cell at least R cells from every face of both windows has the same bytes through either"""
    st = cases.patch_state()
    R = 2
    a = ref.distance(st, ref.defaults(nx=19, ny=17, nz=9, max_dist_voxels=R), (0.3, 0.3, 1.2))
    b = ref.distance(st, ref.defaults(nx=14, ny=22, nz=8, max_dist_voxels=R), (1.9, -0.8, 0.6))
    _assert_shared_cells_equal(a, b, R, 3)


def _assert_shared_cells_equal(a, b, R, least):
    ia, ib = a["info"], b["info"]
    span = []
    for o, n in (("x0", "nx"), ("y0", "ny"), ("z0", "nz")):
        lo, hi = max(ia[o], ib[o]) + R, min(ia[o] + ia[n], ib[o] + ib[n]) - R
        assert hi - lo >= least, (o, lo, hi)
        span.append((lo, hi))
    cut = lambda out, i: tuple(slice(lo - i[o], hi - i[o]) for (lo, hi), o in zip(span[::-1], ("z0", "y0", "x0")))
    for k, _ in ref.CELL_ARRAYS:
        assert a[k][cut(a, ia)].tobytes() == b[k][cut(b, ib)].tobytes(), k
    assert (a["dist_sq"][cut(a, ia)] >= 0).any()


def test_the_restatements_refusals():
    st = cases.patch_state()
    ok = dict(nx=4, ny=4, nz=4)
    centre = (0.0, 0.0, 0.0)
    assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**ok), centre) is None
    for what, kw in cases.REFUSED.items():
        assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**{**ok, **kw}), centre), what
        with pytest.raises(ref.Refused):
            ref.distance(st, ref.defaults(**{**ok, **kw}), centre)
    for what, kw in cases.ACCEPTED.items():
        assert ref.refusal(st["leaf_size"], st["num_classes"], ref.defaults(**{**ok, **kw}), centre) is None, what
    p = ref.defaults(**ok)
    for name in ("ignore", "only"):  # a label list on a map without classes; a list too long
        assert ref.refusal(0.5, 0, ref.defaults(**{**ok, name: (0,)}), centre) == name
        assert ref.refusal(0.5, 70, ref.defaults(**{**ok, name: tuple(range(65))}), centre) == name
        assert ref.refusal(0.5, 70, ref.defaults(**{**ok, name: tuple(range(64))}), centre) is None
    assert ref.refusal(0.5, 4, None, centre) == "params" and ref.refusal(0.5, 4, p, None) == "center"
    far = 0.5 * (1 << 20)
    for c in ((math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, math.nan), (far, 0.0, 0.0), (0.0, 0.0, -far - 0.5), (1e300, 0.0, 0.0)):
        assert ref.refusal(0.5, 4, p, c) == "center", c
    assert ref.refusal(0.5, 4, p, (far - 0.5, -far + 0.5, far - 0.5)) is None  # |vc| = 2^20 - 1 on every axis
    flat = ref.defaults(nx=4, ny=4, nz=1, planar=1)
    assert ref.refusal(0.5, 4, flat, (0.0, 0.0, far)) is None and ref.refusal(0.5, 4, flat, (0.0, 0.0, math.inf)) == "center"
    assert ref.refusal(0.5, 4, p, centre, qt=[0, 0, 0, 1, math.nan, 0, 0]) == "pose"
    assert ref.refusal(0.5, 4, p, centre, want_points=True) == "points"
    assert ref.refusal(0.5, 4, p, centre, have_handle=True, which=2) == "which"
    assert ref.refusal(0.5, 4, flat, centre, have_handle=True, want_points=True, want_range=True) == "point_range_sq"
    assert ref.refusal(0.5, 4, p, centre, have_handle=True, which=1, want_points=True, want_range=True) is None
