"""CPU tests of the camera rules: tests/camera_ref.py, the numpy restatement the GPU tests compare to the bit, against
independent statements -- a plain float64 pinhole in OpenCV's operation order for the projection, hand-derived pixels for the
points on pixel edges and bounds, the round trip depth frame -> points -> pixels on three published calibrations, two walls
for the occlusion test, hand cases for the label rules -- and the host-only entry points sicp_default_camera_params /
sicp_camera_matrices."""
import importlib

import numpy as np
import pytest

import camera_cases
import camera_ref as R

sicp = importlib.import_module("semantic-icp_amd")
MARGIN = 1e-9  # px: a point nearer than this to a pixel edge may fall to either side of it in another operation order


def _pinhole(xyz, p, qt):
    """OpenCV's projectPoints in float64: matrix product, r2 / r4 / r6 powers, the tangential terms as OpenCV writes them"""
    m = R.matrices(qt)
    Rm, t = m["cam_to_cloud"][:, :3], m["cam_to_cloud"][:, 3]
    with np.errstate(all="ignore"):
        pc = (xyz.astype(np.float64) - t) @ Rm  # R^T (x - t)
        x, y = pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2]
        r2 = x * x + y * y
        r4, r6 = r2 * r2, r2 * r2 * r2
        rad = 1 + p.k1 * r2 + p.k2 * r4 + p.k3 * r6
        xd = x * rad + 2 * p.p1 * x * y + p.p2 * (r2 + 2 * x * x)
        yd = y * rad + p.p1 * (r2 + 2 * y * y) + 2 * p.p2 * x * y
        u, v = p.fx * xd + p.cx, p.fy * yd + p.cy
    return pc[:, 2], r2, u, v


# ---- (a) the projection ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(camera_cases.RANDOM))
def test_the_restatement_equals_a_plain_pinhole(name):
    c = camera_cases.random_case(name)
    p = R.params(**c["p"])
    W, H = p.width, p.height
    pr = R.project(c["xyz"], p, R.matrices(c["qt"]))
    Z, r2, u, v = _pinhole(c["xyz"], p, c["qt"])
    with np.errstate(all="ignore"):
        finite = np.isfinite(c["xyz"]).all(axis=1)
        safe = finite & (np.abs(u + 0.5 - np.round(u + 0.5)) > MARGIN) & (np.abs(v + 0.5 - np.round(v + 0.5)) > MARGIN)
        want = finite & (Z >= p.min_depth) & (Z < p.max_depth) & (r2 <= p.max_tan_sq)
        col, row = np.floor(u + 0.5), np.floor(v + 0.5)
        want &= (col >= 0) & (col < W) & (row >= 0) & (row < H)
        pixel = np.where(want, row * W + col, -1)
    left_out = 1.0 - safe[finite].mean()
    print("points:", len(u), "finite:", int(finite.sum()), "left out by the margin:", left_out, "with a pixel:", int(want.sum()))
    assert left_out <= 0.001
    assert want.sum() > 0.3 * len(u) and (~want & finite).sum() > 0.1 * len(u)
    assert (pr["pixel"][safe] == pixel[safe]).all()
    assert (pr["pixel"][~finite] == -1).all()
    # u, v themselves agree far below a pixel
    both = safe & want
    assert np.abs(pr["u"][both] - u[both]).max() < 1e-9 and np.abs(pr["v"][both] - v[both]).max() < 1e-9


def test_points_on_pixel_edges_and_bounds_by_hand():
    c, want = camera_cases.edges_case()
    p = R.params(**c["p"])
    im = R.image(c["xyz"], c["labels"], p, R.matrices(None))
    print(im["pixel"].tolist())
    assert im["pixel"].tolist() == want.tolist()
    # r2 = 4 exactly is inside the view and has u, v; r2 just above is not and has none
    i4 = np.flatnonzero((c["xyz"] == [4, 0, 2]).all(axis=1))[0]
    assert im["u"][i4] == 39.5 and im["v"][i4] == 5.5 and np.isnan(im["u"][i4 + 1]) and np.isnan(im["v"][i4 + 1])
    assert im["n_finite"] == len(want) - 3 and im["n_kept"] == im["n_finite"] - 5
    assert im["n_outside"] == im["n_kept"] - (want >= 0).sum()


def test_the_winner_by_hand():
    c = camera_cases.winner_case()
    im = R.image(c["xyz"], c["labels"], R.params(**c["p"]), R.matrices(None))
    assert im["visible"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0]
    assert im["index"][6, 8] == 3 and im["depth"][6, 8] == 1.0 and im["count"][6, 8] == 5 and im["label"][6, 8] == 4
    assert im["index"][6, 3] == 5 and im["depth"][6, 3] == 2.0 and im["count"][6, 3] == 3
    assert im["n_pixels_hit"] == 2 and (im["index"] >= 0).sum() == 2
    c = camera_cases.crowd_case()
    im = R.image(c["xyz"], c["labels"], R.params(**c["p"]), R.matrices(None))
    assert im["n_pixels_hit"] == 1 and im["count"].max() == 3000 and im["visible"].sum() == 1
    assert im["visible"][np.argmin(c["xyz"][:, 2])] == 1


# ---- (b) the round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(camera_cases.CALIBRATIONS))
def test_unproject_then_project_returns_every_pixel(name):
    """depths of 0.5 .. 60 m over the whole frame, the default 20 iterations: every pixel comes back to itself, |u - c| and
    |v - r| below 1e-3 px (the restated formula gave 2.6e-5 px at worst, on KITTI raw, with the points kept in float64; the float32
    points of the engine add up to about 1e-4 px at the image's edge)"""
    p = R.params(**camera_cases.CALIBRATIONS[name])
    W, H = p.width, p.height
    depth = np.random.default_rng(5).uniform(0.5, 60.0, (H, W)).astype(np.float32)
    mat = R.matrices(camera_cases.QT)
    un = R.unproject(depth, p, mat)
    assert un["valid"].all() and un["n_valid"] == W * H
    pr = R.project(un["xyz"], p, mat)
    c, r = np.meshgrid(np.arange(W), np.arange(H))
    du, dv = np.abs(pr["u"] - c.reshape(-1)).max(), np.abs(pr["v"] - r.reshape(-1)).max()
    print(name, "worst |u - c|:", du, "worst |v - r|:", dv)
    assert pr["inimage"].all()
    assert (pr["pixel"] == np.arange(W * H)).all()
    assert du < 1e-3 and dv < 1e-3


def test_five_iterations_are_not_enough_on_a_wide_lens():
    """why the default is 20 and not OpenCV's 5: KITTI raw's lens is off by more than a pixel at the corners after 5 passes"""
    p = R.params(**dict(camera_cases.CALIBRATIONS["kitti_raw"], undistort_iterations=5))
    mat = R.matrices(None)
    un = R.unproject(np.full((p.height, p.width), 10.0, np.float32), p, mat)
    pr = R.project(un["xyz"], p, mat)
    c, _ = np.meshgrid(np.arange(p.width), np.arange(p.height))
    worst = np.abs(pr["u"] - c.reshape(-1)).max()
    print("worst |u - c| at 5 iterations:", worst)
    assert worst > 0.5


def test_zero_coefficients_make_every_pass_exact():
    p0 = R.params(**dict(camera_cases.intrinsics(64, 48), undistort_iterations=0))
    p64 = R.params(**dict(camera_cases.intrinsics(64, 48), undistort_iterations=64))
    d = camera_cases.depth_f32(64, 48, 3)
    mat = R.matrices(camera_cases.QT)
    a, b = R.unproject(d, p0, mat), R.unproject(d, p64, mat)
    assert a["xyz"].tobytes() == b["xyz"].tobytes() and a["valid"].tobytes() == b["valid"].tobytes()


def test_invalid_depths():
    p = R.params(**camera_cases.intrinsics(16, 12))
    d = camera_cases.depth_u16(16, 12, 1)
    un = R.unproject(d, p, R.matrices(None))
    assert un["valid"][0, 0] == 0 and un["valid"][0, 1] == 1 and un["valid"][1, 0] == 0 and un["valid"][11, 15] == 1 and un["valid"][11, 0] == 1
    assert (un["valid"] == ((d >= 300) & (d.astype(np.float64) * 0.001 < 100.0))).all()
    assert np.isnan(un["xyz"][~un["valid"].reshape(-1).astype(bool)]).all() and np.isfinite(un["xyz"][un["valid"].reshape(-1).astype(bool)]).all()
    assert un["xyz"][1, 2] == np.float32(65535 * 0.001)
    f = camera_cases.depth_f32(16, 12, 2)
    un = R.unproject(f, p, R.matrices(None))
    assert un["valid"][0, 0] == 1 and un["valid"][0, 1] == 0 and un["valid"][1, 0] == 0 and un["valid"][1, 1] == 1
    with np.errstate(all="ignore"):
        assert (un["valid"] == (np.isfinite(f) & (f >= np.float32(0.3)) & (f < 100))).all()
    assert 0 < un["n_valid"] < 16 * 12


# ---- (c) occlusion --------------------------------------------------------------------------------------------------------------
def test_the_far_wall_behind_the_near_wall_is_occluded():
    c, wall = camera_cases.walls_case()
    p = R.params(**c["p"])
    W, H, half = p.width, p.height, p.window // 2
    out = R.labels(c["xyz"], c["labels"], c["pixel_label"], p, R.matrices(c["qt"]))
    # independently: the pixel of every point by the plain pinhole; a pixel with a near-wall point is won by the near wall
    Z, r2, u, v = _pinhole(c["xyz"], p, c["qt"])
    col, row = np.floor(u + 0.5).astype(int), np.floor(v + 0.5).astype(int)
    inimage = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    near_px = np.zeros((H + 2 * half, W + 2 * half), dtype=bool)
    sel = inimage & (wall == 1)
    near_px[row[sel] + half, col[sel] + half] = True
    covered = np.zeros(len(wall), dtype=bool)
    for wr in range(2 * half + 1):
        for wc in range(2 * half + 1):
            covered[inimage] |= near_px[row[inimage] + wr, col[inimage] + wc]
    want = np.where(~inimage, 0, np.where((wall == 2) & covered, 2, 1))
    print("points:", len(wall), "in the image:", int(inimage.sum()), "occluded:", int((want == 2).sum()), "the restatement's:", out["n_occluded"])
    assert (want == 2).sum() > 200 and ((want == 1) & (wall == 2)).sum() > 200 and ((want == 1) & (wall == 1)).sum() > 200 and (want == 0).sum() > 0
    assert out["state"].tolist() == want.tolist()
    assert (out["labels"][want == 1] == 7).all() and (out["labels"][want != 1] == wall[want != 1]).all()


# ---- (d) the label rules --------------------------------------------------------------------------------------------------------
def test_label_rules_by_hand():
    """the edge camera, window 3: A alone at pixel (6, 8), class 5 -> takes it; B at (6, 3), class 0 -> keeps its own, state 3;
    C behind B in the same pixel -> occluded; D one column beside B, 0.4 m behind it -> occluded by the window (0.4 > 0.3 + 0.02 * 2);
    E in D's place but 0.3 m behind -> seen (0.3 < 0.34); F outside the image; G not finite"""
    pts = [(0.0, 0.0, 3.0), (-0.625, 0.0, 2.0), (-0.9375, 0.0, 3.0), (-0.5, 0.0, 2.4), (-0.5, 0.0, 2.3), (4.0, 0.0, 2.0), (np.nan, 0.0, 1.0)]
    own = np.array([11, 12, 13, 14, 15, 16, 17], np.uint32)
    p = R.params(**camera_cases.EDGE_P)
    pl = np.zeros((12, 16), np.uint32)
    pl[6, 8], pl[6, 4] = 5, 9
    mat = R.matrices(None)
    im = R.image(np.array(pts, np.float32), own, p, mat)
    assert im["pixel"].tolist() == [6 * 16 + 8, 6 * 16 + 3, 6 * 16 + 3, 6 * 16 + 4, 6 * 16 + 4, -1, -1]
    out = R.labels(np.array(pts[:4] + pts[5:], np.float32), own[[0, 1, 2, 3, 5, 6]], pl, p, mat)  # without E
    assert out["state"].tolist() == [1, 3, 2, 2, 0, 0] and out["labels"].tolist() == [5, 12, 13, 14, 16, 0]
    out = R.labels(np.array(pts[:3] + pts[4:], np.float32), own[[0, 1, 2, 4, 5, 6]], pl, p, mat)  # without D
    assert out["state"].tolist() == [1, 3, 2, 1, 0, 0] and out["labels"].tolist() == [5, 12, 13, 9, 16, 0]
    assert (out["n_labelled"], out["n_occluded"], out["n_unclassed"]) == (2, 1, 1)
    # window 1: only C's own pixel counts, D is seen
    out = R.labels(np.array(pts[:4] + pts[5:], np.float32), own[[0, 1, 2, 3, 5, 6]], pl, R.params(**dict(camera_cases.EDGE_P, window=1)), mat)
    assert out["state"].tolist() == [1, 3, 2, 1, 0, 0]
    # a cloud without labels: 0 wherever the point keeps its own
    out = R.labels(np.array(pts[:4] + pts[5:], np.float32), None, pl, p, mat)
    assert out["labels"].tolist() == [5, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("window", [1, 3, 15])
def test_windows_at_the_image_corners(window):
    """a near point in each corner pixel and a far one in the pixel diagonally inside it: the window is cut at the border, never
    wrapped -- at 1 nobody is occluded, at 3 the four inner points are, at 15 also every far point within 7 pixels of a corner"""
    p = R.params(**dict(camera_cases.EDGE_P, window=window))
    pts, far = [], []
    for r, c in ((0, 0), (0, 15), (11, 0), (11, 15)):
        pts.append(((c - 7.5) / 16.0, (r - 5.5) / 16.0, 1.0))
        ri, ci = (1 if r == 0 else 10), (1 if c == 0 else 14)
        pts.append(((ci - 7.5) / 16.0 * 2.0, (ri - 5.5) / 16.0 * 2.0, 2.0))
    pts.append(((8 - 7.5) / 16.0 * 2.0, (0 - 5.5) / 16.0 * 2.0, 2.0))  # row 0, column 8: 8 columns from the left corner, 7 from the right
    pts.append(((7 - 7.5) / 16.0 * 2.0, (11 - 5.5) / 16.0 * 2.0, 2.0))  # row 11, column 7: the mirror image
    out = R.labels(np.array(pts, np.float32), None, np.full((12, 16), 3, np.uint32), p, R.matrices(None))
    inner = [1, 3, 5, 7]
    want = np.ones(10, int)
    if window >= 3:
        want[inner] = 2
    if window == 15:
        want[8:] = 2
    assert out["state"].tolist() == want.tolist()
    # wrapping would have reached across: column 8 of row 0 is 8 columns from (0, 0) -- outside a window of 15 -- and would be 8 from (0, 15 + 1)
    assert out["image"]["pixel"][8] == 8 and out["image"]["pixel"][9] == 11 * 16 + 7


# ---- (e) the binding ------------------------------------------------------------------------------------------------------------
def test_default_params_and_matrices():
    p = sicp.default_camera_params()
    ref = R.params()
    for k, v in vars(ref).items():
        assert getattr(p, k) == v, k
    assert sicp.default_camera_params(window=7, k1=0.25).window == 7
    with pytest.raises(AttributeError):
        sicp.default_camera_params(nothing=1)
    for qt in (None, camera_cases.QT, [0, 0, 0, 2, 1, 2, 3]):
        m = sicp.camera_matrices(qt)
        ref = R.matrices(qt)
        assert m["cam_to_cloud"].tobytes() == ref["cam_to_cloud"].tobytes() and m["cloud_to_cam"].tobytes() == ref["cloud_to_cam"].tobytes()
    m = sicp.camera_matrices(camera_cases.QT)
    a, b = np.eye(4), np.eye(4)
    a[:3], b[:3] = m["cam_to_cloud"], m["cloud_to_cam"]
    err = max(np.abs(a @ b - np.eye(4)).max(), np.abs(b @ a - np.eye(4)).max())
    print("the matrices' product differs from the identity by", err)
    assert err < 1e-15
    ident = sicp.camera_matrices(None)
    assert (ident["cam_to_cloud"] == np.eye(4)[:3]).all() and (ident["cloud_to_cam"] == np.eye(4)[:3]).all()
    for bad in ([0, 0, 0, 0, 1, 2, 3], [0, 0, 0, 1, np.nan, 0, 0], [np.inf, 0, 0, 1, 0, 0, 0]):
        with pytest.raises(sicp.SicpError) as err:
            sicp.camera_matrices(bad)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT


def test_struct_layouts_match_the_header(tmp_path):
    """sizes and the offsets of the last fields, computed by the C compiler for the header's declarations"""
    import os
    import subprocess

    C = sicp.C
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sicp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", '
                   "sizeof(sicp_camera_params), offsetof(sicp_camera_params, undistort_iterations), offsetof(sicp_camera_params, occlusion_rel), "
                   "sizeof(sicp_camera_info), offsetof(sicp_camera_info, t_total_ms)); return 0; }\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    P, I = sicp.SicpCameraParams, sicp.SicpCameraInfo
    assert got == [C.sizeof(P), P.undistort_iterations.offset, P.occlusion_rel.offset, C.sizeof(I), I.t_total_ms.offset]
