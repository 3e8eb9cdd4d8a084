"""Inputs of the camera tests (tests/test_camera_cpu.py, tests/test_gpu_camera.py): seeded clouds in front of, beside and behind
a camera, the points that sit exactly on pixel edges and on the depth bounds, the winner and view-gate constructions, depth
frames with every kind of invalid pixel, three published calibrations, and two walls for the occlusion test.  A case is {"xyz":
float32 [n, 3], "labels": uint32 [n] or None, "p": keywords for camera_ref.params / default_camera_params, "qt": 7 floats or
None, "pixel_label": uint32 [H, W]}."""
import numpy as np

import camera_ref as R

F = np.float32
QT = np.array([0.18, -0.12, 0.31, 0.0, 0.7, -0.4, 1.1])  # a general pose (camera -> cloud); the quaternion is scaled to length 1 below
QT[3] = np.sqrt(1.0 - (QT[:3] ** 2).sum())
LENS = dict(k1=-0.21, k2=0.09, p1=0.003, p2=-0.002, k3=-0.01)  # a mild wide-angle lens
# published calibrations (k1, k2, p1, p2, k3 in OpenCV's order): the NYU Depth v2 toolbox's RGB and depth cameras, KITTI raw's camera 0
CALIBRATIONS = {
    "nyu_rgb": dict(width=640, height=480, fx=518.86, fy=519.47, cx=325.58, cy=253.74, k1=0.2624, k2=-0.9531, p1=-0.0054, p2=0.0026, k3=1.1633),
    "nyu_depth": dict(width=640, height=480, fx=582.62, fy=582.69, cx=313.04, cy=238.44, k1=-0.0999, k2=0.3926, p1=0.0019, p2=-0.0013, k3=-0.6762),
    "kitti_raw": dict(width=1392, height=512, fx=984.2, fy=980.8, cx=690.0, cy=233.2, k1=-0.3728, k2=0.2037, p1=0.0022, p2=0.0014, k3=-0.0723),
}


def intrinsics(W, H):
    """a pinhole of about 70 degrees across W, the principal point off the centre by a fraction of a pixel"""
    return dict(width=W, height=H, fx=0.71 * W, fy=0.73 * W, cx=0.5 * W - 0.37, cy=0.5 * H - 0.61)


def case(xyz, labels=None, qt=None, pixel_label=None, seed=0, **p):
    q = R.params(**p)
    if pixel_label is None:
        pixel_label = np.random.default_rng(1000 + seed).integers(0, 4, (q.height, q.width)).astype(np.uint32)
    return {"xyz": np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3), "labels": None if labels is None else np.asarray(labels, np.uint32),
            "p": p, "qt": None if qt is None else np.asarray(qt, dtype=np.float64), "pixel_label": pixel_label}


def cloud(n, seed, p, qt=None, z_lo=0.1, z_hi=30.0, behind=0.05, spread=1.3):
    """n seeded points given in the camera's frame by an (undistorted) pixel position spread beyond the image and a log-uniform depth,
    a share of them behind the camera, moved into the cloud's frame; float32, labels 1 .. 9"""
    rng = np.random.default_rng(seed)
    q = R.params(**p)
    u = q.cx + (rng.uniform(-0.5, 0.5, n) * spread) * q.width
    v = q.cy + (rng.uniform(-0.5, 0.5, n) * spread) * q.height
    Z = np.exp(rng.uniform(np.log(z_lo), np.log(z_hi), n))
    Z[rng.random(n) < behind] *= -1.0
    pc = np.stack([(u - q.cx) / q.fx * Z, (v - q.cy) / q.fy * Z, Z], axis=1)
    m = R.matrices(qt)["cam_to_cloud"]
    return (pc @ m[:, :3].T + m[:, 3]).astype(F), rng.integers(1, 10, n).astype(np.uint32)


# ---- random clouds --------------------------------------------------------------------------------------------------------------
# (W, H, points, lens, pose, window): the two small images, no multiple of anything, with and without lens and pose
RANDOM = {"w16h12": (16, 12, 2000, False, False, 3), "w16h12_lens_pose": (16, 12, 3000, True, True, 15), "w64h48": (64, 48, 20000, False, True, 5),
          "w64h48_lens": (64, 48, 8000, True, False, 1), "w9h8": (9, 8, 2500, True, True, 15)}


def random_case(name, labelled=True):
    W, H, n, lens, pose, window = RANDOM[name]
    p = dict(intrinsics(W, H), window=window, max_depth=25.0, **(LENS if lens else {}))
    qt = QT if pose else None
    xyz, lab = cloud(n, 11 + W + n, p, qt)
    xyz[::97] = np.nan
    xyz[5::211, 1] = np.inf
    return case(xyz, lab if labelled else None, qt, seed=W + n, **p)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
EDGE_P = dict(width=16, height=12, fx=16.0, fy=16.0, cx=7.5, cy=5.5, min_depth=0.5, max_depth=8.0, max_tan_sq=4.0, window=3)


def edges_case():
    """fx = fy = 16, cx = 7.5, cy = 5.5, identity pose, Z a power of two: xn = k / 16 puts u + 0.5 = k + 8 on an integer exactly.
    Returns the case and, per point, the pixel derived by hand (-1: none)."""
    pts, want = [], []

    def add(x, y, z, pixel):
        pts.append((x, y, z))
        want.append(pixel)

    # u + 0.5 = 3 exactly, v + 0.5 = 6 exactly: the edge belongs to the pixel to its right / below (floor)
    add(-5 / 16 * 2.0, 0.0, 2.0, 6 * 16 + 3)
    # the floats next to that edge in x: one to the left falls into column 2, one to the right stays in column 3
    add(float(np.nextafter(F(-0.625), F(-1))), 0.0, 2.0, 6 * 16 + 2)
    add(float(np.nextafter(F(-0.625), F(0))), 0.0, 2.0, 6 * 16 + 3)
    # the image's borders: u + 0.5 = 0 is inside (column 0), u + 0.5 = 16 is outside; the same for the rows
    add(-8 / 16 * 4.0, 0.0, 4.0, 6 * 16 + 0)
    add(8 / 16 * 4.0, 0.0, 4.0, -1)
    add(0.0, -6 / 16 * 4.0, 4.0, 0 * 16 + 8)
    add(0.0, 6 / 16 * 4.0, 4.0, -1)
    add(float(np.nextafter(F(-2.0), F(-3))), 0.0, 4.0, -1)
    add(0.0, float(np.nextafter(F(1.5), F(0))), 4.0, 11 * 16 + 8)
    # the corners' pixels
    add(-7.5 / 16 * 1.0, -5.5 / 16 * 1.0, 1.0, 0)
    add(7.5 / 16 * 1.0, 5.5 / 16 * 1.0, 1.0, 11 * 16 + 15)
    # the depth gate: min_depth is inside, max_depth is not; behind the camera; Zc = 0
    add(0.0, 0.0, 0.5, 6 * 16 + 8)
    add(0.0, 0.0, float(np.nextafter(F(0.5), F(0))), -1)
    add(0.0, 0.0, 8.0, -1)
    add(0.0, 0.0, float(np.nextafter(F(8.0), F(0))), 6 * 16 + 8)
    add(0.1, 0.1, -1.0, -1)
    add(0.1, 0.1, 0.0, -1)
    add(0.0, 0.0, 0.0, -1)
    # the view gate: r2 = 4 exactly is inside the view (and beyond the image), r2 = 4 + 2^-40 is not
    add(4.0, 0.0, 2.0, -1)
    add(4.0, 2.0 ** -19, 2.0, -1)
    # not finite
    add(np.nan, 0.0, 2.0, -1)
    add(0.0, 0.0, np.inf, -1)
    add(-np.inf, 0.0, 2.0, -1)
    xyz = np.array(pts, dtype=F)
    return case(xyz, np.arange(1, len(xyz) + 1), seed=1, **EDGE_P), np.array(want, dtype=np.int32)


def winner_case():
    """pixel (6, 8) of the edge camera: five points, the nearest comes fourth (index 3); pixel (6, 3): a point, its duplicate and
    a farther one -- equal float depths go to the smaller index (5)"""
    pts = [(0.01, 0.0, 3.0), (0.0, 0.0, 2.0), (0.02, 0.01, 2.0), (0.0, 0.0, 1.0), (0.0, 0.0, 4.0),
           (-0.625, 0.0, 2.0), (-0.625, 0.0, 2.0), (-0.7, 0.01, 2.5)]
    return case(np.array(pts, dtype=F), [1, 2, 3, 4, 5, 6, 7, 8], seed=2, **EDGE_P)


def crowd_case(n=3000):
    """n points in one pixel with seeded depths: one winner, count n"""
    rng = np.random.default_rng(21)
    Z = rng.uniform(1.0, 7.0, n)
    xyz = np.stack([0.01 * Z, -0.01 * Z, Z], axis=1).astype(F)
    return case(xyz, rng.integers(1, 9, n), seed=3, **EDGE_P)


# ---- depth frames ---------------------------------------------------------------------------------------------------------------
def depth_u16(W, H, seed):
    """a seeded uint16 frame: 0, 65535, the units at either side of min_depth = 0.3 at depth_scale 0.001, and holes"""
    rng = np.random.default_rng(seed)
    d = rng.integers(250, 9000, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < 0.15] = 0
    d[0, 0], d[0, 1], d[1, 0], d[H - 1, W - 1], d[H - 1, 0] = 0, 65535, 299, 300, 301
    return d


def depth_f32(W, H, seed):
    """a seeded float frame in metres with NaN, +-Inf, negative and zero pixels and both bounds"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.2, 12.0, (H, W)).astype(F)
    bad = rng.random((H, W))
    d[bad < 0.05] = np.nan
    d[(bad >= 0.05) & (bad < 0.08)] = np.inf
    d[(bad >= 0.08) & (bad < 0.10)] = -np.inf
    d[(bad >= 0.10) & (bad < 0.13)] = -1.5
    d[(bad >= 0.13) & (bad < 0.15)] = 0.0
    d[0, 0], d[0, 1], d[1, 0], d[1, 1] = 0.3, np.nextafter(F(0.3), F(0)), 100.0, np.nextafter(F(100.0), F(0))
    return d


def frame_labels(W, H, seed):
    return np.random.default_rng(seed).integers(0, 6, (H, W)).astype(np.uint32)


# (W, H, dtype, lens, pose, iterations)
FRAMES = {"u16_w16h12": (16, 12, np.uint16, False, False, 20), "f32_w16h12_lens_pose": (16, 12, F, True, True, 20),
          "u16_w64h48_lens_pose_it64": (64, 48, np.uint16, True, True, 64), "f32_w64h48_lens_it0": (64, 48, F, True, False, 0),
          "f32_w9h8_pose_it1": (9, 8, F, False, True, 1), "u16_w640h480_lens_pose": (640, 480, np.uint16, True, True, 20)}


def frame_case(name):
    W, H, dtype, lens, pose, it = FRAMES[name]
    p = dict(intrinsics(W, H), undistort_iterations=it, **(LENS if lens else {}))
    depth = depth_u16(W, H, 31 + W) if dtype == np.uint16 else depth_f32(W, H, 37 + W)
    return {"depth": depth, "label": frame_labels(W, H, 41 + W), "p": p, "qt": QT if pose else None}


# ---- two walls ------------------------------------------------------------------------------------------------------------------
def walls_case(W=64, H=48):
    """a scanner at the origin looks along +z at a near wall (z = 5, x < 0.4) in front of a far wall (z = 10); the camera sits 1.5 m
    to the scanner's left, on the near wall's side, so far-wall places the scanner saw past the near wall's edge lie behind that wall
    for the camera.  Returns the case and, per point, 1 for a near-wall point, 2 for a far one."""
    ax, ay = np.meshgrid(np.linspace(-0.55, 0.55, 150), np.linspace(-0.4, 0.4, 110))  # the scanner's rays, by their slopes
    ax, ay = ax.reshape(-1), ay.reshape(-1)
    near = ax * 5.0 < 0.4
    Z = np.where(near, 5.0, 10.0)
    xyz = np.stack([ax * Z, ay * Z, Z], axis=1).astype(F)
    wall = np.where(near, 1, 2).astype(np.uint32)
    qt = np.array([0, 0, 0, 1, -1.5, 0, 0], dtype=np.float64)
    p = dict(width=W, height=H, fx=0.9 * W, fy=0.9 * W, cx=0.5 * W - 0.5, cy=0.5 * H - 0.5, window=5)
    return case(xyz, wall, qt, pixel_label=np.full((H, W), 7, np.uint32), **p), wall
