"""Inputs of the range-image tests (tests/test_range_cpu.py, tests/test_gpu_range.py): seeded clouds around a sensor, the
points that sit exactly on sector edges, row edges, the view's borders, the vertical axis and the range bounds, the winner and
vote constructions, and a 64-beam scan of a box room.  A case is {"xyz": float32 [n, 3], "labels": uint32 [n] or None, "p":
keywords for range_ref.params / default_range_params, "origin": 3 floats or None, "beam": float64 [H] or None}."""
import numpy as np

F = np.float32


def sphere(n, seed, r_lo=0.2, r_hi=60.0, el_lo=-0.6, el_hi=0.25, origin=None):
    """n seeded points by azimuth, elevation and range (log-uniform), float32, about `origin`, with labels 1 .. 9"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(el_lo, el_hi, n)
    r = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), n))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1)
    if origin is not None:
        xyz = xyz + np.asarray(origin, dtype=np.float64)
    return xyz.astype(F), rng.integers(1, 10, n).astype(np.uint32)


def case(xyz, labels=None, origin=None, beam=None, **p):
    return {"xyz": np.ascontiguousarray(xyz, dtype=F).reshape(-1, 3), "labels": None if labels is None else np.asarray(labels, np.uint32),
            "p": p, "origin": origin, "beam": None if beam is None else np.asarray(beam, dtype=np.float64)}


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# (W, H, points): one row; two rows; neither half nor rows a power of two; the largest tables
SHAPES = {"w16h1": (16, 1, 700), "w16h2": (16, 2, 700), "w24h5": (24, 5, 4000), "w4096h256": (4096, 256, 3000)}


def shape_case(name, clockwise=1, col_shift=None):
    W, H, n = SHAPES[name]
    xyz, lab = sphere(n, 100 + W + H, origin=(1.5, -2.0, 0.5))
    kw = dict(width=W, height=H, clockwise=clockwise, min_range=0.5, max_range=40.0)
    if col_shift is not None:
        kw["col_shift"] = col_shift
    return case(xyz, lab, origin=(1.5, -2.0, 0.5), **kw)


def beam_table(H, seed=5, up=0.2, down=-0.45):
    """an uneven, strictly descending table: a dense middle and sparse ends (the layout of a 64-beam sensor in miniature)"""
    rng = np.random.default_rng(seed)
    gaps = rng.uniform(0.5, 2.0, H - 1) if H > 1 else np.zeros(0)
    t = np.concatenate([[0.0], np.cumsum(gaps)])
    return up - (up - down) * (t / t[-1] if H > 1 else t)


# ---- edges ----------------------------------------------------------------------------------------------------------------------
def _neighbours(v):
    v = F(v)
    return [np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]


def edges_case(W=16, H=2):
    """fov +-0.3 with H even puts an inner edge at elevation 0 exactly; min_range 0.5 and max_range 8 have exact squares"""
    up = 0.3
    pts = []
    for r in (1.0, 3.0, 0.7):
        # on the sector edges of every W = 8 m: the axes and the diagonals, and a hair to either side of them
        for x, y in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (-1, -1), (1, -1)):
            pts.append((r * x, r * y, 0.0))                     # on the row edge at elevation 0 too
            pts.append((r * x, r * y, 0.125 * r))
            pts.append((r * x, r * y, -0.125 * r))
            for e in _neighbours(r * y)[::2]:
                pts.append((r * x, e, 0.05))
            for e in _neighbours(r * x)[::2]:
                pts.append((e, r * y, -0.05))
    # the top and bottom edges of the view: z = +-tan(fov) at D = 1, and the floats next to it; a little beyond; the zero row edge
    t = np.tan(up)
    for s in (1.0, -1.0):
        for z in _neighbours(s * t):
            pts += [(1.0, 0.0, z), (0.0, -1.0, z), (0.6, 0.8, z)]
        pts += [(2.0, 1.0, s * 2.3 * t), (2.0, 1.0, s * 2.2 * t)]
    for z in _neighbours(0.0):
        pts += [(2.0, 0.5, z), (-1.0, 2.0, z)]
    # the vertical axis, above and below, and the sensor itself (out of range here; edges_origin_case keeps it)
    pts += [(0.0, 0.0, 5.0), (0.0, 0.0, -5.0), (0.0, 0.0, 0.0), (-0.0, -0.0, 1.0)]
    # r2 equal to each bound: 0.25 is kept, 64 is not, the floats next to them
    for x in _neighbours(0.5) + _neighbours(8.0):
        pts += [(x, 0.0, 0.0), (0.0, -x, 0.0)]
    pts += [(0.3, 0.4, 0.0), (4.8, 6.4, 0.0), (-4.8, -6.4, 0.0)]
    xyz = np.array(pts, dtype=F)
    lab = (1 + np.arange(len(xyz)) % 7).astype(np.uint32)
    return case(xyz, lab, width=W, height=H, fov_up=up, fov_down=-up, min_range=0.5, max_range=8.0)


def edges_origin_case():
    """min_range = 0: the sensor's own position is kept and, with D = 0 and Zs = 0, inside the view"""
    c = edges_case(24, 4)
    c["p"]["min_range"] = 0.0
    return c


def mixed_case():
    """NaN / Inf points mixed in, with an origin and a beam table"""
    xyz, lab = sphere(1500, 9, origin=(0.5, 0.25, -1.0))
    xyz[[0, 17, 400, 1499], [0, 1, 2, 0]] = [np.nan, np.inf, -np.inf, np.nan]
    xyz[700] = np.nan
    return case(xyz, lab, origin=(0.5, 0.25, -1.0), beam=beam_table(7), width=40, height=7, min_range=0.5, max_range=30.0)


def one_point_case():
    return case([[3.0, -1.0, -0.4]], [5], width=16, height=4)


def all_dropped_case():
    xyz, lab = sphere(300, 3, r_lo=0.01, r_hi=0.4)
    return case(xyz, lab, width=16, height=4)


def not_finite_only_case():
    return case(np.full((5, 3), np.nan), [1, 2, 3, 4, 5], width=16, height=4)


# ---- winner ---------------------------------------------------------------------------------------------------------------------
def winner_case():
    """W = 16, H = 1: duplicates, mirror images in z (equal r2, one column, one row), a nearer point that comes later"""
    pts = [(3.0, 1.0, 0.5), (3.0, 1.0, -0.5), (3.0, 1.0, 0.5), (3.0, 1.0, 0.5),      # column A: index 0 wins
           (-2.0, 1.0, 0.25), (-2.0, 1.0, -0.25), (-1.0, 0.5, 0.125),                 # column B: index 6 is nearer
           (1.0, -4.0, 0.0), (1.0, -4.0, 0.0), (-1.0, -4.0, 1.0), (-1.0, -4.0, -1.0)]
    return case(pts, np.arange(1, len(pts) + 1), width=16, height=1, fov_up=0.6, fov_down=-0.6)


def crowd_case(n=2000):
    """n points in one pixel of 16 x 2, a few of them duplicates of the nearest"""
    rng = np.random.default_rng(21)
    az, el, r = rng.uniform(0.05, 0.3, n), rng.uniform(0.02, 0.25, n), rng.uniform(2.0, 30.0, n)
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], axis=1).astype(F)
    near = int(np.argmin((xyz.astype(np.float64) ** 2).sum(axis=1)))
    xyz[[1500, 1900]] = xyz[near]
    return case(xyz, rng.integers(1, 5, n), width=16, height=2, fov_up=0.3, fov_down=-0.3), near


# ---- vote -----------------------------------------------------------------------------------------------------------------------
def vote_case(seed=31, n=2500, W=24, H=5, labelled=True):
    """a cloud several points deep per pixel and a picture of classes 0 .. 3: empty classes, ties and occlusions everywhere,
    windows over the column seam and at rows 0 and H - 1"""
    xyz, lab = sphere(n, seed, r_lo=1.0, r_hi=12.0, el_lo=-0.5, el_hi=0.12)
    rng = np.random.default_rng(seed + 1)
    c = case(xyz, lab if labelled else None, width=W, height=H, min_range=0.5, max_range=40.0, max_dist_sq=9.0)
    c["pixel_label"] = rng.integers(0, 4, (H, W)).astype(np.uint32)
    return c


def tie_case(clockwise):
    """W = 16, H = 1.  P = (5, 0, 0) alone in its pixel (sector 0: it lies on that sector's lower edge); A = (4, 3, 0) in sector 1
    and B = (4, -3, 0) in sector 14 -- across the column seam with col_shift = 0 -- both at d2 = 10 from P exactly, both inside a
    window of 5.  The picture: P's pixel 0, A's 9, B's 7."""
    c = case([(5.0, 0.0, 0.0), (4.0, 3.0, 0.0), (4.0, -3.0, 0.0)], [1, 2, 3], width=16, height=1, fov_up=0.5, fov_down=-0.5, clockwise=clockwise,
             col_shift=0, window=5, max_dist_sq=10.5)
    return c


# ---- a scan of a box room -------------------------------------------------------------------------------------------------------
ROOM = (6.0, 4.0, 1.2, 2.0)  # half length (x), half width (y), floor below and ceiling above the sensor


def room_case(W=256, H=64):
    """a 64-beam sensor at the origin of a box room, one ray through the middle of every pixel of the default field of view; the
    class of a point is the face it lies on: 1 .. 4 the walls (+x, -x, +y, -y), 5 the floor, 6 the ceiling"""
    import range_ref
    p = range_ref.params(width=W, height=H, clockwise=0, col_shift=0, min_range=0.5, max_range=120.0)
    a = range_ref.edge_angles(p)
    el = 0.5 * (a[:-1] + a[1:])
    az = 2.0 * np.pi * (np.arange(W) + 0.5) / W
    d = np.stack([np.outer(np.cos(el), np.cos(az)), np.outer(np.cos(el), np.sin(az)), np.outer(np.sin(el), np.ones(W))], axis=2).reshape(-1, 3)
    hx, hy, zf, zc = ROOM
    with np.errstate(divide="ignore"):
        t = np.stack([hx / d[:, 0], -hx / d[:, 0], hy / d[:, 1], -hy / d[:, 1], -zf / d[:, 2], zc / d[:, 2]], axis=1)
    t[t <= 0] = np.inf
    face = np.argmin(t, axis=1)
    xyz = (d * t[np.arange(len(d)), face][:, None]).astype(F)
    c = case(xyz, None, width=W, height=H, clockwise=0, col_shift=0, min_range=0.5, max_range=120.0, window=5, k=5, max_dist_sq=1.0)
    c["face"] = (face + 1).astype(np.uint32)
    return c
