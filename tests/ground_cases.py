"""The inputs of the sicp_segment_ground tests, from fixed seeds: case(name) -> {"xyz", "labels", "mask", "origin", "ring_edge",
"params"}, params being keywords of ground_ref.segment_ground (and, but for `ignore`, fields of sicp_ground_params);
reference(name) is the restatement's answer, computed once.  The small cases live on a 4 x 4 grid of 5 m rings from 1 m and
quarter-circle sectors, so that a cell is easy to aim at: patch(ring, sector) scatters points inside one."""
import functools

import numpy as np

import ground_ref

SMALL = dict(n_rings=4, n_sectors=4, min_range=1.0, max_range=21.0)
CELL_SIZES = (1, 2, 9, 10, 63, 64, 65, 128, 129, 4097)  # min_points = 10
ROAD = -1.73
BIG = 262145 + 4097


def _params(**over):
    p = dict(ground_ref.DEFAULTS)
    p.update(over)
    p["ignore"] = tuple(p["ignore"])
    return p


def _case(xyz, params, labels=None, mask=None, origin=None, ring_edge=None):
    return {"xyz": np.ascontiguousarray(xyz, np.float32), "labels": None if labels is None else np.ascontiguousarray(labels, np.uint32),
            "mask": None if mask is None else np.ascontiguousarray(mask, np.uint8), "origin": origin, "ring_edge": ring_edge, "params": params}


def patch(rng, n, ring, sector, z=ROAD, noise=0.02, grid=SMALL, tilt=(0.0, 0.0)):
    """n points inside cell (ring, sector) of a uniform grid, half a metre and ten degrees clear of its borders, on the plane
    z + tilt . (x, y) with Gaussian noise"""
    R, S = grid["n_rings"], grid["n_sectors"]
    w = (grid["max_range"] - grid["min_range"]) / R
    r = rng.uniform(grid["min_range"] + ring * w + 0.1 * w, grid["min_range"] + (ring + 1) * w - 0.1 * w, n)
    step = 360.0 / S
    a = np.deg2rad(rng.uniform(sector * step + 0.12 * step, (sector + 1) * step - 0.12 * step, n))
    x, y = r * np.cos(a), r * np.sin(a)
    return np.stack([x, y, z + tilt[0] * x + tilt[1] * y + noise * rng.normal(size=n)], axis=1)


def _shuffled(rng, parts, labels=None):
    xyz = np.concatenate(parts)
    o = rng.permutation(len(xyz))
    return (xyz[o], None) if labels is None else (xyz[o], np.concatenate(labels)[o])


def _cell_sizes():
    """ten cells of 1, 2, min_points - 1, min_points, 63, 64, 65, 128, 129 and 4 097 members, a few object points over each"""
    rng = np.random.default_rng(11)
    parts = []
    for k, n in enumerate(CELL_SIZES):
        ring, sector = k % 4, k // 4
        parts.append(patch(rng, n, ring, sector, tilt=(0.02, -0.01)))
        if n >= 63:
            parts[-1][::7, 2] += rng.uniform(0.4, 1.5, len(parts[-1][::7]))
    xyz, _ = _shuffled(rng, parts)
    return _case(xyz, _params(**SMALL))


def _seeds_scene():
    rng = np.random.default_rng(12)
    parts = [patch(rng, 30, 0, 0), patch(rng, 200, 1, 1, tilt=(0.05, 0.0)), patch(rng, 64, 2, 2), patch(rng, 40, 1, 1, z=-0.5, noise=0.3)]
    return _shuffled(rng, parts)[0]


def _n_lpr(n_lpr):
    """cells of 30, 64 and 240 members: n_lpr = 64 is larger than the first and exactly the second"""
    return _case(_seeds_scene(), _params(n_lpr=n_lpr, **SMALL))


def _n_iter(n_iter):
    rng = np.random.default_rng(13)
    parts = [patch(rng, 300, r, s, tilt=(0.08, 0.03), noise=0.05) for r in range(3) for s in range(4)]
    parts += [patch(rng, 60, r, s, z=-1.0, noise=0.4) for r in range(3) for s in range(4)]
    return _case(_shuffled(rng, parts)[0], _params(n_iter=n_iter, **SMALL))


def _lattice(x0, y0, nx, ny, z):
    u, v = np.meshgrid(np.arange(nx, dtype=np.float64) + x0, np.arange(ny, dtype=np.float64) + y0, indexing="ij")
    return np.stack([u.ravel(), v.ravel(), np.full(nx * ny, z)], axis=1)


def _equal_heights():
    """sensor_height 0.  Cell (0, 0): a lattice at one height -- every z ties, Q has a zero row.  Cell (0, 1): twelve collinear
    points at one height -- two zero eigenvalues.  Cell (0, 2): twelve identical points -- Q = 0.  Cell (0, 3): a lattice whose
    heights are -0.0 and +0.0 in turn.  Cell (1, 0): twelve points on a vertical line -- the
    zero eigenvalues of x and y tie, u = (0, 1, 0), uz = 0 exactly: NOT_UPRIGHT."""
    a = _lattice(1.5, 1.5, 3, 4, -0.25)
    b = np.stack([-1.5 - 0.125 * np.arange(12), 1.5 + 0.25 * np.arange(12), np.full(12, 0.5)], axis=1)
    c = np.tile([[-2.0, -3.0, 0.125]], (12, 1))
    d = _lattice(1.5, -3.5, 4, 3, 0.0)
    d[::2, 2] = -0.0
    e = np.stack([np.full(12, 7.0), np.full(12, 3.0), -0.5 + 0.0625 * np.arange(12)], axis=1)
    return _case(np.concatenate([a, b, c, d, e]), _params(sensor_height=0.0, min_points=10, **SMALL))


def _boundaries():
    """rings [0, 10), [10, 20): points exactly on a ring edge and one float ulp either side, on edge2[0] (the origin) and
    edge2[R]; on the sector boundaries, the wrap S-1 -> 0 and both dy == 0 half-lines among them; over a ground that fills
    every cell"""
    rng = np.random.default_rng(14)
    grid = dict(n_rings=2, n_sectors=8, min_range=0.0, max_range=20.0, elevation_rings=2)
    parts = [patch(rng, 40, r, s, grid=grid) for r in range(2) for s in range(8)]
    f = np.float32
    up, dn = (lambda v: np.nextafter(f(v), f(np.inf))), (lambda v: np.nextafter(f(v), f(-np.inf)))
    z = ROAD
    edge = []
    for r in (10.0, 20.0):
        edge += [[r, 0, z], [up(r), 0, z], [dn(r), 0, z], [0, r, z], [0, up(r), z], [0, dn(r), z], [-r, 0, z], [0.6 * r, 0.8 * r, z],
                 [f(0.6 * r), dn(0.8 * r), z], [f(0.6 * r), up(0.8 * r), z]]
    tiny = f(1e-30)
    edge += [[0, 0, z], [0.0, -0.0, z], [-0.0, 0.0, z], [tiny, 0, z], [0, tiny, z], [-tiny, 0, z], [0, -tiny, z]]
    for r in (3.0, 13.0):  # the eight sector boundaries, and a hair to either side of each
        for k in range(8):
            a = np.deg2rad(45.0 * k)
            x, y = f(r * np.cos(a)), f(r * np.sin(a))
            edge += [[x, y, z], [x, up(y), z], [x, dn(y), z], [up(x), y, z], [dn(x), y, z]]
        edge += [[r, -tiny, z], [r, tiny, z], [-r, -tiny, z], [-r, tiny, z], [r, -0.0, z], [-r, -0.0, z]]
    return _case(np.concatenate([np.concatenate(parts), np.array(edge, np.float64)]), _params(**grid))


RING_EDGE = (1.0, 2.5, 6.0, 21.0)


def _custom_edges():
    """a caller's ring table, narrow near the sensor; points on every edge of it"""
    rng = np.random.default_rng(15)
    r = rng.uniform(1.0, 21.0, 1500)
    a = rng.uniform(0, 2 * np.pi, 1500)
    xyz = np.stack([r * np.cos(a), r * np.sin(a), ROAD + 0.02 * rng.normal(size=1500)], axis=1)
    on = [[e, 0, ROAD] for e in RING_EDGE] + [[0, -e, ROAD] for e in RING_EDGE] + [[np.nextafter(np.float32(1.0), np.float32(0)), 0, ROAD]]
    return _case(np.concatenate([xyz, np.array(on)]), _params(n_rings=3, n_sectors=6, min_range=0.5, max_range=30.0, elevation_rings=1), ring_edge=np.array(RING_EDGE))


def _grid_1x4():
    rng = np.random.default_rng(16)
    grid = dict(n_rings=1, n_sectors=4, min_range=1.0, max_range=21.0)
    parts = [patch(rng, 150, 0, s, grid=grid, tilt=(0.01 * s, 0.0)) for s in range(4)]
    return _case(_shuffled(rng, parts)[0], _params(elevation_rings=1, **grid))


def _grid_64x256():
    """the finest grid on the sloped street: most cells are empty or too few"""
    xyz, _ = sloped_street()
    return _case(xyz, _params(n_rings=64, n_sectors=256, elevation_rings=16))


ONE_CELL = dict(n_rings=1, n_sectors=4, min_range=1.0, max_range=21.0, n_iter=1, elevation_rings=0)
F32 = np.float32


def _th_dist_edge():
    """an 8 x 8 integer lattice at z = -2 in one cell: its fit is g = (6.5, 4.5, -2), u = (0, 0, 1) exactly.  Points at
    th_dist = 0.25 above it (outside: the test is <), one float ulp below that (inside) and one beyond (outside)"""
    at = F32(-1.75)
    extra = [[5.0, 3.0, at], [6.0, 4.0, np.nextafter(at, F32(-3))], [7.0, 5.0, np.nextafter(at, F32(0))]]
    xyz = np.concatenate([_lattice(3.0, 1.0, 8, 8, -2.0), np.array(extra, np.float64)])
    return _case(xyz, _params(th_dist=0.25, th_seeds=0.125, **ONE_CELL))


def _th_seeds_edge():
    """the lattice again, lpr = -2: points at lpr + th_seeds = -1.75 (no seed), one ulp below (a seed) and one beyond (none):
    n_fit says who was a seed"""
    at = F32(-1.75)
    extra = [[5.0, 3.0, at], [6.0, 4.0, np.nextafter(at, F32(-3))], [7.0, 5.0, np.nextafter(at, F32(0))]]
    xyz = np.concatenate([_lattice(3.0, 1.0, 8, 8, -2.0), np.array(extra, np.float64)])
    return _case(xyz, _params(th_dist=0.5, th_seeds=0.25, **ONE_CELL))


def _below_edge():
    """sensor_height 1.75, max_below 1: the bound is -2.75 exactly.  A point on it is a candidate, one ulp under it is counted
    in n_below, and so are deeper ones"""
    rng = np.random.default_rng(17)
    at = F32(-2.75)
    extra = [[4.0, 2.0, at], [5.0, 3.0, np.nextafter(at, F32(-3))], [6.0, 2.0, np.nextafter(at, F32(0))], [5.0, 5.0, -4.0], [6.0, 6.0, -30.0]]
    xyz = np.concatenate([patch(rng, 100, 0, 0, z=-1.75), np.array(extra, np.float64)])
    return _case(xyz, _params(sensor_height=1.75, **SMALL))


STATUS_GRID = dict(n_rings=8, n_sectors=8, min_range=1.0, max_range=41.0)


def _statuses():
    """one cell each, on 8 x 8 cells with max_thickness 0.05 and n_lpr 3:
    (0, 0) GROUND; (1, 0) five low points under seven 1 m higher: TOO_FEW at the first set; (2, 0) a lattice whose heights
    alternate between -2 and -1.6: all seeds, a flat fit half way, th_dist keeps the lower six: TOO_FEW at the second set;
    (1, 1) a wall foot: NOT_UPRIGHT; (1, 2) a flat roof at +0.2 in ring 1: TOO_HIGH; (5, 2) the same roof in a ring >=
    elevation_rings: GROUND; (1, 3) 0.1 m of noise: TOO_THICK; (2, 3) and (3, 3): points over no ground model of their own"""
    rng = np.random.default_rng(18)
    g = STATUS_GRID
    ok = patch(rng, 200, 0, 0, grid=g)
    few1 = np.concatenate([patch(rng, 5, 1, 0, z=-2.0, noise=0.0, grid=g), patch(rng, 7, 1, 0, z=-1.0, noise=0.0, grid=g)])
    few2 = _lattice(12.0, 3.0, 4, 3, -2.0)
    few2[(np.arange(12) // 3 + np.arange(12) % 3) % 2 == 1, 2] = -1.6
    wall = np.stack([np.full(120, 3.0), rng.uniform(6.5, 9.0, 120), rng.uniform(-1.7, 0.5, 120)], axis=1)
    roof1 = patch(rng, 150, 1, 2, z=0.2, grid=g)
    roof5 = patch(rng, 150, 5, 2, z=0.2, grid=g)
    thick = patch(rng, 300, 1, 3, noise=0.1, grid=g)
    over = np.concatenate([patch(rng, 6, 2, 3, z=-1.0, noise=0.3, grid=g), patch(rng, 4, 3, 3, z=0.5, noise=0.3, grid=g)])
    xyz = np.concatenate([ok, few1, few2, wall, roof1, roof5, thick, over])
    return _case(xyz, _params(max_thickness=0.05, n_lpr=3, th_dist=0.1, **g))


STATUS_CELLS = {(0, 0): ground_ref.GROUND, (1, 0): ground_ref.TOO_FEW, (2, 0): ground_ref.TOO_FEW, (1, 1): ground_ref.NOT_UPRIGHT,
                (1, 2): ground_ref.TOO_HIGH, (5, 2): ground_ref.GROUND, (1, 3): ground_ref.TOO_THICK, (2, 3): ground_ref.TOO_FEW,
                (3, 3): ground_ref.TOO_FEW}


def _height_fallback():
    """sector 0: a ground in ring 0, nothing in ring 1, five points in ring 2 that take ring 0's model, two rings inward; sector
    1: five points in ring 1 and nothing inward of them: NaN; sector 2: a point of a GROUND cell that the mask leaves out still
    has a height"""
    rng = np.random.default_rng(19)
    parts = [patch(rng, 120, 0, 0, tilt=(0.03, 0.0)), patch(rng, 5, 2, 0, z=-0.5, noise=0.5), patch(rng, 5, 1, 1, z=-1.0, noise=0.5),
             patch(rng, 80, 1, 2), patch(rng, 10, 1, 2, z=0.0, noise=0.5)]
    xyz = np.concatenate(parts)
    mask = np.ones(len(xyz), np.uint8)
    mask[-10:] = 0
    return _case(xyz, _params(**SMALL), mask=mask)


def _labelled_scene(seed, n=900):
    rng = np.random.default_rng(seed)
    r, a = rng.uniform(1.0, 21.0, n), rng.uniform(0, 2 * np.pi, n)
    high = rng.random(n) < 0.25
    z = np.where(high, rng.uniform(-1.2, 1.0, n), ROAD + 0.03 * rng.normal(size=n) + 0.02 * r * np.cos(a))
    lab = np.where(high, 2 + rng.integers(0, 2, n), 1).astype(np.uint32)
    return np.stack([r * np.cos(a), r * np.sin(a), z], axis=1).astype(np.float32), lab


def _nan_mix():
    xyz, lab = _labelled_scene(20)
    xyz[1] = np.nan
    xyz[40, 2] = np.inf
    xyz[333, 0] = -np.inf
    xyz[-1] = np.nan
    return _case(xyz, _params(**SMALL), labels=lab)


def _ignore_mask():
    xyz, lab = _labelled_scene(21)
    lab[::13] = 7
    mask = (np.arange(len(xyz)) % 5 != 2).astype(np.uint8)
    return _case(xyz, _params(ignore=(3, 7), **SMALL), labels=lab, mask=mask)


def _interleaved():
    """three interleaved labels, label 3 on five points only: a label-grouped cloud lies on the device in another order"""
    xyz, _ = _labelled_scene(22)
    lab = (1 + np.arange(len(xyz)) % 2).astype(np.uint32)
    lab[[17, 230, 411, 650, 888]] = 3
    xyz[5] = np.nan
    return _case(xyz, _params(**SMALL), labels=lab)


def _no_labels():
    return _case(_labelled_scene(23)[0], _params(**SMALL))


ORIGIN = (10.5, -3.25, 0.375)


def _origin():
    xyz, lab = _labelled_scene(24)
    return _case(xyz + np.array(ORIGIN, np.float32), _params(**SMALL), labels=lab, origin=np.array(ORIGIN))


def _no_candidates():
    """every point is outside the rings, under the road or not finite"""
    xyz, _ = _labelled_scene(25, 200)
    xyz[:100] *= np.float32(0.01)
    xyz[:100, 2] = ROAD
    xyz[100:, 2] = -9.0
    xyz[7] = np.nan
    return _case(xyz, _params(**SMALL))


@functools.lru_cache(maxsize=None)
def sloped_street():
    """(xyz [20 000, 3] float32, truth [20 000] bool): a street without labels, the sensor 1.73 m over the road at the origin.
    The road (8 m) and its sidewalks (3 m each, a 0.15 m kerb) run from x = -40 to x = 75, flat to x = 15 and rising by 8 degrees
    from there; a flat cross street 12 m wide crosses behind the sensor; the ground is sampled on a jittered 0.4 m grid (closer
    than the clustering tolerance of the recipe) but for the 3 m about the sensor that the vehicle hides; facades with gaps, cars,
    poles, foliage.  truth: road and sidewalk points."""
    rng = np.random.default_rng(7)
    slope = np.tan(np.deg2rad(8.0))
    step = 0.4

    def road_z(x):
        return ROAD + slope * np.maximum(x - 15.0, 0.0)

    def grid(x0, x1, y0, y1):
        u, v = np.meshgrid(np.arange(x0 + step / 2, x1, step), np.arange(y0 + step / 2, y1, step), indexing="ij")
        return u.ravel() + rng.uniform(-0.02, 0.02, u.size), v.ravel() + rng.uniform(-0.02, 0.02, u.size)

    x, y = grid(-40.0, 75.0, -7.0, 7.0)
    seen = x * x + y * y >= 9.0
    x, y = x[seen], y[seen]
    main = np.stack([x, y, road_z(x) + np.where(np.abs(y) > 4.0, 0.15, 0.0) + 0.015 * rng.normal(size=len(x))], axis=1)
    cross = []
    for y0, y1 in ((7.0, 35.0), (-35.0, -7.0)):
        x, y = grid(-26.0, -14.0, y0, y1)
        cross.append(np.stack([x, y, ROAD + 0.15 + 0.015 * rng.normal(size=len(x))], axis=1))
    ground = np.concatenate([main] + cross)
    objects = []
    for side in (-1.0, 1.0):  # facades 8 m long with 2 m gaps, 3.5 m high, none across the cross street
        for x0 in np.arange(-40.0, 70.0, 10.0):
            if -30.0 < x0 < -10.0:
                continue
            n = 150
            fx = rng.uniform(x0, x0 + 8.0, n)
            objects.append(np.stack([fx, np.full(n, side * 7.2), road_z(fx) + 0.15 + rng.uniform(0.0, 3.5, n)], axis=1))
    for cx, cy in ((8.0, 2.0), (20.0, -2.0), (32.0, 2.0), (44.0, -2.0), (-8.0, -2.0), (-34.0, 2.0), (56.0, 2.0)):  # cars: 4 x 1.8 x 1.3 shells
        n = 160
        p = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([2.0, 0.9, 0.65])
        face = rng.integers(0, 3, n)
        p[np.arange(n), face] = np.sign(p[np.arange(n), face]) * np.array([2.0, 0.9, 0.65])[face]
        objects.append(p + np.stack([np.full(n, cx), np.full(n, cy), road_z(np.full(n, cx) + p[:, 0]) + 0.35 + 0.65], axis=1))
    for px in np.arange(-35.0, 70.0, 9.0):  # poles on the sidewalks
        n = 40
        side = 1.0 if int(px) % 2 else -1.0
        objects.append(np.stack([px + 0.05 * rng.normal(size=n), side * 5.0 + 0.05 * rng.normal(size=n),
                                 road_z(np.full(n, px)) + 0.15 + rng.uniform(0.0, 4.0, n)], axis=1))
    objects = np.concatenate(objects)
    n_fill = 20000 - len(ground) - len(objects)
    assert n_fill >= 0, (len(ground), len(objects))
    fx = rng.uniform(-40, 70, n_fill)  # foliage over the facades
    fill = np.stack([fx, rng.choice([-7.6, 7.6], n_fill) + 0.3 * rng.normal(size=n_fill), road_z(fx) + rng.uniform(4.5, 7.0, n_fill)], axis=1)
    xyz = np.concatenate([ground, objects, fill])
    truth = np.zeros(len(xyz), bool)
    truth[:len(ground)] = True
    o = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[o], np.float32), truth[o]


def _street():
    return _case(sloped_street()[0], _params())


def _big():
    """262 145 + 4 097 points under the defaults: a gently rolling ground to 75 m, three points in five within 8 m of the sensor
    (the cells of ring 0 hold more than 4 097 each), one point in eight over the ground, a few not finite"""
    rng = np.random.default_rng(26)
    r, a = np.where(rng.random(BIG) < 0.6, rng.uniform(2.0, 8.0, BIG), rng.uniform(8.0, 85.0, BIG)), rng.uniform(0, 2 * np.pi, BIG)
    x, y = r * np.cos(a), r * np.sin(a)
    z = ROAD + 0.3 * np.sin(0.05 * x) + 0.02 * y + 0.02 * rng.normal(size=BIG)
    z[::8] += rng.uniform(0.3, 3.0, len(z[::8]))
    xyz = np.stack([x, y, z], axis=1).astype(np.float32)
    xyz[[5, 262144, 262145, BIG - 1]] = np.nan
    return _case(xyz, _params())


_CASES = {
    "cell_sizes": _cell_sizes,
    **{f"n_lpr_{k}": (lambda k=k: _n_lpr(k)) for k in (1, 20, 64)},
    **{f"n_iter_{k}": (lambda k=k: _n_iter(k)) for k in (1, 8)},
    "equal_heights": _equal_heights,
    "boundaries": _boundaries,
    "custom_edges": _custom_edges,
    "grid_1x4": _grid_1x4,
    "grid_64x256": _grid_64x256,
    "th_dist_edge": _th_dist_edge,
    "th_seeds_edge": _th_seeds_edge,
    "below_edge": _below_edge,
    "statuses": _statuses,
    "height_fallback": _height_fallback,
    "nan_mix": _nan_mix,
    "ignore_mask": _ignore_mask,
    "interleaved": _interleaved,
    "no_labels": _no_labels,
    "origin": _origin,
    "no_candidates": _no_candidates,
    "street": _street,
    "big": _big,
}
NAMES = list(_CASES)
TINY = ["equal_heights", "th_dist_edge", "th_seeds_edge", "below_edge", "statuses", "height_fallback", "n_lpr_64", "boundaries"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


def run_reference(c, **over):
    return ground_ref.segment_ground(c["xyz"], c["labels"], c["mask"], c["origin"], c["ring_edge"], **dict(c["params"], **over))


@functools.lru_cache(maxsize=None)
def reference(name):
    return run_reference(case(name))
