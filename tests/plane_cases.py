"""The inputs of the sicp_segment_planes tests, from fixed seeds: case(name) -> {"xyz", "labels", "mask", "params"}, params being
the keywords of plane_ref.segment_planes (and, but for `ignore` and `axis`, the fields of sicp_plane_params); reference(name) is
the restatement's answer, computed once."""
import functools

import numpy as np

import cluster_cases
import plane_ref

TILE = plane_ref.TILE
GROUP = plane_ref.HYP_GROUP
TILE_SIZES = (TILE - 1, TILE, TILE + 1, 3 * TILE + 77)
HYPOTHESES = (1, GROUP - 1, GROUP, GROUP + 1, 4096)
STREET_T = 0.1
Z, Y = (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)


def _params(**over):
    p = dict(plane_ref.DEFAULTS)
    p.update(over)
    p["ignore"] = tuple(p["ignore"])
    return p


def _case(xyz, labels, params, mask=None):
    return {"xyz": np.ascontiguousarray(xyz, np.float32), "labels": None if labels is None else np.ascontiguousarray(labels, np.uint32),
            "mask": mask, "params": params}


def _street(refine, axis):
    """the cluster's 20 K-point street scan: the road, then whatever else is flat"""
    xyz, lab = cluster_cases._street_scan()
    extra = {} if axis is None else dict(axis=axis, min_cos=0.95)
    return _case(xyz, lab, _params(distance_threshold=STREET_T, num_hypotheses=256, max_planes=4, refine=refine, **extra))


def _scene(seed, n, inlier_share=0.7, noise=0.02):
    """a tilted noisy plane in a 10 m box of uniform points, shuffled; labels 1 (plane) / 2 / 3"""
    rng = np.random.default_rng(seed)
    k = int(n * inlier_share)
    uv = rng.uniform(-5, 5, (k, 2))
    plane = np.stack([uv[:, 0], uv[:, 1], 0.3 * uv[:, 0] - 0.1 * uv[:, 1] + 1.0 + noise * rng.normal(size=k)], axis=1)
    xyz = np.concatenate([plane, rng.uniform(-5, 5, (n - k, 3))])
    lab = np.concatenate([np.ones(k, np.uint32), (2 + rng.integers(0, 2, n - k)).astype(np.uint32)])
    o = rng.permutation(n)
    return xyz[o].astype(np.float32), lab[o]


def _room_corner():
    """three orthogonal noisy planes of 300 points each and 20 stray points: three planes, the fourth round is scored and stops
    at min_inliers"""
    rng = np.random.default_rng(5)
    uv = rng.uniform(0.2, 3.0, (3, 300, 2))
    w = 0.01 * rng.normal(size=(3, 300))
    floor = np.stack([uv[0, :, 0], uv[0, :, 1], w[0]], axis=1)
    wall_x = np.stack([w[1], uv[1, :, 0], uv[1, :, 1]], axis=1)
    wall_y = np.stack([uv[2, :, 0], w[2], uv[2, :, 1]], axis=1)
    stray = rng.uniform(0.5, 3.0, (20, 3))
    xyz = np.concatenate([floor, wall_x, wall_y, stray])
    lab = np.concatenate([np.full(300, k, np.uint32) for k in (1, 2, 3)] + [np.full(20, 4, np.uint32)])
    o = rng.permutation(len(xyz))
    return _case(xyz[o], lab[o], _params(distance_threshold=0.05, num_hypotheses=128, max_planes=4, min_inliers=100))


def _three_points():
    xyz = np.array([[0.5, 0.25, 1.0], [2.0, -1.0, 0.5], [-1.5, 3.0, 0.75]], np.float32)
    return _case(xyz, np.array([1, 1, 1], np.uint32), _params(num_hypotheses=16, min_inliers=3))


def _tile(n):
    """the score kernel's tile at n candidates exactly: every point finite and unmasked, but for the several-tile size, which has
    masked holes and a non-finite point"""
    xyz, lab = _scene(200 + n % 89, n)
    mask = None
    if n > TILE + 1:
        mask = np.ones(n, np.uint8)
        mask[5::11] = 0
        xyz[7] = np.nan
    return _case(xyz, lab, _params(distance_threshold=0.05, num_hypotheses=GROUP + 1, max_planes=2, min_inliers=50), mask)


def _hypotheses(H):
    xyz, lab = _scene(300, 500)
    return _case(xyz, lab, _params(distance_threshold=0.05, num_hypotheses=H, max_planes=2, min_inliers=3))


def _degenerate(which):
    """no three points span a plane: no valid hypothesis, 0 planes, SICP_OK"""
    if which == "identical":
        xyz = np.tile(np.array([[1.5, -2.25, 0.75]], np.float32), (200, 1))
    elif which == "collinear":
        xyz = (np.arange(200)[:, None] * np.array([0.5, 0.25, -1.0]) + np.array([3.0, 1.0, 2.0])).astype(np.float32)
    else:
        xyz = np.tile(np.array([[1.5, -2.25, 0.75], [0.5, 4.0, -1.0]], np.float32), (100, 1))
    return _case(xyz, None, _params(num_hypotheses=GROUP, min_inliers=3))


def _lattice_ties():
    """a 6 x 6 integer lattice in the plane z = 2: every valid hypothesis holds every point exactly, so all of them tie and the
    first valid h wins; many triples are collinear"""
    g = np.arange(6, dtype=np.float32)
    u, v = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([u.ravel(), v.ravel(), np.full(36, 2.0, np.float32)], axis=1)
    return _case(xyz, None, _params(num_hypotheses=200, min_inliers=3, refine=0))


def _threshold_edge():
    """an 8 x 8 integer lattice in the plane z = 0, one point exactly t = 0.25 above it and one a float ulp beyond: with refine = 0
    the lattice's plane has an integer normal (0, 0, nz), e e = nz nz / 16 = (t t) nn for the first -- inside -- and above for the
    second"""
    g = np.arange(8, dtype=np.float32)
    u, v = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([u.ravel(), v.ravel(), np.zeros(64, np.float32)], axis=1)
    at = np.float32(0.25)
    xyz = np.concatenate([xyz, [[3.0, 4.0, at], [5.0, 2.0, np.nextafter(at, np.float32(1))]]]).astype(np.float32)
    return _case(xyz, None, _params(distance_threshold=0.25, num_hypotheses=GROUP, min_inliers=10, refine=0))


AT_T, BEYOND_T = 64, 65  # the two points of "threshold_edge"


def _nan_mix():
    xyz, lab = _scene(310, 700)
    xyz[1] = np.nan
    xyz[40, 2] = np.inf
    xyz[333, 0] = -np.inf
    xyz[-1] = np.nan
    return _case(xyz, lab, _params(distance_threshold=0.05, num_hypotheses=100, max_planes=2, min_inliers=30))


def _ignore_mask():
    xyz, lab = _scene(320, 900)
    mask = (np.arange(900) % 5 != 2).astype(np.uint8)
    return _case(xyz, lab, _params(distance_threshold=0.05, num_hypotheses=100, max_planes=2, min_inliers=30, ignore=(3, 7)), mask)


def _interleaved():
    """three interleaved labels, label 3 on five points only: a label-grouped cloud lies on the device in another order"""
    xyz, lab = _scene(330, 900)
    lab = (1 + np.arange(900) % 2).astype(np.uint32)
    lab[[17, 230, 411, 650, 888]] = 3
    return _case(xyz, lab, _params(distance_threshold=0.05, num_hypotheses=100, max_planes=3, min_inliers=30, axis=(0.3, -0.1, -1.0), min_cos=0.9))


def _no_labels():
    xyz, _ = _scene(340, 800)
    return _case(xyz, None, _params(distance_threshold=0.05, num_hypotheses=100, max_planes=2, min_inliers=30))


_CASES = {
    **{f"street_refine{r}_{name}": (lambda r=r, axis=axis: _street(r, axis)) for r in (0, 1) for name, axis in (("free", None), ("z", Z), ("y", Y))},
    "room_corner": _room_corner,
    "three_points": _three_points,
    **{f"tile_{n}": (lambda n=n: _tile(n)) for n in TILE_SIZES},
    **{f"hypotheses_{H}": (lambda H=H: _hypotheses(H)) for H in HYPOTHESES},
    "identical": lambda: _degenerate("identical"),
    "collinear": lambda: _degenerate("collinear"),
    "two_points": lambda: _degenerate("two_points"),
    "lattice_ties": _lattice_ties,
    "threshold_edge": _threshold_edge,
    "nan_mix": _nan_mix,
    "ignore_mask": _ignore_mask,
    "interleaved": _interleaved,
    "no_labels": _no_labels,
}
NAMES = list(_CASES)
STREET = [n for n in NAMES if n.startswith("street")]
DEGENERATE = ["identical", "collinear", "two_points"]


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return plane_ref.segment_planes(c["xyz"], c["labels"], c["mask"], **c["params"])


@functools.lru_cache(maxsize=None)
def unlabelled_street():
    """the street scan without labels and what the recipe gives on it ("Planes of a cloud"): the ground by
    segment_planes(axis = z), the rest clustered"""
    xyz, _ = cluster_cases._street_scan()
    return np.ascontiguousarray(xyz, np.float32)


RECIPE_PLANE = dict(distance_threshold=0.2, axis=Z, min_cos=0.95, num_hypotheses=256, max_planes=1)
RECIPE_CLUSTER = dict(tolerance=0.5, min_points=10, max_points=0, same_label=0, ignore=())
