"""The inputs of the sicp_filter tests, from fixed seeds: case(name) -> {"xyz", "labels", "mask", "params"}, params being the
keywords of filter_ref.filter (and, but for the lists, the fields of sicp_filter_params); reference(name) is the restatement's
answer, computed once.  small(name) cuts a case down to what the O(n^2) check of the restatement can afford."""
import functools

import numpy as np

import cluster_cases
import filter_ref

R = cluster_cases.T  # the radius of every radius case: the tolerance of the cluster's generators
MEAN_KS = (1, 3, 4, 19, 20, 31)  # the lists are mean_k + 1 long: they cross the search's list lengths 4, 20 and 32
TREE_SIZES = (filter_ref.TREE_RUN - 1, filter_ref.TREE_RUN, filter_ref.TREE_RUN + 1, 3 * filter_ref.TREE_RUN + 77)


def _params(mean_k=0, std_mul=2.0, radius=0.0, min_neighbors=2, drop=(), protect=()):
    return dict(mean_k=mean_k, std_mul=std_mul, radius=radius, min_neighbors=min_neighbors, drop=tuple(drop), protect=tuple(protect))


def _case(xyz, labels, params, mask=None):
    return {"xyz": np.ascontiguousarray(xyz, np.float32), "labels": None if labels is None else np.ascontiguousarray(labels, np.uint32),
            "mask": mask, "params": params}


@functools.lru_cache(maxsize=None)
def _street_scan():
    """the cluster's 20 K-point street scan with 60 isolated points planted above and beside it, shuffled in; label 9 marks them
    for the tests (the filter does not look at it)"""
    xyz, lab = cluster_cases._street_scan()
    rng = np.random.default_rng(71)
    stray = np.stack([rng.uniform(-35, 35, 60), rng.uniform(-12, 12, 60), rng.uniform(6, 25, 60)], axis=1).astype(np.float32)
    xyz = np.concatenate([xyz, stray])
    lab = np.concatenate([lab, np.full(60, 9, np.uint32)])
    o = rng.permutation(len(xyz))
    return xyz[o], lab[o]


def _street(which):
    xyz, lab = _street_scan()
    if which == "stat":
        return _case(xyz, lab, _params(mean_k=20, protect=(1,)))
    if which == "radius":
        return _case(xyz, lab, _params(radius=R, min_neighbors=2, drop=(3,)))
    mask = (np.arange(len(xyz)) % 7 != 3).astype(np.uint8)
    return _case(xyz, lab, _params(mean_k=20, std_mul=1.0, radius=R, min_neighbors=3, drop=(4,), protect=(1,)), mask)


def _cloud(seed, n):
    """a 6 m box of uniform points with a denser core: every mean distance differs"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-3, 3, (n, 3))
    xyz[: n // 3] *= 0.2
    return xyz.astype(np.float32), (1 + rng.integers(0, 3, n)).astype(np.uint32)


def _mean_k(k):
    xyz, lab = _cloud(80 + k, 150)
    return _case(xyz, lab, _params(mean_k=k, std_mul=1.0))


def _exact_count(k, missing=0):
    """mean_k + 1 - missing finite points among non-finite ones"""
    xyz, lab = _cloud(90 + k, k + 1 - missing + 3)
    xyz[1] = np.nan
    xyz[2, 2] = np.inf
    xyz[-1, 0] = -np.inf
    return _case(xyz, lab, _params(mean_k=k, std_mul=0.5))


def _duplicates():
    """every point of a small cloud five times over (m = 0 with mean_k = 4), and some single points"""
    xyz, lab = _cloud(61, 40)
    xyz = np.concatenate([np.repeat(xyz[:30], 5, axis=0), xyz[30:]])
    lab = np.concatenate([np.repeat(lab[:30], 5), lab[30:]])
    o = np.random.default_rng(62).permutation(len(xyz))
    return _case(xyz[o], lab[o], _params(mean_k=4, std_mul=1.0, radius=0.3, min_neighbors=4))


def _nan_mix():
    c = cluster_cases.case("nan_mix")
    return _case(c["xyz"], c["labels"], _params(mean_k=8, std_mul=1.0, radius=0.15, min_neighbors=6, protect=(9,)))


def _tree(n):
    """the tree sum at n points, with masked, dropped and protected holes and a non-finite point"""
    xyz, lab = _cloud(100 + n % 97, n)
    mask = np.ones(n, np.uint8)
    mask[5::11] = 0
    mask[n - 1] = 1
    xyz[7] = np.nan
    return _case(xyz, lab, _params(mean_k=6, std_mul=1.5, drop=(3,), protect=(2,)), mask)


def _two_points():
    """m_0 = m_1 = threshold exactly: both kept"""
    xyz = np.array([[0.1, 0.2, 0.3], [0.7, -0.4, 1.9]], np.float32)
    return _case(xyz, np.array([1, 1], np.uint32), _params(mean_k=1, std_mul=0.0))


def _rectangles(a, b, count):
    """`count` far-apart a x b rectangles on exact coordinates: with mean_k = 3 every corner has the same m, so the variance is
    zero in real numbers and whatever the roundings of S1 and S2 leave in double"""
    corner = np.array([[0, 0, 0], [a, 0, 0], [0, b, 0], [a, b, 0]], np.float64)
    xyz = np.concatenate([corner + np.array([64.0 * i, 0, 0]) for i in range(count)])
    return _case(xyz, None, _params(mean_k=3, std_mul=1.0))


def _clamped():
    """found by search_clamped(): the raw variance is below zero and rule 3 clamps it"""
    return _rectangles(*CLAMPED)


CLAMPED = (0.5, 1.25, 3)


def search_clamped():
    """the first (a, b, count) whose raw variance rounds below zero, or None"""
    for count in (3, 5, 6, 7, 9, 11, 13):
        for a in (0.75, 0.5, 1.5, 0.625, 1.125):
            for b in (1.25, 1.0, 0.875, 1.75, 2.5):
                c = _rectangles(a, b, count)
                if filter_ref.filter(c["xyz"], None, **c["params"])["raw_variance"] < 0.0:
                    return a, b, count
    return None


def _radius_edge():
    """pairs exactly at r (not neighbours) and one ulp inside (neighbours), far from each other"""
    r = np.float32(R)
    inside = np.nextafter(r, np.float32(0))
    xyz = np.array([[0, 0, 0], [r, 0, 0], [0, 10, 0], [inside, 10, 0], [3, 20, 0], [3, 20, -r], [3, 30, 0], [3, 30, -inside]], np.float32)
    return _case(xyz, None, _params(radius=R, min_neighbors=1))


def _faces():
    """the cluster's pairs T (1 -+ 2^-20) apart across cell faces, edges and corners at every magnitude; labels play no part here,
    so the pairs about one corner see each other: min_neighbors lies above every count and neighbors shows each pair's decision"""
    c = cluster_cases.case("faces")
    return _case(c["xyz"], c["labels"], _params(radius=R, min_neighbors=12))


def _dense():
    """5000 points in a fifth of a cell and one point three radii away: neighbors saturates at min_neighbors"""
    c = cluster_cases.case("dense")
    return _case(c["xyz"], c["labels"], _params(radius=R, min_neighbors=7))


def _interleaved():
    """three interleaved labels, label 3 on five points only: fewer than mean_k + 1, so its segment of a label-grouped cloud
    pads its lists"""
    xyz, lab = _cloud(55, 900)
    lab = (1 + np.arange(900) % 2).astype(np.uint32)
    lab[[17, 230, 411, 650, 888]] = 3
    return _case(xyz, lab, _params(mean_k=8, std_mul=1.0, radius=0.4, min_neighbors=3, protect=(3,)))


def _select(which):
    xyz, lab = _cloud(57, 300)
    xyz[11] = np.nan
    mask = (np.arange(300) % 3 != 1).astype(np.uint8)
    if which == "mask":
        return _case(xyz, lab, _params(), mask)
    if which == "mask_no_labels":
        return _case(xyz, None, _params(), mask)
    return _case(xyz, lab, _params(drop=(2,)) if which == "drop" else _params(protect=(1, 3)))


_CASES = {
    "street_stat": lambda: _street("stat"),
    "street_radius": lambda: _street("radius"),
    "street_both": lambda: _street("both"),
    **{f"mean_k_{k}": (lambda k=k: _mean_k(k)) for k in MEAN_KS},
    **{f"exact_count_{k}": (lambda k=k: _exact_count(k)) for k in MEAN_KS},
    "duplicates": _duplicates,
    "nan_mix": _nan_mix,
    **{f"tree_{n}": (lambda n=n: _tree(n)) for n in TREE_SIZES},
    "two_points": _two_points,
    "clamped": _clamped,
    "radius_edge": _radius_edge,
    "faces": _faces,
    "dense": _dense,
    "interleaved": _interleaved,
    "select_mask": lambda: _select("mask"),
    "select_mask_no_labels": lambda: _select("mask_no_labels"),
    "select_drop": lambda: _select("drop"),
    "select_protect": lambda: _select("protect"),
}
NAMES = list(_CASES)
STREET = [n for n in NAMES if n.startswith("street")]
REALISTIC = STREET + ["interleaved", "duplicates"]  # every test that is on removes some tested points and keeps some


@functools.lru_cache(maxsize=None)
def case(name):
    return _CASES[name]()


def too_few(k):
    """mean_k finite points: refused"""
    return _exact_count(k, missing=1)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    return filter_ref.filter(c["xyz"], c["labels"], c["mask"], **c["params"])


def small(name, limit=1500):
    """the case itself, or its first `limit` points"""
    c = case(name)
    if len(c["xyz"]) <= limit:
        return c
    cut = lambda a: None if a is None else a[:limit]
    return {"xyz": c["xyz"][:limit], "labels": cut(c["labels"]), "mask": cut(c["mask"]), "params": c["params"]}
