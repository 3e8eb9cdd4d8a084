"""The inputs of the sicp_cluster tests, from fixed seeds: case(name) -> {"xyz", "labels", "params", ...}, params being the
keywords of cluster_ref.cluster (and, but for `ignore`, the fields of sicp_cluster_params); reference(name) is the restatement's
answer, computed once.  small=True gives the same family on at most 600 points, for the O(n^2) check of the restatement."""
import functools

import numpy as np

import cluster_ref
import synth

T = 0.5  # the tolerance of every synthetic family
T_UP = float(np.nextafter(np.float32(0.5), np.float32(1)))


def _params(tolerance=T, min_points=1, max_points=0, same_label=1, ignore=()):
    return dict(tolerance=tolerance, min_points=min_points, max_points=max_points, same_label=same_label, ignore=tuple(ignore))


@functools.lru_cache(maxsize=None)
def _street_scan():
    src, sl, *_ = synth.lidar_pair(seed=2, n_points=20000)
    return src, sl


def _street(tolerance, same_label, small):
    xyz, lab = _street_scan()
    if small:  # the 600 points about the first car point: objects, kerb and speckle at full density
        car = np.flatnonzero(lab == 3)[0]
        near = np.argsort(np.linalg.norm(xyz[:, :2] - xyz[car, :2], axis=1), kind="stable")[:600]
        sel = np.sort(near)
        xyz, lab = xyz[sel], lab[sel]
    return {"xyz": xyz, "labels": lab, "params": _params(tolerance, 3 if small else 10, 0, same_label, (1, 2))}


def _lattice(tolerance, small):
    m = 5 if small else 9
    g = np.arange(m, dtype=np.float32) * np.float32(0.5) - np.float32(1.0)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return {"xyz": xyz, "labels": np.full(len(xyz), 4, np.uint32), "params": _params(tolerance)}


def _chain(small):
    n = 512 if small else 4096
    step = 0.9 * T / np.sqrt(3.0)
    xyz = (np.arange(n)[:, None] * np.array([step, step, step]) + np.array([-300.0, 2.0, -1.0])).astype(np.float32)
    return xyz


def _comb(small):
    n = 250 if small else 1000
    a = np.stack([np.arange(n) * 0.9 * T, np.zeros(n), np.zeros(n)], axis=1)
    b = a + np.array([0.0, 1.5 * T, 0.0])
    bridge = np.array([[(n - 1) * 0.9 * T, 0.5 * T * 0.99, 0.0], [(n - 1) * 0.9 * T, 1.0 * T, 0.0]])
    return (np.concatenate([a, b, bridge]) + np.array([-7.3, 11.1, 0.4])).astype(np.float32)


def _sheet(small):
    m = 24 if small else 64
    u, v = np.meshgrid(np.arange(m) * 0.9 * T, np.arange(m) * 0.9 * T, indexing="ij")
    return np.stack([u.ravel() - 3.0, v.ravel() - 20.0, 0.05 * np.sin(u.ravel())], axis=1).astype(np.float32)


def _long(shape, shuffled, small):
    xyz = {"chain": _chain, "comb": _comb, "sheet": _sheet}[shape](small)
    c = {"params": _params(), "perm": None}
    if shuffled:
        c["perm"] = np.random.default_rng(41).permutation(len(xyz))
        xyz = xyz[c["perm"]]
    c["xyz"], c["labels"] = xyz, np.full(len(xyz), 5, np.uint32)
    return c


def _dense(max_points, small):
    n = 500 if small else 5000
    rng = np.random.default_rng(17)
    d = rng.normal(size=(n, 3))
    d *= (0.2 * T * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
    centre = np.array([10.1, -4.2, 0.7])
    xyz = np.concatenate([centre + d, [centre + np.array([3 * T, 0.0, 0.0])]]).astype(np.float32)
    return {"xyz": xyz, "labels": np.full(n + 1, 3, np.uint32), "params": _params(max_points=max_points)}


FACE_BASES = {  # cell corners (in cells per axis) the pairs straddle
    "origin": (0, 0, 0),
    "near": (1, 2, -1),
    "negative": (-3, -1, -2),
    "tens": (-37, 25, -12),
    "plus_1000": (2000, 2000, 3),
    "minus_1000": (-2000, -1999, -4),
    "largest": (cluster_ref.CELL_LIMIT - 1,) * 3,
    "smallest": (-(cluster_ref.CELL_LIMIT - 2),) * 3,
}
FACE_DIRS = {"face": (1.0, 0.0, 0.0), "edge": (1.0, 1.0, 0.0), "corner": (1.0, 1.0, 1.0)}


def _faces():
    """per base, per direction (through a cell face, edge, corner), per sign: a pair of its own label at distance
    T (1 -+ 2^-20) centred on the corner (before the rounding to float32, which decides at the large coordinates)"""
    edge = 1.0 / float(cluster_ref.grid_inv(T))
    pts, lab, names = [], [], []
    for bname, cells in FACE_BASES.items():
        corner = np.array(cells, dtype=np.float64) * edge
        for dname, d in FACE_DIRS.items():
            u = np.array(d) / np.linalg.norm(d)
            off = np.where(np.array(d) == 0.0, 0.2 * edge, 0.0)  # off the other faces
            for sign in (-1.0, 1.0):
                dist = T * (1.0 + sign * 2.0 ** -20)
                pts += [corner + off - 0.5 * dist * u, corner + off + 0.5 * dist * u]
                lab += [len(names) + 1] * 2
                names.append((bname, dname, sign))
    return {"xyz": np.array(pts).astype(np.float32), "labels": np.array(lab, np.uint32), "params": _params(), "pairs": names}


def beyond_the_grid():
    """one point whose x cell is CELL_LIMIT: refused at tolerance T"""
    x = (cluster_ref.CELL_LIMIT + 0.5) / float(cluster_ref.grid_inv(T))
    return np.array([[0.0, 0.0, 0.0], [x, 1.0, 2.0]], dtype=np.float32)


def _blobs(rng, centres, n):
    return np.concatenate([c + rng.uniform(-0.1, 0.1, (n, 3)) for c in centres]).astype(np.float32)


def _nan_mix():
    rng = np.random.default_rng(23)
    xyz = _blobs(rng, [(0, 0, 0), (5, 0, 0), (0, 7, 1), (-4, -4, 2)], 70)
    lab = np.repeat(np.array([3, 4, 3, 9], np.uint32), 70)
    p = rng.permutation(len(xyz))
    xyz, lab = xyz[p], lab[p]
    xyz[0] = np.nan  # the first point: first_index must skip it
    xyz[5::17, 0] = np.nan
    xyz[9::31, 2] = np.inf
    xyz[11::53, 1] = -np.inf
    return {"xyz": xyz, "labels": lab, "params": _params(min_points=2, ignore=(9,))}


def _all_ignored():
    rng = np.random.default_rng(24)
    return {"xyz": _blobs(rng, [(0, 0, 0), (2, 0, 0)], 40), "labels": np.repeat(np.array([1, 2], np.uint32), 40),
            "params": _params(ignore=(2, 1, 77))}


def _one_point():
    return {"xyz": np.array([[1.5, -2.5, 0.25]], np.float32), "labels": np.array([6], np.uint32), "params": _params()}


def _no_labels():
    rng = np.random.default_rng(25)
    xyz = _blobs(rng, [(0, 0, 0), (3, 0, 0), (0, 3, 0)], 90)
    xyz[7] = np.nan
    return {"xyz": xyz, "labels": None, "params": _params(min_points=2, same_label=0)}


def _two_label_blob():
    """same_label = 0: a blob of 6 + 6 points of labels 7 and 3 (the tie goes to 3), one of 5 + 3 of labels 9 and 2 (9 wins), one
    of a single label, and a point of an ignored label inside the first blob"""
    rng = np.random.default_rng(26)
    xyz = _blobs(rng, [(0, 0, 0)], 13)
    xyz = np.concatenate([xyz, _blobs(rng, [(4, 0, 0)], 8), _blobs(rng, [(0, 4, 0)], 5)])
    lab = np.array([7, 3] * 6 + [1] + [9] * 5 + [2] * 3 + [0xFFFFFFFF] * 5, np.uint32)
    return {"xyz": xyz, "labels": lab, "params": _params(same_label=0, ignore=(1,))}


_CASES = {
    "street_05_same": lambda s: _street(0.5, 1, s),
    "street_05_any": lambda s: _street(0.5, 0, s),
    "street_03_same": lambda s: _street(0.3, 1, s),
    "street_03_any": lambda s: _street(0.3, 0, s),
    "lattice_tie": lambda s: _lattice(T, s),
    "lattice_join": lambda s: _lattice(T_UP, s),
    "chain": lambda s: _long("chain", False, s),
    "chain_shuffled": lambda s: _long("chain", True, s),
    "comb": lambda s: _long("comb", False, s),
    "comb_shuffled": lambda s: _long("comb", True, s),
    "sheet": lambda s: _long("sheet", False, s),
    "sheet_shuffled": lambda s: _long("sheet", True, s),
    "dense": lambda s: _dense(0, s),
    "dense_max": lambda s: _dense((500 if s else 5000) - 1, s),
    "faces": lambda s: _faces(),
    "nan_mix": lambda s: _nan_mix(),
    "all_ignored": lambda s: _all_ignored(),
    "one_point": lambda s: _one_point(),
    "no_labels": lambda s: _no_labels(),
    "two_label_blob": lambda s: _two_label_blob(),
}
NAMES = list(_CASES)
STREET = [n for n in NAMES if n.startswith("street")]
LONG = ["chain", "comb", "sheet"]


@functools.lru_cache(maxsize=None)
def case(name, small=False):
    return _CASES[name](small)


@functools.lru_cache(maxsize=None)
def _components(name, small):
    c = case(name, small)
    p = c["params"]
    return cluster_ref.components(c["xyz"], c["labels"], p["tolerance"], p["same_label"], p["ignore"])


@functools.lru_cache(maxsize=None)
def reference(name, small=False):
    c = case(name, small)
    shared = {"dense_max": "dense"}.get(name, name)  # the same cloud and edges, other size bounds: one pair search serves both
    return cluster_ref.cluster(c["xyz"], c["labels"], parts=_components(shared, small), **c["params"])
