"""Inputs of the bootstrap edge tests (tests/test_gpu_bootstrap_edges.py, tests/test_bootstrap_edges_cpu.py): clouds and
parameter sets away from the defaults, each built so that one branch of the bootstrap is reached, with the CPU-side
proof that it is (counted in the restatement tests/bootstrap_ref.py alone).  numpy / scipy only: no library, no GPU."""
from __future__ import annotations

import functools

import numpy as np

import bootstrap_ref as R
import synth

SMALL_GAP = 1e-6       # eigenvalue gap below which a normal's direction is not compared (tests/test_gpu_bootstrap.py)
SMALL_GAP_CAP = 0.02   # at most this share of the rows with a normal may be left out for it (non-degenerate cases)


def ref_args(params: dict):
    """(voxel_keypoints kwargs, features kwargs) of a dict of sicp_bootstrap_params overrides"""
    P = dict(R.DEFAULTS, **params)
    return dict(box_max=P["box_max"], leaf=P["leaf_size"]), dict(normal_radius=P["normal_radius"], feature_radius=P["feature_radius"])


@functools.lru_cache(maxsize=None)
def lidar(n=20000, seed=3):
    src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=seed, n_points=n)
    return src, sl, tgt, tl, cm


@functools.lru_cache(maxsize=None)
def lidar_sub(n):
    """n points of each cloud of lidar(), evenly spread over the caller order (no second run of the generator)"""
    src, sl, tgt, tl, cm = lidar()
    a = np.linspace(0, len(src) - 1, n).astype(np.int64)
    b = np.linspace(0, len(tgt) - 1, n).astype(np.int64)
    return src[a], sl[a], tgt[b], tl[b], cm


@functools.lru_cache(maxsize=None)
def rgbd():
    """one frame of the RGB-D generator at a quarter of the resolution: dense, metre scale"""
    src, sl, tgt, tl, T, cm = synth.rgbd_pair(seed=3, stride=4)
    return src, tgt


def _by_distance(cloud):
    """the cloud's indices by distance from one of its points"""
    return np.argsort(((cloud.astype(np.float64) - cloud[len(cloud) // 3]) ** 2).sum(axis=1), kind="stable")


def compact(cloud, n):
    """the n points of a cloud nearest to one of its points (caller order kept): a dense crop"""
    return cloud[np.sort(_by_distance(cloud)[:n])]


def emptied(cloud, box_max=35.0):
    """the cloud with every x moved beyond the box limit: the filter keeps nothing"""
    out = cloud.copy()
    out[:, 0] = np.abs(out[:, 0]) + np.float32(box_max + 1.0)
    return out


def crop_to_keypoints(cloud, want, n_isolated=0, **vk):
    """a crop of `cloud` whose voxel grid has exactly `want` keypoints: the points nearest to one of them, as many as it
    takes (a point more adds one occupied voxel or none), plus `n_isolated` points far from everything (keypoints
    without a feature)"""
    order = _by_distance(cloud)
    iso = np.array([[-30.0 - 9.0 * i, -30.0, 20.0] for i in range(n_isolated)], np.float32).reshape(-1, 3)
    body = want - n_isolated
    assert body >= 0
    lo, hi = body, len(cloud)
    count = lambda m: len(R.voxel_keypoints(cloud[np.sort(order[:m])], **vk)) if m else 0
    while lo < hi:  # smallest m with count(m) >= body; count is non-decreasing and steps by at most 1
        mid = (lo + hi) // 2
        if count(mid) >= body:
            hi = mid
        else:
            lo = mid + 1
    out = np.concatenate([cloud[np.sort(order[:lo])], iso]) if body else iso
    assert len(R.voxel_keypoints(out, **vk)) == want
    return np.ascontiguousarray(out, np.float32)


def lattice(s=0.5, ni=6, nk=(0, 4)):
    """points (i, j, k) * s + s / 4, i, j in -ni..ni, k in nk[0]..nk[1]-1: with leaf s / 2 every point is alone in its
    voxel and off every voxel face, so the keypoints are the points bit for bit and in lattice (k, j, i) order"""
    r = np.arange(-ni, ni + 1)
    k, j, i = np.meshgrid(np.arange(*nk), r, r, indexing="ij")
    p = np.stack([i.ravel(), j.ravel(), k.ravel()], 1).astype(np.float64) * s + s / 4
    return p.astype(np.float32)


def plane(z, s=0.5, ni=8):
    """one lattice layer at height z exactly (z = 0: a plane through the origin, where (-p) . n is 0 for every point)"""
    p = lattice(s, ni, (0, 1))
    p[:, 2] = z
    return p


def diagonal_line(s=0.5, ni=12):
    """points (i, i, 0) * s + (s / 4, s / 4, s / 4): exactly collinear in f32, along (1, 1, 0)"""
    i = np.arange(-ni, ni + 1, dtype=np.float64)
    return np.stack([i * s + s / 4, i * s + s / 4, np.full_like(i, s / 4)], 1).astype(np.float32)


def boundary_pairs(kp, r):
    """ordered pairs (i != j) whose f32 d^2 is exactly f32(r * r): inside with `<=`, outside with the rule's `<`"""
    r2 = np.float32(r * r)
    n = 0
    for i in range(len(kp)):
        n += int((R.d2_f32(kp, kp[i]) == r2).sum())
    return n


def small_gap_share(ref):
    """share of the rows with a normal whose eigenvalue gap is too small for the direction to be compared"""
    ok = ~np.isnan(ref["normals"][:, 0])
    return float((ref["gap"][ok] <= SMALL_GAP).mean()) if ok.any() else 0.0


def one_voxel_cloud():
    """5000 points inside the voxel [0, 0.4)^3, magnitudes spread over 60 binary orders (their f64 sums round), among 100
    points elsewhere, negative coordinates included"""
    rng = np.random.default_rng(21)
    inside = (0.4 * 2.0 ** -rng.uniform(0.01, 60.0, size=(5000, 3))).astype(np.float32)
    other = rng.uniform(-8.0, 8.0, size=(100, 3)).astype(np.float32)
    other = other[(np.floor(other * (np.float32(1) / np.float32(0.4))) != 0).any(axis=1)]
    p = np.concatenate([inside, other])
    return p[rng.permutation(len(p))]


def neighbour_count_cloud():
    """four clusters 20 apart, of 1, 2, 3 and 4 points: with leaf 0.1 and radius 1 every keypoint's list is its cluster"""
    c = [[(0, 0, 5)],
         [(20, 0, 5), (20.3, 0.1, 5)],
         [(0, 20, 5), (0.3, 20, 5.1), (0, 20.4, 5.3)],
         [(20, 20, 5), (20.3, 20, 5.2), (20, 20.4, 5), (20.2, 20.2, 5.6)]]
    return np.array([q for cl in c for q in cl], np.float32)


def hub_cloud():
    """keypoints without a normal inside the lists of keypoints that have one (radius r = 1, leaf 0.05):
    * a hub with six spokes 0.9 r out along the axes: each spoke is within r of the hub and 1.27 r from the other spokes,
      so its list is itself and the hub (2 < 3: no normal), and the hub, which has a normal, has no valid pair at all;
    * a dense patch with two tails leading away from it: t1 sees the patch and t2; t2 sees t1, t3 and itself (a normal);
      t3 sees t2 and itself (none).  t2's list mixes neighbours with and without a normal.
    Returns the cloud, r, and the caller indices of (hub, spokes, t2s, t3s) -- the keypoints keep no caller order, so the
    tests find them again by position."""
    r = 1.0
    hub = np.array([0.0, 0.0, 10.0])
    spokes = [hub + 0.9 * r * np.array(d) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    rng = np.random.default_rng(8)
    uv = rng.uniform(-1.5, 1.5, size=(400, 2))
    patch = np.c_[uv[:, 0] + 10.0, uv[:, 1], 4.0 + 0.2 * np.sin(2 * uv[:, 0]) * np.cos(1.5 * uv[:, 1])]
    tails = []
    for sg in (1.0, -1.0):
        tails += [[10.0 + sg * 2.1, 0.0, 4.0], [10.0 + sg * 2.7, 0.0, 4.0], [10.0 + sg * 3.2, 0.4, 4.0]]
    cloud = np.concatenate([[hub], spokes, patch, tails]).astype(np.float32)
    n0 = 7 + len(patch)
    return cloud, r, dict(hub=[0], spokes=list(range(1, 7)), t2=[n0 + 1, n0 + 4], t3=[n0 + 2, n0 + 5])


def denormal_pair_cloud():
    """a bumpy patch around the origin (leaf 0.05, radius 1) with two points 2e-22 apart on either side of the voxel face
    x = 0, each alone in its voxel: two keypoints whose f32 d^2 = 4e-44 is denormal, and each other's heaviest FPFH weight
    1 / d^2.  Returns the cloud and the two points' caller indices."""
    rng = np.random.default_rng(13)
    uv = rng.uniform(-1.5, 1.5, size=(400, 2))
    uv = uv[np.abs(uv - [0.0, 0.22]).max(axis=1) > 0.1]
    patch = np.c_[uv, 3.0 + 0.2 * np.sin(2 * uv[:, 0]) * np.cos(1.5 * uv[:, 1])]
    z0 = 3.0 + 0.2 * np.sin(0.0) * np.cos(1.5 * 0.22)
    twins = np.array([[-1e-22, 0.22, z0], [1e-22, 0.22, z0]])
    return np.concatenate([patch, twins]).astype(np.float32), (len(patch), len(patch) + 1)


def tie_patches(seed=0, copies=2, lift=8.0):
    """a bumpy lattice patch whose coordinates are multiples of 1/64 (one point per voxel of leaf 0.125), and `copies` of
    it `lift` apart in z (the first `n` keypoints are copy 0, keypoint i + n is the twin of keypoint i).  The differences
    between neighbours are exact and the same in every copy, so a keypoint and its twin get the same f32 feature row and
    any source feature is exactly as far from one as from the other.  (Only the neighbourhood means round differently, 1e-16
    relative; the tests assert the equal rows and the ties rather than take them for granted.)"""
    rng = np.random.default_rng(seed)
    r = np.arange(-8, 9)
    j, i = np.meshgrid(r, r, indexing="ij")
    x, y = i.ravel() * 0.25 + 0.0625, j.ravel() * 0.25 + 0.0625
    z = 4.0 + np.round(64 * (0.25 * np.sin(1.3 * x) * np.cos(0.9 * y) + rng.uniform(-0.04, 0.04, x.shape))) / 64 + 1 / 128
    one = np.stack([x, y, z], 1)
    return np.concatenate([one + [0, 0, lift * c] for c in range(copies)]).astype(np.float32), len(one)


TIE_PARAMS = dict(leaf_size=0.125, normal_radius=0.75, feature_radius=0.75)
LATTICE_S = 0.5
LATTICE_PARAMS = lambda r: dict(leaf_size=LATTICE_S / 2, normal_radius=r, feature_radius=r)
LATTICE_RADII = (LATTICE_S, LATTICE_S * np.sqrt(2.0), 2 * LATTICE_S)
