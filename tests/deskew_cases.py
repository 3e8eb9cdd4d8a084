"""The cases of sicp_deskew shared by tests/test_deskew_cpu.py and tests/test_gpu_deskew.py: each a cloud, a time per point, a
knot trajectory and a reference pose.  Tiny on purpose -- a few hundred points -- but for "launch_shape", which crosses the size
above which the driver's launch stops growing (kernels.h: kDeskewMaxGroups workgroups of 256 points) by one workgroup and one
point, so some workgroups take a second stride and the last one a partial wave."""
from __future__ import annotations

import functools

import numpy as np

import deskew_ref as R

T0, T1 = 100.0, 100.1
LAUNCH_SHAPE_N = 512 * 256 + 257
WORLD = np.array([0.1, -0.2, 0.3, 0.9, 120.0, -35.0, 2.0])  # where the trajectory starts: sensor -> some fixed frame
UNRELATED = np.array([-0.3, 0.1, 0.2, 0.8, 118.0, -33.0, 1.5])


def trajectory(n_knots, twist, seed, wiggle=1e-3, world=WORLD):
    """knot k = world * exp(s_k twist) * a small random motion: not a constant velocity, so every interval differs"""
    rng = np.random.default_rng(seed)
    world = R.normalised(world)
    s = np.arange(n_knots) / (n_knots - 1)
    kq = np.stack([R.mul(R.mul(world, R.se3_exp(sk * np.asarray(twist, float))), R.se3_exp(wiggle * rng.normal(size=6))) for sk in s])
    return T0 + s * (T1 - T0), kq


def cloud(n, seed, labels=True):
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-40, 40, (n, 3)) * [1, 1, 0.1]).astype(np.float32)
    return xyz, (rng.integers(1, 12, n).astype(np.uint32) if labels else None)


CAR = (3.0, 0.1, 0.0, 0.0, 0.01, 0.1)  # 30 m/s, 1 rad/s over the 0.1 s
NAMES = ("n1", "n63", "n64", "n65", "n257", "launch_shape", "knots2", "knots3", "knots1024", "shuffled", "all_equal", "on_knots",
         "clamped", "bad_times", "bad_points", "equal_knots", "sign_flip", "half_turn", "ref_knot", "ref_unrelated", "no_labels")
SMALL = tuple(n for n in NAMES if n != "launch_shape")


@functools.lru_cache(maxsize=None)
def case(name):
    """{"xyz", "labels", "times", "knot_time", "knot_qt", "ref_qt"}"""
    seed = NAMES.index(name) + 1
    rng = np.random.default_rng(1000 + seed)
    n = dict(n1=1, n63=63, n64=64, n65=65, n257=257, launch_shape=LAUNCH_SHAPE_N).get(name, 200)
    nk = dict(knots2=2, knots3=3, knots1024=1024).get(name, 33)
    twist = dict(knots2=(0.5, 0.02, 0, 0, 0.002, 0.15), knots3=(0.8, 0.03, 0, 0, 0.003, 0.3), half_turn=(2.0, 0.5, 0.1, 0.02, -0.03, np.pi)).get(name, CAR)
    xyz, labels = cloud(n, seed, labels=name != "no_labels")
    kt, kq = trajectory(nk, twist, seed)
    times = np.sort(rng.uniform(T0, T1, n))  # firing order
    ref = None
    if name == "shuffled":
        times = rng.permutation(times)
    elif name == "all_equal":
        times[:] = 100.0371
    elif name == "on_knots":
        times[[0, 7, 8, n - 1]] = kt[[0, 11, 11, nk - 1]]
        times[100:133] = kt
    elif name == "clamped":
        times[:20] = T0 - rng.uniform(1e-9, 5.0, 20)
        times[-30:] = T1 + rng.uniform(1e-9, 5.0, 30)
        times[20], times[-31] = np.nextafter(T0, 0), np.nextafter(T1, 1e9)
    elif name == "bad_times":
        times[[3, 64, 65, 199]] = np.nan
        times[[10, 100]] = np.inf
        times[[11, 128]] = -np.inf
    elif name == "bad_points":
        xyz[[0, 63, 150], [0, 1, 2]] = np.nan
        xyz[[5, 64], [1, 0]] = [np.inf, -np.inf]
        xyz[70] = [np.nan, np.inf, 1.0]
        times[[63, 64]] = np.nan      # a point that is not finite stays what it is whatever its time
        times[[1, 151]] = [np.nan, np.inf]
    elif name == "equal_knots":
        kq[17] = kq[16]
        kq[1] = kq[0]
        kq[32] = kq[31]
    elif name == "sign_flip":
        kq[1::2, :4] *= -1.0
        kq[8, :4] *= -1.0
    elif name == "ref_knot":
        ref = kq[5].copy()
    elif name == "ref_unrelated":
        ref = UNRELATED / np.concatenate([np.full(4, np.linalg.norm(UNRELATED[:4])), np.ones(3)])
    return dict(xyz=xyz, labels=labels, times=times, knot_time=kt, knot_qt=kq, ref_qt=ref)


def reference(name, knots):
    """the restatement on the table `knots` the library handed back"""
    c = case(name)
    return R.deskew(c["xyz"], c["times"], c["knot_time"], knots)
