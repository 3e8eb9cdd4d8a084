"""Inputs, sizes and bars of the accumulate tests (tests/test_accumulate_cases_cpu.py on the geometry and the oracle alone,
tests/test_gpu_accumulate_paths.py through the library): the chunk geometry of csrc/kernels.h restated in Python, the seeded
points, the engine / oracle parameter builders, an np.longdouble restatement of the oracle's sums (how far float64 itself is
from the formulas) and the comparison.

The reference everywhere is the oracle's literal accumulate on the indices, weights and covariances the engine reports.

What the sizes are about (csrc/solve_kernels.hip): a pair's K * n_s slots are cut into groups of SG slots (4 when K is a
multiple of 4, else 2: K = 1 puts TWO source points into a group), a lane takes 8 / SG groups 256 apart, 256 lanes make a
chunk of 2048 slots, a workgroup parks the wave sums of up to 8 chunks in LDS before it joins them, and a launch whose
running chunks number at least 8 runs x 8 chunks x gridDim (gridDim = 2 workgroups per CU) hands its chunks out by an
agent-scope counter instead of as equal static ranges.

K = 1 cannot reach that threshold: 64 x 2 x 256 CUs = 32 768 chunks over the 256 pairs one launch holds are 128 chunks =
262 144 source points per pair, and the synthetic scans have about 140 000."""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
import synth
from np_ref import mat_to_qt

C = 11
CHUNK_SLOTS = 2048
COMB_CHUNKS = 8                # chunks parked in LDS between two combining passes = the length of a run
RUNS_PER_WORKGROUP = 8         # kRunsPerWorkgroupForDynamic
WORKGROUPS_PER_CU = 2          # SICP_ACC_OCC
MAX_PAIRS = 256                # kMaxActivePairs
GATE_OPEN = 1e30

MODE_NAMES = {O.MODE_GICP: "gicp", O.MODE_EM: "em", O.MODE_SEMANTIC: "semantic"}


# ---- csrc/kernels.h ---------------------------------------------------------------------------------------------------------------
def slots_per_group(K):
    return 4 if K % 4 == 0 else 2


def acc_geometry(total_slots, spg):
    """AccGeometry acc_geometry(total_slots, slots_per_group), field by field"""
    per_lane = 8 // spg
    n_groups = (total_slots + spg - 1) // spg
    m = max((n_groups + 256 * per_lane * 1024 - 1) // (256 * per_lane * 1024), 1)
    steps = per_lane * m
    chunk_groups = 256 * steps
    n_chunks = max((n_groups + chunk_groups - 1) // chunk_groups, 1)
    return dict(n_groups=n_groups, steps=steps, chunk_groups=chunk_groups, n_chunks=n_chunks)


def n_chunks(n_s, K):
    return acc_geometry(n_s * K, slots_per_group(K))["n_chunks"]


def ragged_last_group(n_s, K):
    """slots of the last group that lie past the end (the kernel reads them and weighs them by zero)"""
    spg = slots_per_group(K)
    return (-(n_s * K)) % spg


def dynamic_threshold(cus):
    """running chunks from which accumulate_staged_kernel hands chunks out by runs"""
    return RUNS_PER_WORKGROUP * COMB_CHUNKS * WORKGROUPS_PER_CU * cus


def handles_for_dynamic(cus, n_s, K):
    per_pair = n_chunks(n_s, K)
    return (dynamic_threshold(cus) + per_pair - 1) // per_pair


def solo_fits(n_s, K, cus):
    """solve_one_fits: one workgroup per chunk and the master, one per CU"""
    g = acc_geometry(n_s * K, slots_per_group(K))
    return n_s > 0 and g["n_chunks"] + 1 <= min(cus, 257) and g["steps"] == 8 // slots_per_group(K)


def largest_source_with_chunks(chunks, K):
    return chunks * CHUNK_SLOTS // K


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
# 1. the dynamic hand-out: (mode, knn, source points); neither size is a multiple of a chunk's source points, so that runs
#    straddle pair boundaries inside a ragged last chunk
DYNAMIC_CASES = {"em_k4": (O.MODE_EM, 4, 130877), "em_k20": (O.MODE_EM, 20, 59999)}
DYNAMIC_TARGET = 60000

# 2. every instantiation: mode x knn x use_sqloss on the mid-size pair
MID_SOURCE, MID_TARGET = 3000, 3000
MATRIX = [(mode, knn, sq) for mode in (O.MODE_EM, O.MODE_GICP) for knn in (1, 4, 20) for sq in (1, 0)]

# 3. chunk geometry edges, by K: (source points) -> what tests/test_accumulate_cases_cpu.py asserts about each
EDGE_SIZES = {
    4: (1, 3, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 4609),
    1: (1, 2, 3, 127, 128, 129, 511, 513, 2047, 2048, 2049, 16383, 16385),
    20: (1, 7, 102, 103, 205, 819, 820),
}
# (K, n_s): (chunks, slots of the last group past the end)
EDGE_EXPECT = {
    (4, 1): (1, 0), (4, 3): (1, 0), (4, 255): (1, 0), (4, 256): (1, 0), (4, 257): (1, 0), (4, 511): (1, 0), (4, 512): (1, 0),
    (4, 513): (2, 0), (4, 4095): (8, 0), (4, 4096): (8, 0), (4, 4097): (9, 0), (4, 4609): (10, 0),
    (1, 1): (1, 1), (1, 2): (1, 0), (1, 3): (1, 1), (1, 127): (1, 1), (1, 128): (1, 0), (1, 129): (1, 1), (1, 511): (1, 1),
    (1, 513): (1, 1), (1, 2047): (1, 1), (1, 2048): (1, 0), (1, 2049): (2, 1), (1, 16383): (8, 1), (1, 16385): (9, 1),
    (20, 1): (1, 0), (20, 7): (1, 0), (20, 102): (1, 0), (20, 103): (2, 0), (20, 205): (3, 0), (20, 819): (8, 0), (20, 820): (9, 0),
}
EDGE_CASES = [(O.MODE_EM, 4, n) for n in EDGE_SIZES[4]] + [(O.MODE_GICP, 1, n) for n in EDGE_SIZES[1]] + \
             [(O.MODE_EM, 1, n) for n in EDGE_SIZES[1]] + [(O.MODE_EM, 20, n) for n in EDGE_SIZES[20]]

# 5. loss and epsilon away from the defaults
LOSS_A = (0.05, 1.5, 3.0, 50.0)
EPSILONS = (1e-1, 1e-3, 1e-6)


def case_id(mode, knn, *rest):
    return "-".join([f"{MODE_NAMES[mode]}_k{knn}"] + [str(r) for r in rest])


# ---- points -------------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def pair20k():
    """synth.lidar_pair(seed=2, n_points=20000) with its source in a seeded random order (the scan comes ring by ring: a
    prefix of it would be a band), its target thinned to MID_TARGET points all over the scan, and the true pose.
    The mid-size pair is the first MID_SOURCE source points; the edge sizes are longer or shorter prefixes."""
    src, sl, tgt, tl, T, _ = synth.lidar_pair(seed=2, n_points=20000)
    perm = np.random.default_rng(31).permutation(len(src))
    pick = np.linspace(0, len(tgt) - 1, MID_TARGET).astype(int)
    return _frozen(np.ascontiguousarray(src[perm]), np.ascontiguousarray(sl[perm]), np.ascontiguousarray(tgt[pick]),
                   np.ascontiguousarray(tl[pick]), mat_to_qt(T))


def mid_pair(n_s=MID_SOURCE):
    src, sl, tgt, tl, qt = pair20k()
    return src[:n_s], sl[:n_s], tgt, tl, qt


@functools.lru_cache(maxsize=None)
def big_pair():
    """the clouds of the dynamic hand-out: one street scan pair, target thinned to DYNAMIC_TARGET points"""
    n = max(v[2] for v in DYNAMIC_CASES.values())
    src, sl, tgt, tl, T, _ = synth.lidar_pair(seed=6, n_points=n)
    pick = np.linspace(0, len(tgt) - 1, DYNAMIC_TARGET).astype(int)
    return _frozen(src, sl, np.ascontiguousarray(tgt[pick]), np.ascontiguousarray(tl[pick]), mat_to_qt(T))


def poses_around(qt, n, seed, sigma_t=0.01, sigma_r=1e-3):
    """n distinct poses near qt: every pair of a batch is evaluated at its own"""
    rng = np.random.default_rng(seed)
    out = np.tile(np.asarray(qt, dtype=np.float64), (n, 1))
    out[:, 4:] += rng.normal(0, sigma_t, (n, 3))
    out[:, :3] += rng.normal(0, sigma_r, (n, 3))
    out[:, :4] /= np.linalg.norm(out[:, :4], axis=1, keepdims=True)
    return out


def far_pose(qt, shift):
    out = np.array(qt, dtype=np.float64)
    out[4:] += shift
    return out


@functools.lru_cache(maxsize=None)
def semantic_first_class_small():
    """SICP_MODE_SEMANTIC: the label of target point 0 -- the first label segment, device record 0 -- has 300 source points,
    not more than min_class_pts = 400: the class is skipped, every one of its source slots is dead and is evaluated ON a
    record of that class, and no live slot refers to it.  (src, labels, tgt, labels, qt, the label)"""
    src, sl, tgt, tl, _ = synth.config1_pair(seed=1, n_per_label=700)
    first = int(tl[0])
    keep = np.ones(len(src), dtype=bool)
    keep[np.nonzero(sl == first)[0][300:]] = False
    qt = mat_to_qt(synth.pose_matrix(1.0, (0, 1, 0), (0.05, 0.0, -0.02)))
    return _frozen(np.ascontiguousarray(src[keep]), np.ascontiguousarray(sl[keep]), tgt, tl, qt) + (first,)


@functools.lru_cache(maxsize=None)
def semantic_one_point_class():
    """SICP_MODE_SEMANTIC: target point 0 is the only target point of its class (a neighbourhood of one point: no plane to
    fit), and 450 source points -- more than min_class_pts -- carry that label: all of them meet that one record, and every
    dead slot is evaluated on it.  (src, labels, tgt, labels, qt, the label)"""
    src, sl, tgt, tl, _ = synth.config1_pair(seed=1, n_per_label=700)
    lone = 9
    rng = np.random.default_rng(17)
    extra = (src[:450] + rng.normal(0, 0.02, (450, 3))).astype(np.float32)
    src2 = np.concatenate([src, extra]); sl2 = np.concatenate([sl, np.full(450, lone)]).astype(np.uint32)
    tgt2 = np.concatenate([tgt[:1] + np.float32(0.01), tgt]).astype(np.float32)
    tl2 = np.concatenate([[lone], tl]).astype(np.uint32)
    # one source class without a target class as well: its slots are dead
    keep = tl2 != tl[0]
    keep[0] = True
    qt = mat_to_qt(synth.pose_matrix(1.0, (0, 1, 0), (0.05, 0.0, -0.02)))
    return _frozen(np.ascontiguousarray(src2), sl2, np.ascontiguousarray(tgt2[keep]), np.ascontiguousarray(tl2[keep]), qt) + (lone,)


# ---- parameters -----------------------------------------------------------------------------------------------------------------------
LOSS_KEYS = ("knn", "cauchy_a", "use_sqloss", "epsilon", "gate_sq", "min_class_pts")


def set_params(p, mode, **kw):
    """the fields the engine's and the oracle's parameter structs share, set on either"""
    p.num_classes = C if mode == O.MODE_EM else 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def oracle_params(mode, **kw):
    p = O.default_params(mode)
    p.use_kdtree = 1
    return set_params(p, mode, **{k: v for k, v in kw.items() if k in LOSS_KEYS})


# ---- slots removed: would the reference notice? ---------------------------------------------------------------------------------------
def removals(idx):
    """the index array with (a) the last source point's slots, (b) the first group of the last chunk, (c) slot 0 removed"""
    n_s, K = idx.shape
    spg = slots_per_group(K)
    g = acc_geometry(n_s * K, spg)
    out = {}
    a = idx.copy(); a[-1, :] = -1
    out["last source point"] = a
    b = idx.copy().reshape(-1)
    first = (g["n_chunks"] - 1) * g["chunk_groups"] * spg
    b[first:first + spg] = -1
    out["first group of the last chunk"] = b.reshape(n_s, K)
    c = idx.copy(); c[0, 0] = -1
    out["slot 0"] = c
    return out


# ---- bars -------------------------------------------------------------------------------------------------------------------------------
def project_bars(ref):
    """absolute bar per entry: H 1e-9 x max |H|; g 1e-9 x max |g| + 1e-9 x max |H|; cost 1e-11 relative
    (tests/test_gpu_parity.py: test_weights_and_accumulate_vs_oracle)"""
    ref = np.asarray(ref, dtype=np.float64)
    bar = np.empty(28)
    scale = np.abs(ref[:21]).max()
    bar[:21] = 1e-9 * scale
    bar[21:27] = 1e-9 * np.abs(ref[21:27]).max() + 1e-9 * scale
    bar[27] = 1e-11 * abs(ref[27])
    return bar


def bars(ref, oracle_distance=None):
    """max(project bar, 4 x the float64 oracle's own distance to the np.longdouble restatement on the same slots)"""
    bar = project_bars(ref)
    if oracle_distance is not None:
        d = np.asarray(oracle_distance, dtype=np.float64)
        grouped = np.empty(28)
        grouped[:21], grouped[21:27], grouped[27] = d[:21].max(), d[21:27].max(), d[27]
        bar = np.maximum(bar, 4.0 * grouped)
    return bar


def excess(got, ref, bar):
    """the largest |got - ref| / bar over the 28 entries (<= 1 passes); entries whose bar is 0 must be equal"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(bar > 0, err / bar, np.where(err == 0, 0.0, np.inf))
    return float(q.max()), err


def assert_sums(got, ref, what, oracle_distance=None):
    bar = bars(ref, oracle_distance)
    q, err = excess(got, ref, bar)
    print(f"{what}: H {err[:21].max():.3e} / {bar[0]:.3e}  g {err[21:27].max():.3e} / {bar[21]:.3e}  "
          f"cost {err[27]:.3e} / {bar[27]:.3e}  worst err / bar = {q:.3g}")
    assert np.isfinite(np.asarray(ref)).all(), what
    assert np.isfinite(np.asarray(got)).all(), (what, got)
    assert q <= 1.0, (what, q, got, ref)
    return q


def moved_beyond(ref, other, factor=1000.0):
    """does `other` differ from ref in some entry by more than factor x that entry's bar?"""
    bar = project_bars(ref)
    return bool((np.abs(np.asarray(other) - np.asarray(ref)) > factor * bar).any())


# ---- the oracle's formulas in np.longdouble ------------------------------------------------------------------------------------------
LD = np.longdouble


def _inv3(A):
    """[n, 3, 3] inverses by the adjugate"""
    a, b, c = A[:, 0, 0], A[:, 0, 1], A[:, 0, 2]
    d, e, f = A[:, 1, 0], A[:, 1, 1], A[:, 1, 2]
    g, h, i = A[:, 2, 0], A[:, 2, 1], A[:, 2, 2]
    co = np.empty_like(A)
    co[:, 0, 0], co[:, 0, 1], co[:, 0, 2] = e * i - f * h, c * h - b * i, b * f - c * e
    co[:, 1, 0], co[:, 1, 1], co[:, 1, 2] = f * g - d * i, a * i - c * g, c * d - a * f
    co[:, 2, 0], co[:, 2, 1], co[:, 2, 2] = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * co[:, 0, 0] + b * co[:, 1, 0] + c * co[:, 2, 0]
    return co / det[:, None, None]


def _rotation(q):
    x, y, z, w = q
    one, two = LD(1), LD(2)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=LD)


def accumulate_longdouble(p, qt, src, scov, tgt, tcov, idx, w):
    """oracle_lib.accumulate restated: GICPCostFunction::Evaluate with the quaternion Jacobian, the plus-Jacobian of the
    SE3 parameterisation, the Ceres losses and Corrector (rho2 <= 0 for every loss stack here), vectorised over the live
    slots in np.longdouble; returns the 28 sums as longdouble"""
    q = np.asarray(qt, dtype=np.float64).astype(LD)
    R, t = _rotation(q[:4]), q[4:]
    idx = np.asarray(idx)
    ii, cc = np.nonzero(idx >= 0)
    out = np.zeros(28, dtype=LD)
    if len(ii) == 0:
        return out
    jj = idx[ii, cc]
    ps, pt = np.asarray(src, dtype=np.float32)[ii].astype(LD), np.asarray(tgt, dtype=np.float32)[jj].astype(LD)
    Cs, Ct = np.asarray(scov, dtype=np.float64).reshape(-1, 3, 3)[ii].astype(LD), np.asarray(tcov, dtype=np.float64).reshape(-1, 3, 3)[jj].astype(LD)
    Cst, Ctt = Cs.transpose(0, 2, 1), Ct.transpose(0, 2, 1)
    M = _inv3(Ct + R @ Cs @ R.T)
    Ta = _inv3(Ctt + R @ Cst @ R.T)
    res = pt - (ps @ R.T + t)
    tb = np.einsum("nij,nj->ni", M, res)
    tc = np.einsum("nij,nj->ni", Ta, res)
    r = (res * tb).sum(axis=1)
    r1 = np.einsum("ni,nij->nj", np.einsum("ni,nij->nj", res, Ta) @ R, Cst)
    r2 = np.einsum("ni,nij->nj", np.einsum("ni,nij->nj", res, M) @ R, Cs)
    dR = -(tb[:, :, None] * ps[:, None, :] + tc[:, :, None] * r1[:, None, :] + tb[:, :, None] * r2[:, None, :] + tc[:, :, None] * ps[:, None, :])
    tx, ty, tz, tw = (LD(2) * q[k] for k in range(4))
    mfx, mfy, mfz, mtw, z0 = -LD(2) * tx, -LD(2) * ty, -LD(2) * tz, -tw, LD(0)
    dRd = [np.array(v, dtype=LD).reshape(3, 3) for v in (
        [z0, ty, tz, ty, mfx, mtw, tz, tw, mfx],      # d/dx
        [mfy, tx, tw, tx, z0, tz, mtw, tz, mfy],      # d/dy
        [mfz, mtw, tx, tw, mfz, ty, tx, ty, z0],      # d/dz
        [z0, -tz, ty, tz, z0, -tx, -ty, tx, z0])]     # d/dw
    j7 = np.empty((len(ii), 7), dtype=LD)
    for k in range(4):
        j7[:, k] = (dR * dRd[k]).sum(axis=(1, 2))
    j7[:, 4:] = -LD(2) * tb
    P = np.zeros((7, 6), dtype=LD)
    h = LD(0.5)
    c0, c1, c3, c4 = h * q[3], h * q[2], h * q[1], h * q[0]
    P[0, 3:] = (c0, -c1, c3)
    P[1, 3:] = (c1, c0, -c4)
    P[2, 3:] = (-c3, c4, c0)
    P[3, 3:] = (-c4, -c3, -c1)
    P[4:, :3] = R
    J = j7 @ P
    # the losses at s = r^2
    a = LD(p.cauchy_a)
    b = a * a
    c = LD(1) / b
    s = r * r
    ww = np.ones(len(ii), dtype=LD) if w is None else np.asarray(w, dtype=np.float64)[ii, cc].astype(LD)
    tiny = LD(np.finfo(np.float64).tiny)
    if p.use_sqloss:
        v = s + LD(np.finfo(np.float64).eps)
        g0, g1 = np.sqrt(v), LD(1) / (LD(2) * np.sqrt(v))
        total = LD(1) + g0 * c
        f0, f1 = b * np.log(total), np.maximum(LD(1) / total, tiny)
        if p.mode == O.MODE_EM:
            f0, f1 = f0 * ww, f1 * ww
        rho0, rho1 = f0, f1 * g1
    else:
        total = LD(1) + s * c
        rho0, rho1 = b * np.log(total), np.maximum(LD(1) / total, tiny)
    o = 0
    for x in range(6):
        for y in range(x, 6):
            out[o] = (rho1 * J[:, x] * J[:, y]).sum()
            o += 1
        out[21 + x] = (rho1 * J[:, x] * r).sum()
    out[27] = (LD(0.5) * rho0).sum()
    return out


def oracle_distance(p, qt, src, scov, tgt, tcov, idx, w, ref):
    """|float64 oracle - longdouble restatement| per entry, as float64"""
    return np.abs(np.asarray(ref, dtype=np.float64).astype(LD) - accumulate_longdouble(p, qt, src, scov, tgt, tcov, idx, w)).astype(np.float64)
