"""sicp_pose_covariance (csrc/pose_cov_kernels.hip, csrc/pose_cov.cpp) against the numpy restatement (tests/pose_cov_ref.py)
on the engine's own correspondences, weights and normals, at every path the kernels have and the rest of the suite does
not reach (cases and bar: tests/pose_cov_cases.py, checked without a GPU by tests/test_pose_cov_cases_cpu.py):

 1. every loss stack: 3 modes x K in {1, 4, 20} x use_sqloss in {0, 1}; EM without SQLoss must NOT match the restatement
    with the EM weights applied (the weights belong to the SQLoss stack alone);
 2. cauchy_a and epsilon away from the defaults, and a pair at its exact pose (r = 0 on every slot);
 3. tile and owner geometry on crafted pairs whose sorted layout is known: runs inside a tile, on a tile edge, at every
    phase, across and through workgroups, chains of up to 513 tiles, the gated tail on and beside a tile edge, n_t and
    n_s K exact powers of two; and the source kernel's last column;
 4. the same jobs away from a group's origin, reordered by kind, one of them with every slot gated out: lone bytes;
 5. a stream registration on a non-default stack: lone bytes.

The bar: |got - want|_max <= max(1e-8, 4 x gap) x max |diag(want)|, gap = the float64 restatement's distance to its own
np.longdouble run on the same inputs.  Every comparison prints its kernel gap, restatement gap and bar
(profiles/pose_cov_paths/figures.txt)."""
import ctypes
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pose_cov_cases as P
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
MODES = (sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC)
MODE_NAMES = {sicp.MODE_GICP: "gicp", sicp.MODE_EM: "em", sicp.MODE_SEMANTIC: "semantic"}


def _qt(T):
    return np.concatenate([Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]])


_cache = {}


def lidar(n=2000, seed=11):
    """(src, labels, tgt, labels, a pose near the true one, confusion matrix) of one street scan pair, computed once"""
    if (n, seed) not in _cache:
        src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=seed, n_points=n)
        rng = np.random.default_rng(seed)
        D = np.eye(4)
        D[:3, :3] = Rotation.from_rotvec(rng.normal(scale=0.004, size=3)).as_matrix()
        D[:3, 3] = rng.normal(scale=0.02, size=3)
        for a in (src, sl, tgt, tl, cm):
            a.setflags(write=False)
        _cache[(n, seed)] = (src, sl, tgt, tl, _qt(T @ D), cm)
    return _cache[(n, seed)]


def params_of(mode, **kw):
    p = sicp.default_params(mode)
    p.num_classes = P.C
    if mode == sicp.MODE_SEMANTIC:
        p.min_class_pts = 40
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def engine(mode, src, sl, tgt, tl, cm=None, **kw):
    return loaded(sicp.Engine(0, params_of(mode, **kw)), mode, src, sl, tgt, tl, cm)


def loaded(e, mode, src, sl, tgt, tl, cm=None):
    try:
        if mode == sicp.MODE_EM:
            e.set_confusion(synth.confusion_matrix(P.C) if cm is None else cm)
        lab = mode != sicp.MODE_GICP
        e.set_source(src, sl if lab else None)
        e.set_target(tgt, tl if lab else None)
    except Exception:
        e.close()
        raise
    return e


def raw(e, qt):
    r = sicp.SicpPoseCovarianceResult()
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    assert sicp.lib().sicp_pose_covariance(e._h, sicp._ptr(qt, sicp._dp), 1.0, 1.0, ctypes.byref(r)) == sicp.OK
    return bytes(r)


def check(e, mode, src, tgt, qt, what):
    """sicp_pose_covariance at qt: H, g, cost are sicp_accumulate's bits, active the count of idx >= 0, S_src and S_tgt within
    the bar of the restatement on the engine's idx, w and normals.  Returns (result, idx, w or None, the inputs of P.reference)"""
    r = e.pose_covariance(qt)
    idx, _, w = e.correspondences(qt)
    out28 = e.accumulate(qt)
    assert np.array_equal(r["hessian21"], out28[:21]) and np.array_equal(r["gradient"], out28[21:27]) and r["cost"] == out28[27], what
    assert r["active"] == int((idx >= 0).sum()), what
    sn, tn = e.covariances(sicp.SOURCE)[1], e.covariances(sicp.TARGET)[1]
    p = e.get_params()
    w = w if mode == sicp.MODE_EM else None          # the other modes have no weights
    inputs = (qt, src, sn, tgt, tn, idx, w, p.epsilon, p.use_sqloss, p.cauchy_a)
    want, gaps = P.reference(*inputs)
    line, ok = [], True
    for name, got, S, gap in (("source", r["cross_source"], want[0], gaps[0]), ("target", r["cross_target"], want[1], gaps[1])):
        assert np.isfinite(got).all() and np.isfinite(S).all(), (what, name)
        d, bar = P.distance(got, S), P.bar_of(gap)
        line.append(f"{name} kernel {d:.3e} restatement {gap:.3e} bar {bar:.3e}")
        ok = ok and d <= bar
    print(f"pose_cov_paths: {what}: active {r['active']}  " + "  ".join(line))
    assert ok, (what, line)
    return r, idx, w, inputs


# ---- 1. every stack -----------------------------------------------------------------------------------------------------------------------
STACKS = [(m, K, sq) for m in MODES for K in (1, 4, 20) for sq in (0, 1)]


@pytest.mark.parametrize("mode,K,sq", STACKS, ids=[f"{MODE_NAMES[m]}_k{K}_{'sqloss' if sq else 'cauchy'}" for m, K, sq in STACKS])
def test_every_stack(mode, K, sq):
    src, sl, tgt, tl, qt, cm = lidar()
    what = f"stack {MODE_NAMES[mode]} K={K} sqloss={sq}"
    e = sicp.Engine(0, params_of(mode, use_sqloss=sq))      # the stack at the mode's own K: never refused
    try:
        e.set_params(params_of(mode, knn=K, use_sqloss=sq))      # only a refusal of this K is a reason to skip
    except sicp.SicpError as err:
        e.close()
        if err.status != sicp.ERR_INVALID_ARGUMENT:
            raise
        pytest.skip(f"{MODE_NAMES[mode]} refuses knn = {K}")
    with loaded(e, mode, src, sl, tgt, tl, cm) as e:
        r, idx, w, inputs = check(e, mode, src, tgt, qt, what)
    assert idx.shape == (len(src), K) and (idx >= 0).mean() > 0.5
    assert np.abs(r["gradient"]).max() > 0      # off the minimum: rho' r dJ/dz takes part
    if mode == sicp.MODE_EM:
        live = w[idx >= 0]
        assert (live != 1.0).any() and live.std() > 0.01      # the EM weights exist and vary
        if not sq:    # ... and stay out of the Cauchy stack, as they stay out of H
            weighted, gaps = P.reference(*inputs, weights_always=True)
            for name, got, S, gap in (("source", r["cross_source"], weighted[0], gaps[0]), ("target", r["cross_target"], weighted[1], gaps[1])):
                d = P.distance(got, S)
                print(f"pose_cov_paths: {what}: {name} distance to the weighted restatement {d:.3e} (bar {P.bar_of(gap):.3e})")
                assert d > P.bar_of(gap), (what, name, d)


# ---- 2. parameters off the defaults ------------------------------------------------------------------------------------------------------
PARAM_MODES = [(sicp.MODE_EM, 4), (sicp.MODE_GICP, 1)]
LOSS_CASES = [(m, K, a, sq) for m, K in PARAM_MODES for a in (0.5, 10.0) for sq in (0, 1)]


@pytest.mark.parametrize("mode,K,a,sq", LOSS_CASES, ids=[f"{MODE_NAMES[m]}_k{K}_a{a:g}_{'sqloss' if sq else 'cauchy'}" for m, K, a, sq in LOSS_CASES])
def test_cauchy_a_off_the_default(mode, K, a, sq):
    src, sl, tgt, tl, qt, cm = lidar()
    with engine(mode, src, sl, tgt, tl, cm, knn=K, cauchy_a=a, use_sqloss=sq) as e:
        check(e, mode, src, tgt, qt, f"cauchy_a {MODE_NAMES[mode]} K={K} a={a:g} sqloss={sq}")


@pytest.mark.parametrize("eps", [1e-2, 1e-6])
@pytest.mark.parametrize("mode,K", PARAM_MODES, ids=[f"{MODE_NAMES[m]}_k{K}" for m, K in PARAM_MODES])
def test_epsilon_off_the_default(mode, K, eps):
    src, sl, tgt, tl, qt, cm = lidar()
    with engine(mode, src, sl, tgt, tl, cm, knn=K, epsilon=eps) as e:
        check(e, mode, src, tgt, qt, f"epsilon {MODE_NAMES[mode]} K={K} eps={eps:g}")
        ev = np.linalg.eigvalsh(e.covariances(sicp.TARGET)[0][:50])
    assert np.allclose(ev[:, 0], eps, rtol=1e-6) and np.allclose(ev[:, 1:], 1.0, rtol=1e-9)   # the records carry this epsilon


@pytest.mark.parametrize("sq", [0, 1], ids=["cauchy", "sqloss"])
def test_exact_pose_gives_zero_residuals_and_zero_sums(sq):
    """the target is the source moved by a translation that float32 holds exactly, the pose that translation: d = 0 and
    r = 0 on every slot.  Nothing divides by r: every output is finite, S_src = S_tgt = 0 exactly, g = 0, and positive_definite
    says what a Cholesky factorisation of accumulate's H says (H = sum rho' J J^T = 0 here: not positive definite).
    Translation only (R = I) is a restriction of this case, not of the property: a rotated source is not a float32 cloud
    again, so under a rotation d = 0 cannot be had exactly and r = 0 is not tested there"""
    src = np.round(np.asarray(lidar()[0]) * 256.0) / 256.0
    src = np.unique(src.astype(np.float32), axis=0)
    shift = np.array([1.5, -2.25, 0.5], dtype=np.float32)
    tgt = src + shift
    assert np.array_equal(tgt.astype(np.float64), src.astype(np.float64) + shift.astype(np.float64))
    qt = np.array([0, 0, 0, 1.0, 1.5, -2.25, 0.5])
    with engine(sicp.MODE_GICP, src, None, tgt, None, use_sqloss=sq) as e:
        r = e.pose_covariance(qt)
        idx, d2, _ = e.correspondences(qt)
        out28 = e.accumulate(qt)
    assert (idx[:, 0] == np.arange(len(src))).all() and (d2 <= 1e-6).all()
    assert r["active"] == len(src)
    assert np.array_equal(r["hessian21"], out28[:21]) and np.array_equal(r["gradient"], out28[21:27]) and r["cost"] == out28[27]
    for key in ("hessian", "gradient", "cross_source", "cross_target"):
        assert np.isfinite(r[key]).all(), key
    assert np.isfinite(r["cost"])
    assert not r["cross_source"].any() and not r["cross_target"].any() and not r["gradient"].any()
    try:
        np.linalg.cholesky(r["hessian"])
        pd = bool(np.isfinite(np.linalg.inv(r["hessian"])).all())
    except np.linalg.LinAlgError:
        pd = False
    assert bool(r["positive_definite"]) == pd
    assert np.isfinite(r["covariance"]).all() if pd else np.isnan(r["covariance"]).all()
    print(f"pose_cov_paths: exact pose sqloss={sq}: active {r['active']} max |H| {np.abs(r['hessian']).max():.3e} cost {r['cost']:.3e} "
          f"positive_definite {r['positive_definite']}")


# ---- 3. geometry ------------------------------------------------------------------------------------------------------------------------------
def crafted_engine(case, **kw):
    src, sl, tgt, tl = P.case_pair(case)
    return engine(sicp.MODE_EM, src, sl, tgt, tl, knn=case.K, **kw)


@pytest.mark.parametrize("name", list(P.GEOMETRY))
def test_tile_and_owner_geometry(name):
    case = P.GEOMETRY[name]
    src, sl, tgt, tl = P.case_pair(case)
    n_s, n_t, live, gated = P.slots_of_case(case)
    with crafted_engine(case) as e:
        assert e.get_params().gate_sq == P.GATE_SQ
        r, idx, w, _ = check(e, sicp.MODE_EM, src, tgt, P.IDENT, f"geometry {name}")
    runs, dead = P.run_lengths_of(idx, n_t)
    assert idx.shape == (n_s, case.K) and dead == gated and len(runs) == n_t and (runs == case.L).all(), (name, dead, runs)
    assert r["active"] == live
    geo = P.tile_geometry(runs.tolist(), dead)
    P.check_claims(case, geo)
    print(f"pose_cov_paths: geometry {name}: {geo}")


@pytest.mark.parametrize("n_s", P.SOURCE_SIZES)
def test_source_kernel_last_column(n_s):
    src, sl, tgt, tl, qt = P.source_pair(n_s)
    assert len(src) == n_s
    for mode, K in ((sicp.MODE_EM, 4), (sicp.MODE_GICP, 1)):
        with engine(mode, src, sl, tgt, tl, knn=K) as e:
            r, idx, _, _ = check(e, mode, src, tgt, qt, f"source {MODE_NAMES[mode]} K={K} n_s={n_s}")
        assert (idx >= 0).all()      # the last source point's slots are live: its lane's share is in the sums


# ---- 4. origins inside a group ------------------------------------------------------------------------------------------------------------
def _geo_of(case):
    return P.tile_geometry([case.L] * (case.T * case.K), case.g * case.K)


# every crafted case with a chain across a workgroup edge or with a gated tail, in the case list's order, and in their middle
# one job with every slot gated out
GROUP_CRAFTED = [name for name, case in P.GEOMETRY.items() if _geo_of(case)["crossing_workgroup"] >= 1 or case.g > 0]
GROUP_CRAFTED.insert(len(GROUP_CRAFTED) // 2, "ALL_GATED")


def test_jobs_inside_a_group_give_lone_bytes():
    """one sicp_pose_covariance_batch call: [lidar EM K = 4 | every crafted case with a chain across a workgroup edge or with
    a gated tail, and among them one job with every slot gated out | lidar GICP K = 1 without SQLoss | lidar EM K = 20]: 27
    jobs, some 150 000 slots, one group.  The sweep orders its jobs by (K, loss): the Cauchy K = 1 pair comes first, the
    crafted K = 1 jobs behind it, the crafted K = 4 and K = 20 jobs behind and before a lidar pair of their kind -- no
    crafted job is first or last, so its tiles, pieces, flags and columns start away from the scratch's origin"""
    src, sl, tgt, tl, qt, cm = lidar()
    es, qts = [], []
    try:
        es.append(engine(sicp.MODE_EM, src, sl, tgt, tl, cm, knn=4)); qts.append(qt)
        for name in GROUP_CRAFTED:
            if name == "ALL_GATED":
                es.append(crafted_engine(P.GEOMETRY["T37_K1_L9_g1"], gate_sq=1e-30))
            else:
                es.append(crafted_engine(P.GEOMETRY[name]))
            qts.append(P.IDENT)
        es.append(engine(sicp.MODE_GICP, src, sl, tgt, tl, knn=1, use_sqloss=0)); qts.append(qt)
        es.append(engine(sicp.MODE_EM, src, sl, tgt, tl, cm, knn=20)); qts.append(qt)
        n = len(es)
        kinds = [2 * e.get_params().knn + e.get_params().use_sqloss for e in es]
        order = sorted(range(n), key=lambda i: kinds[i])       # (stable, as the sweep's)
        crafted = set(range(1, 1 + len(GROUP_CRAFTED)))
        assert order[0] not in crafted and order[-1] not in crafted and order != list(range(n))
        at = order.index(1 + GROUP_CRAFTED.index("ALL_GATED"))
        assert order[at - 1] in crafted and order[at + 1] in crafted      # the all-gated job lies between crafted jobs
        # one group holds them all: 256 pairs and 2^30 / 152 slots bound a sweep (csrc/pose_cov.cpp)
        slots = len(src) * (4 + 1 + 20) + sum(P.slots_of_case(P.GEOMETRY[m])[0] * P.GEOMETRY[m].K for m in GROUP_CRAFTED if m != "ALL_GATED")
        assert n <= 256 and slots + P.slots_of_case(P.GEOMETRY["T37_K1_L9_g1"])[0] < (1 << 30) // 152
        names = set(GROUP_CRAFTED)
        assert {"T37_K1_L63_g0", "T37_K20_L7_g0", "T3_K1_L2049_g0", "T2_K1_L4104_g0"} <= names      # chains across a workgroup edge
        assert sum(P.GEOMETRY[m].g > 0 for m in names - {"ALL_GATED"}) == sum(c.g > 0 for c in P.GEOMETRY_CASES) >= 16
        lone = [raw(e, q) for e, q in zip(es, qts)]
        out = (sicp.SicpPoseCovarianceResult * n)()
        status = np.full(n, 99, dtype=np.int32)
        q = np.ascontiguousarray(np.stack(qts))
        rc = sicp.lib().sicp_pose_covariance_batch(sicp._handles(es), n, sicp._ptr(q, sicp._dp), 1.0, 1.0, out, sicp._ptr(status, sicp._ip))
        assert rc == sicp.OK and (status == 0).all(), status
        for k in range(n):
            assert bytes(out[k]) == lone[k], (k, (["lidar"] + GROUP_CRAFTED + ["lidar", "lidar"])[k])
        gated = out[1 + GROUP_CRAFTED.index("ALL_GATED")]
        assert gated.active == 0 and gated.positive_definite == 0
        assert all(out[k].active > 0 for k in range(n) if k != 1 + GROUP_CRAFTED.index("ALL_GATED"))
    finally:
        for e in es:
            e.close()


# ---- 5. stream --------------------------------------------------------------------------------------------------------------------------------
def test_stream_on_a_non_default_stack_gives_lone_bytes():
    """EM without SQLoss at cauchy_a = 2: the stream's pass runs the sweep of the lone call, on the stream's params"""
    if "seq" not in _cache:
        _cache["seq"] = synth.lidar_sequence(seed=5, n_scans=2, n_points=2000)
    scans, _, cm = _cache["seq"]
    p = params_of(sicp.MODE_EM, use_sqloss=0, cauchy_a=2.0)
    ident = P.IDENT
    with sicp.Stream(0, p, max_in_flight=2, confusion=cm) as S:
        a, b = S.add_cloud(*scans[0]), S.add_cloud(*scans[1])
        t = S.submit(b, a, ident, pose_covariance=True)
        got = S.drain()
        assert [(g[0], g[1]) for g in got] == [(t, sicp.OK)]
        r = sicp.SicpPoseCovarianceResult()
        assert sicp.lib().sicp_stream_take_pose_covariance(S._s, t, 1.0, 1.0, ctypes.byref(r)) == sicp.OK
    with engine(sicp.MODE_EM, scans[1][0], scans[1][1], scans[0][0], scans[0][1], cm, use_sqloss=0, cauchy_a=2.0) as e:
        q1, _ = e.align(ident)
        assert np.array_equal(got[0][2], q1)
        want = raw(e, q1)
        assert bytes(r) == want
        assert r.active > 0
        check(e, sicp.MODE_EM, scans[1][0], scans[0][0], q1, "stream stack em K=4 a=2 sqloss=0")
