"""accumulate_staged_kernel / solve_one_kernel (csrc/solve_kernels.hip) against the oracle's literal accumulate and solve --
GICPCostFunction::Evaluate on full 3x3 covariances with the Ceres losses, on the indices, weights and covariances the engine
reports -- at every path the kernels have and the rest of the suite does not reach (sizes and bars: tests/accumulate_cases.py,
checked without a GPU by tests/test_accumulate_cases_cpu.py):

 1. the dynamic hand-out of chunks (launches of at least 64 chunks per workgroup; the handle count follows the CU count the HIP
    runtime reports), bit for bit against lone evaluations, again after the counters were reset, and against the oracle;
 2. every instantiation K in {1, 4, 20} x SQLoss x weights present / absent: accumulate, the inner solve by persistent
    launches, ticks and the host loop, and the residency boundary of the persistent solve;
 3. chunk geometry edges: every size on either side of a wave, a workgroup step, a chunk, the 8 chunks parked in LDS, a ragged
    last group -- each with the check that the oracle itself notices a single slot missing there;
 4. dead slots at the edges, everywhere, nowhere but one point, and Semantic targets whose record 0 is special;
 5. cauchy_a, use_sqloss and epsilon away from the defaults.

K = 1 cannot reach the dynamic hand-out's threshold within the 256 pairs of a launch at any size the synthetic scans have
(tests/accumulate_cases.py), so 1. has no K = 1 case.

Bars: H 1e-9 x max |H|, g 1e-9 x max |g| + 1e-9 x max |H|, cost 1e-11 relative (tests/test_gpu_parity.py); where loss or
epsilon leave the defaults, the larger of that and 4 x the float64 oracle's own distance to its np.longdouble restatement on
the same slots.  Everything "bit for bit" has no tolerance."""
import ctypes
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import accumulate_cases as A
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63   # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
HALF_GATE_SHIFT = (0.0, 22.0, 0.0)               # the reference drops 53 % of the mid-size pair's slots there


@pytest.fixture(scope="module")
def cus():
    """compute units of device 0, from the HIP runtime libsicp.so itself links (torch would bring a second copy)"""
    hip = ctypes.CDLL("libamdhip64.so")
    v = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(v), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0) == 0
    assert 1 <= v.value <= 1024, v.value
    print(f"compute units: {v.value}")
    return v.value


def make_engine(mode, **kw):
    p = A.set_params(sicp.default_params(mode), mode, **kw)
    e = sicp.Engine(0, p)
    if mode == sicp.MODE_EM:
        e.set_confusion(synth.confusion_matrix(A.C))
    return e


def set_clouds(e, mode, src, sl, tgt, tl):
    lab = mode != sicp.MODE_GICP
    e.set_source(src, sl if lab else None)
    e.set_target(tgt, tl if lab else None)


def pose_delta(qa, qb):
    D = np.linalg.inv(O.se3_matrix(qa)) @ O.se3_matrix(qb)
    return np.linalg.norm(Rotation.from_matrix(D[:3, :3]).as_rotvec()), np.linalg.norm(D[:3, 3])


def slots_of(e, mode, qt):
    """(idx, w or None, source covariances, target covariances) as the engine reports them"""
    idx, _, w = e.correspondences(qt)
    return idx, (w if mode == sicp.MODE_EM else None), e.covariances(sicp.SOURCE)[0], e.covariances(sicp.TARGET)[0]


def check_accumulate(e, mode, src, tgt, qt, what, measure_oracle=False, **params):
    """sicp_accumulate at qt against the oracle on the engine's slots; run to run the same bits; returns
    (the 28 sums, the reference, the slots)"""
    idx, w, cs, ct = slots_of(e, mode, qt)
    got = e.accumulate(qt)
    assert np.array_equal(got, e.accumulate(qt)), what
    op = A.oracle_params(mode, **params)
    assert op.knn == idx.shape[1]
    ref = O.accumulate(op, qt, src, cs, tgt, ct, idx, w)
    dist = None
    if measure_oracle:
        dist = A.oracle_distance(op, qt, src, cs, tgt, ct, idx, w, ref)
        print(f"{what}: oracle to longdouble H {dist[:21].max():.3e}  g {dist[21:27].max():.3e}  cost {dist[27]:.3e}")
    A.assert_sums(got, ref, what, dist)
    return got, ref, (op, idx, w, cs, ct)


# ---- 1. the dynamic hand-out ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.DYNAMIC_CASES))
def test_dynamic_hand_out_equals_lone_evaluations_and_the_oracle(cus, name):
    """Enough handles on two shared clouds, every one at its own pose, that the launch has at least 8 runs of 8 chunks per
    workgroup: the chunks are fetched from the agent-scope counter of the launch's header.  Every pair's 28 sums are the bits
    of its lone evaluation (static ranges); three launches back to back at other poses give the lone bits of those (the last
    workgroup out reset the counters each time); so does a small batch on the same leader afterwards, and the large one after
    that.  Then the handles
    are registered in lock step: the launch as a node of the tick graph, against lone registrations."""
    mode, knn, n_s = A.DYNAMIC_CASES[name]
    src, sl, tgt, tl, qt0 = A.big_pair()
    src, sl = src[:n_s], sl[:n_s]
    n = A.handles_for_dynamic(cus, n_s, knn)
    total, need = n * A.n_chunks(n_s, knn), A.dynamic_threshold(cus)
    print(f"{name}: {cus} CUs, {n} handles x {A.n_chunks(n_s, knn)} chunks = {total} chunks, threshold {need}")
    assert total >= need and n <= A.MAX_PAIRS and A.n_chunks(n_s, knn) < need
    qts = A.poses_around(qt0, n, seed=41)
    engines, lone, kept = [], [], {}
    try:
        for k in range(n):
            e = make_engine(mode, knn=knn, max_outer=2, reuse_features=1)
            engines.append(e)
            if k == 0:
                set_clouds(e, mode, src, sl, tgt, tl)
            else:
                e.share_cloud(sicp.SOURCE, engines[0], sicp.SOURCE); e.share_cloud(sicp.TARGET, engines[0], sicp.TARGET)
            idx, _, w = e.correspondences(qts[k])
            if k in (0, n - 1):
                kept[k] = (idx, w)
            lone.append(e.accumulate(qts[k]))
        # A handle's partial columns outlive a launch, and a chunk nobody computes would keep the column of the launch
        # before: every batch below runs on columns that a lone evaluation at ANOTHER pose has just filled.
        other = np.roll(qts, 1, axis=0)
        lone, lone_other = np.array(lone), np.array([e.accumulate(q) for e, q in zip(engines, other)])
        assert len({r.tobytes() for r in np.concatenate([lone, lone_other])}) == 2 * n

        def differ(a, b):
            return np.nonzero((a != b).any(axis=1))[0]

        out, _ = sicp.accumulate_batch(engines, qts)
        assert np.array_equal(out, lone), differ(out, lone)
        again, _ = sicp.accumulate_batch(engines, other, repeat=3)
        assert np.array_equal(again, lone_other), differ(again, lone_other)
        few, _ = sicp.accumulate_batch(engines[:5], qts[:5])
        assert np.array_equal(few, lone[:5])
        out, _ = sicp.accumulate_batch(engines, qts)
        assert np.array_equal(out, lone), differ(out, lone)
        cs, ct = engines[0].covariances(sicp.SOURCE)[0], engines[0].covariances(sicp.TARGET)[0]
        op = A.oracle_params(mode, knn=knn)
        for k, (idx, w) in kept.items():
            assert (idx >= 0).mean() > 0.9
            A.assert_sums(out[k], O.accumulate(op, qts[k], src, cs, tgt, ct, idx, w), f"{name}, pair {k}")
        # The same launch inside the tick graph of sicp_align_batch: [accumulate, LM step] x lm_batch replayed on ONE header, every
        # accumulate at the poses the step before it left -- nothing but the last workgroup out resets the counters in between.
        # (Two outer iterations; while all pairs iterate the launch is over the threshold.)
        res = sicp.align_batch(engines, qts)
        assert len({q.tobytes() for q, _ in res}) == n
        for k in (0, n // 2, n - 1):
            q1, s1 = engines[k].align(qts[k])
            assert np.array_equal(res[k][0], q1), (k, res[k][0], q1)
            for key in ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost"):
                assert res[k][1][key] == s1[key], (k, key, res[k][1][key], s1[key])
            assert s1["total_evals"] >= 3
    finally:
        for e in engines:
            e.close()


# ---- 2. every instantiation ---------------------------------------------------------------------------------------------------------------
def matrix_id(mode, knn, sq):
    return A.case_id(mode, knn, "sqloss" if sq else "cauchy")


@pytest.mark.parametrize("mode,knn,sq", A.MATRIX, ids=[matrix_id(*c) for c in A.MATRIX])
def test_every_instantiation_accumulates_and_solves_like_the_oracle(mode, knn, sq):
    """K x SQLoss x (EM: weights present, GICP: absent): sicp_accumulate against the oracle, sicp_solve against the oracle's
    trust-region solve (equal iteration counts), and the persistent solve, the tick graph and the host loop bit for bit"""
    src, sl, tgt, tl, qt = A.mid_pair()
    what = matrix_id(mode, knn, sq)
    start = A.far_pose(qt, (0.05, -0.03, 0.02))
    solved = {}
    for lm in (1, 2, 0):
        with make_engine(mode, knn=knn, use_sqloss=sq, lm_on_device=lm) as e:
            set_clouds(e, mode, src, sl, tgt, tl)
            if lm == 1:
                got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, start, what, knn=knn, use_sqloss=sq)
                assert (idx >= 0).mean() > 0.9
                assert (w is not None and (w[idx >= 0] != 1.0).any()) if mode == sicp.MODE_EM else w is None
            else:
                e.correspondences(start)
            est, info = e.solve(start)
            est2, info2 = e.solve(start)
            assert np.array_equal(est, est2) and info == info2, (what, lm)
            solved[lm] = (est, info)
    for lm in (2, 0):
        assert np.array_equal(solved[1][0], solved[lm][0]), (what, lm, solved[1], solved[lm])
        assert solved[1][1] == solved[lm][1], (what, lm, solved[1][1], solved[lm][1])
    oest, oinfo = O.solve(op, src, cs, tgt, ct, idx, w, start)
    est, info = solved[1]
    rot, tr = pose_delta(est, oest)
    print(f"{what}: solve {info['lm_iters']} iterations (oracle {oinfo['lm_iters']}), pose {rot:.2e} rad {tr:.2e} m, "
          f"cost {info['cost']:.12g} (oracle {oinfo['cost']:.12g})")
    assert info["lm_iters"] == oinfo["lm_iters"] and info["lm_iters"] >= 2
    assert rot < 1e-7 and tr < 1e-7
    assert np.isclose(info["cost"], oinfo["cost"], rtol=1e-9, atol=0)


def test_persistent_solve_at_its_residency_boundary(cus):
    """knn = 20 sources of exactly CUs - 1 chunks (one workgroup per chunk and the master: the persistent solve fits) and of
    CUs chunks (it does not: ticks): sicp_align with the persistent solve allowed against ticks only -- the same pose bits,
    the same counters, and persistent launches on the fitting side only"""
    src, sl, tgt, tl, _ = A.big_pair()
    fits = A.largest_source_with_chunks(min(cus, 257) - 1, 20)
    for n_s in (fits, fits + 1):
        assert A.solo_fits(n_s, 20, cus) == (n_s == fits) and A.n_chunks(n_s, 20) == min(cus, 257) - 1 + (n_s != fits)
        got = {}
        for lm in (1, 2):
            with make_engine(sicp.MODE_EM, knn=20, lm_on_device=lm, max_outer=3) as e:
                set_clouds(e, sicp.MODE_EM, src[:n_s], sl[:n_s], tgt, tl)
                got[lm] = e.align(IDENT)
        assert np.array_equal(got[1][0], got[2][0]), (n_s, got[1][0], got[2][0])
        for key in ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost"):
            assert got[1][1][key] == got[2][1][key], (n_s, key)
        print(f"{n_s} points, {A.n_chunks(n_s, 20)} chunks: accumulate launches {got[1][1]['acc_launches']} (persistent allowed) "
              f"against {got[2][1]['acc_launches']} (ticks)")
        if n_s == fits:
            assert got[1][1]["acc_launches"] < got[2][1]["acc_launches"]
        else:
            assert got[1][1]["acc_launches"] == got[2][1]["acc_launches"]


# ---- 3. chunk geometry edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,knn,n_s", A.EDGE_CASES, ids=[A.case_id(*c) for c in A.EDGE_CASES])
def test_chunk_geometry_edges(mode, knn, n_s):
    """the first n_s source points, every slot live (gate wide open): sums against the oracle, and the oracle itself moves by
    more than 1000 bars when the last source point's slots, the first group of the last chunk or slot 0 are taken away"""
    src, sl, tgt, tl, qt = A.mid_pair(n_s)
    what = A.case_id(mode, knn, n_s)
    with make_engine(mode, knn=knn, gate_sq=A.GATE_OPEN) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, qt, what, knn=knn, gate_sq=A.GATE_OPEN)
    assert idx.shape == (n_s, knn) and (idx >= 0).all()
    assert A.n_chunks(n_s, knn) == A.EDGE_EXPECT[(knn, n_s)][0]
    for gone, less in A.removals(idx).items():
        other = O.accumulate(op, qt, src, cs, tgt, ct, less, w)
        assert A.moved_beyond(ref, other), (what, gone, np.abs(other - ref) / A.project_bars(ref))
        assert A.excess(got, other, A.project_bars(other))[0] > 1.0, (what, gone)


# ---- 4. dead slots --------------------------------------------------------------------------------------------------------------------------
DEAD_MODES = [(sicp.MODE_EM, 4, 3000), (sicp.MODE_GICP, 1, 2999)]   # (K = 1, odd: the last group is the last point and one past the end)
DEAD_IDS = [A.case_id(*c) for c in DEAD_MODES]


@pytest.mark.parametrize("mode,knn,n_s", DEAD_MODES, ids=DEAD_IDS)
def test_half_of_the_slots_gated_out(mode, knn, n_s):
    src, sl, tgt, tl, qt = A.mid_pair(n_s)
    far = A.far_pose(qt, HALF_GATE_SHIFT)
    with make_engine(mode, knn=knn) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, far, "half dead")
    dead = (idx < 0).mean()
    print(f"dead slots: {100 * dead:.1f} %")
    assert 0.3 <= dead <= 0.7
    if knn > 1:   # source points with some of their slots dead, not only all or none
        part = ((idx < 0).any(axis=1) & (idx >= 0).any(axis=1)).sum()
        assert part > 20, part


@pytest.mark.parametrize("mode,knn,n_s", DEAD_MODES, ids=DEAD_IDS)
def test_every_slot_gated_out(mode, knn, n_s):
    """a gate nothing passes: all 28 sums are exactly zero (and finite: a dead slot is evaluated on target 0 and weighted by
    zero), lone and in a batch beside a live pair"""
    src, sl, tgt, tl, qt = A.mid_pair(n_s)
    with make_engine(mode, knn=knn, gate_sq=1e-30) as e, make_engine(mode, knn=knn) as live:
        set_clouds(e, mode, src, sl, tgt, tl)
        set_clouds(live, mode, src, sl, tgt, tl)
        idx, _, w = e.correspondences(qt)
        assert (idx == -1).all() and (w == 0).all()
        got = e.accumulate(qt)
        assert np.isfinite(got).all() and (got == 0).all(), got
        live.correspondences(qt)
        want = live.accumulate(qt)
        out, _ = sicp.accumulate_batch([e, live, e], np.tile(qt, (3, 1)))
        assert (out[0] == 0).all() and (out[2] == 0).all() and np.array_equal(out[1], want)
        est, info = e.solve(qt)
        assert np.isfinite(est).all() and max(pose_delta(est, qt)) < 1e-12 and info["cost"] == 0.0, (est, info)


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("mode,knn,n_s", DEAD_MODES, ids=DEAD_IDS)
def test_one_source_point_dead(mode, knn, n_s, where):
    """the first or the last source point lies a kilometre away: its slots, and only they, are gated out"""
    src, sl, tgt, tl, qt = A.mid_pair(n_s)
    src = np.array(src)
    row = 0 if where == "first" else n_s - 1
    src[row] += np.float32(1000.0)
    with make_engine(mode, knn=knn) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, qt, f"{where} source point dead")
    assert (idx[row] == -1).all() and (np.delete(idx, row, axis=0) >= 0).all()
    # the reference notices one live slot more or less right there
    neighbour = 1 if where == "first" else n_s - 2
    less = idx.copy(); less[neighbour, 0] = -1
    assert A.moved_beyond(ref, O.accumulate(op, qt, src, cs, tgt, ct, less, w))


def test_semantic_first_target_class_is_skipped():
    """the class of device record 0 has too few source points: no slot refers to it, every dead slot is evaluated on it"""
    src, sl, tgt, tl, qt, first = A.semantic_first_class_small()
    mode = sicp.MODE_SEMANTIC
    with make_engine(mode) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, qt, "semantic, first class skipped")
    assert tl[0] == first and (sl == first).sum() == 300 and (idx[sl == first] == -1).all() and (idx[sl != first] >= 0).all()
    assert not np.isin(idx[idx >= 0], np.nonzero(tl == first)[0]).any()


def test_semantic_one_point_target_class():
    """target point 0 is a class of its own: 450 source points meet that one record (whatever covariance the engine reports
    for a neighbourhood of one point, the oracle is given the same), a class without a target is dead"""
    src, sl, tgt, tl, qt, lone = A.semantic_one_point_class()
    mode = sicp.MODE_SEMANTIC
    with make_engine(mode) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, qt, "semantic, one-point class")
    assert tl[0] == lone and (tl == lone).sum() == 1 and (sl == lone).sum() == 450
    assert (idx[sl == lone] == 0).all()
    gone = ~np.isin(sl, tl)
    assert gone.sum() == 700 and (idx[gone] == -1).all() and (idx[~gone] >= 0).all()
    assert np.isfinite(ct[0]).all() and np.isfinite(cs).all()


# ---- 5. loss and epsilon --------------------------------------------------------------------------------------------------------------------
LOSS_MODES = [(sicp.MODE_EM, 4), (sicp.MODE_GICP, 1)]
LOSS_CASES = [(m, k, a, sq) for m, k in LOSS_MODES for a in A.LOSS_A for sq in (1, 0)]


@pytest.mark.parametrize("mode,knn,a,sq", LOSS_CASES, ids=[A.case_id(m, k, f"a{a:g}", "sqloss" if sq else "cauchy") for m, k, a, sq in LOSS_CASES])
def test_cauchy_scale_and_loss_stack(mode, knn, a, sq):
    src, sl, tgt, tl, qt = A.mid_pair()
    at = A.far_pose(qt, (0.05, -0.03, 0.02))
    with make_engine(mode, knn=knn, cauchy_a=a, use_sqloss=sq) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, _ = check_accumulate(e, mode, src, tgt, at, f"a = {a:g}, sqloss = {sq}", measure_oracle=True, knn=knn, cauchy_a=a, use_sqloss=sq)
    assert (np.abs(ref[21:27]) > 0).all() and ref[27] > 0


@pytest.mark.parametrize("mode,knn", LOSS_MODES, ids=[A.case_id(*c) for c in LOSS_MODES])
def test_loss_parameters_change_the_sums(mode, knn):
    """(the cases above compare at one setting each: a kernel that ignored cauchy_a or use_sqloss would fail them, and the
    settings do differ from each other by far more than a bar)"""
    src, sl, tgt, tl, qt = A.mid_pair()
    at = A.far_pose(qt, (0.05, -0.03, 0.02))
    sums = {}
    for a, sq in ((3.0, 1), (1.5, 1), (3.0, 0)):
        with make_engine(mode, knn=knn, cauchy_a=a, use_sqloss=sq) as e:
            set_clouds(e, mode, src, sl, tgt, tl)
            e.correspondences(at)
            sums[(a, sq)] = e.accumulate(at)
    for other in ((1.5, 1), (3.0, 0)):
        assert A.moved_beyond(sums[(3.0, 1)], sums[other]), other


@pytest.mark.parametrize("eps", A.EPSILONS)
@pytest.mark.parametrize("mode,knn", LOSS_MODES, ids=[A.case_id(*c) for c in LOSS_MODES])
def test_epsilon_away_from_the_default(mode, knn, eps):
    """epsilon = 1e-6 puts 1 / (2 epsilon) between a residual along both normals and the sums: the bar is 4 x what float64
    itself loses in the literal formulas there, measured on the same slots"""
    src, sl, tgt, tl, qt = A.mid_pair()
    at = A.far_pose(qt, (0.05, -0.03, 0.02))
    with make_engine(mode, knn=knn, epsilon=eps) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        got, ref, (op, idx, w, cs, ct) = check_accumulate(e, mode, src, tgt, at, f"epsilon = {eps:g}", measure_oracle=True, knn=knn, epsilon=eps)
    # the covariances the engine reports carry this epsilon: I - (1 - eps) n n^T has the eigenvalues (1, 1, eps)
    ev = np.linalg.eigvalsh(cs[:50])
    assert np.allclose(ev[:, 0], eps, rtol=1e-6) and np.allclose(ev[:, 1:], 1.0, rtol=1e-9)
