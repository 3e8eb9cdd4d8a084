"""The full-matrix covariance path -- sicp_set_covariances with matrices that are not I - (1 - eps) n n^T, Cloud::cov_general,
accumulate_general_kernel (csrc/solve_kernels.hip) with its own chunk split and closed-form Jacobian, the trust-region loop on
the host, the six packed doubles per point in device order -- against the oracle's literal Evaluate, solve and outer loop on
the indices the engine reports and the matrices it hands back (cases and bars: tests/general_cov_cases.py, checked without a GPU
by tests/test_general_cov_cases_cpu.py):

 1. every instantiation: K in {1, 4, 20} x loss stack x which cloud is general x matrix family, loss scale and epsilon;
 2. the general kernel's split (one slot, either side of a lane stride and of a chunk, several chunks with a ragged `per`),
    dead slots by the gate, all dead, non-finite points with NaN rows;
 3. SICP_MODE_SEMANTIC, whose device order is label-grouped: given order and shuffled caller order, matrices shuffled alike;
 4. solve and align on the host loop against the oracle's trust region and outer loop, lm_on_device without effect, a
    singular system;
 5. state: cov_general cleared or honoured after every call that replaces, recomputes, shares or recycles a cloud, the
    classifier's tolerances, refusals that change nothing, the multi-pair entry points.

sicp_solve returns no termination status and no accept / reject sequence: they are read off lm_iters (one per attempt), evals
(1 + the attempts that are not invalid) and whether the pose is still the start, as tests/test_gpu_solver_options.py does.

Bars: accumulate_cases.project_bars (H 1e-9 x max |H|, g 1e-9 x max |g| + 1e-9 x max |H|, cost 1e-11 relative), widened only by
4 x the float64 oracle's distance to its np.longdouble restatement on the same slots (at most a tenth of the bar: the CPU
module); poses 1e-7 rad / 1e-7 m.  Everything "bits" or "bytes" has no tolerance."""
import ctypes
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import accumulate_cases as A
import general_cov_cases as G
import oracle_lib as O
import synth

pytestmark = pytest.mark.gpu

sicp = importlib.import_module("semantic-icp_amd")
GICP, SEM = sicp.MODE_GICP, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
COUNTERS = ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost")
NEAR_SHIFT = (0.05, -0.03, 0.02)


def make_engine(mode, **kw):
    """GICP keeps caller covariances over an align() only with reuse_features = 1 (include/sicp.h)"""
    kw.setdefault("reuse_features", 1)
    return sicp.Engine(0, A.set_params(sicp.default_params(mode), mode, **kw))


def load(e, mode, src, sl, tgt, tl, cs=None, ct=None):
    lab = mode != GICP
    e.set_source(src, sl if lab else None)
    e.set_target(tgt, tl if lab else None)
    if cs is not None:
        e.set_covariances(SRC, cs)
    if ct is not None:
        e.set_covariances(TGT, ct)
    return e


def last_error(e):
    return sicp.lib().sicp_last_error(e._h).decode()


def pose_delta(qa, qb):
    D = np.linalg.inv(O.se3_matrix(qa)) @ O.se3_matrix(qb)
    return np.linalg.norm(Rotation.from_matrix(D[:3, :3]).as_rotvec()), np.linalg.norm(D[:3, 3])


def cov_bytes(e):
    """what sicp_covariances hands back for both clouds, through both of its paths"""
    out = []
    for which in (SRC, TGT):
        cov, nrm, _, _ = e.covariances(which)
        assert cov.tobytes() == e.covariance_matrices(which).tobytes()
        out.append((cov.tobytes(), nrm.tobytes()))
    return out


def check_given_back(e, cs, ct):
    """a general cloud hands back the given bytes and NaN normals; a cloud of the engine's form its normals"""
    for which, given in ((SRC, cs), (TGT, ct)):
        cov, nrm, _, _ = e.covariances(which)
        assert cov.tobytes() == e.covariance_matrices(which).tobytes()
        if given is None:
            assert np.isfinite(nrm).all() and np.isfinite(cov).all()
        else:
            assert cov.tobytes() == np.ascontiguousarray(given).tobytes() and np.isnan(nrm).all(), which


def check_accumulate(e, mode, src, tgt, qt, what, **params):
    """sicp_accumulate at qt against the oracle on the engine's slots and matrices; run to run the same bits; returns
    (the 28 sums, the reference, (oracle parameters, idx, source matrices, target matrices))"""
    idx, _, _ = e.correspondences(qt)
    cs, ct = e.covariances(SRC)[0], e.covariances(TGT)[0]
    got = e.accumulate(qt)
    assert got.tobytes() == e.accumulate(qt).tobytes(), what
    op = G.oracle_params(mode, **params)
    assert op.knn == idx.shape[1]
    ref = O.accumulate(op, qt, src, cs, tgt, ct, idx, None)
    dist = G.oracle_distance(op, qt, src, cs, tgt, ct, idx, None, ref)
    w = G.widening(ref, dist)
    print(f"{what}: 4 x oracle distance / project bar  H {w[0]:.2e}  g {w[1]:.2e}  cost {w[2]:.2e}")
    G.assert_sums(got, ref, what, dist)
    return got, ref, (op, idx, cs, ct)


def same_align(a, b):
    return a[0].tobytes() == b[0].tobytes() and all(a[1][k] == b[1][k] for k in COUNTERS)


def check_solve(e, what, start, op, src, cs, tgt, ct):
    """sicp_solve from `start` against the oracle's trust region on the engine's slots: (pose, info, the expectation)"""
    idx, _, _ = e.correspondences(start)
    est, info = e.solve(start)
    ex = G.expectation(op, src, cs, tgt, ct, idx, None, start)
    rot, tr = pose_delta(ex["pose"], est)
    print(f"{what}: status {ex['status']} {ex['seq']}  lm_iters {info['lm_iters']} (oracle {ex['lm_iters']}) evals {info['evals']} "
          f"({ex['evals']}) pose to oracle {rot:.3e} rad {tr:.3e} m cost rel {abs(info['cost'] - ex['cost']) / max(abs(ex['cost']), 1e-300):.3e}")
    assert (info["lm_iters"], info["evals"]) == (ex["lm_iters"], ex["evals"]), (what, info, ex["seq"])
    assert np.array_equal(est, start) == ex["unchanged"], what
    assert rot < G.POSE_BOUND and tr < G.POSE_BOUND, (what, rot, tr)
    assert np.isclose(info["cost"], ex["cost"], rtol=1e-9, atol=0), (what, info["cost"], ex["cost"])
    return est, info, ex


def check_align(e, what, start, op, src, cs, tgt, ct, sem):
    """sicp_align from `start` against the outer loop replayed around the oracle's solve on the engine's slots"""
    qt, st = e.align(start)

    def slots(pose):
        return e.correspondences(pose)[0], None

    rq, r_outer, r_iters, r_evals, _ = G.outer_replay(op, slots, src, cs, tgt, ct, start, sem)
    rot, tr = pose_delta(rq, qt)
    print(f"{what}: align outer {st['outer_iters']} ({r_outer}) lm {st['total_lm_iters']} ({r_iters}) evals {st['total_evals']} ({r_evals}) "
          f"pose to oracle {rot:.3e} rad {tr:.3e} m")
    assert (st["outer_iters"], st["total_lm_iters"], st["total_evals"]) == (r_outer, r_iters, r_evals), (what, st)
    assert rot < G.POSE_BOUND and tr < G.POSE_BOUND, (what, rot, tr)
    return qt, st


# ---- 1. every instantiation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn,sq,which,fam", G.INSTANTIATIONS, ids=[G.inst_id(*c) for c in G.INSTANTIATIONS])
def test_every_instantiation_accumulates_like_the_oracle(knn, sq, which, fam):
    src, sl, tgt, tl, qt = G.mid_pair()
    cs, ct = G.matrices(fam, which, len(src), len(tgt))
    what = G.inst_id(knn, sq, which, fam)
    with load(make_engine(GICP, knn=knn, use_sqloss=sq), GICP, src, sl, tgt, tl, cs, ct) as e:
        check_given_back(e, cs, ct)
        for k, pose in enumerate((qt, A.poses_around(qt, 3, seed=5)[1])):
            got, ref, (op, idx, bs, bt) = check_accumulate(e, GICP, src, tgt, pose, f"{what} pose {k}", knn=knn, use_sqloss=sq)
            assert idx.shape == (len(src), knn) and (idx >= 0).mean() > 0.9
            assert (np.abs(ref[21:27]) > 0).all() and ref[27] > 0
        check_given_back(e, cs, ct)


@pytest.mark.parametrize("knn,sq,which,fam,kw", G.LOSS_CASES, ids=[G.inst_id(*c[:4], *c[4].items()) for c in G.LOSS_CASES])
def test_loss_scale_and_epsilon(knn, sq, which, fam, kw):
    src, sl, tgt, tl, qt = G.mid_pair()
    cs, ct = G.matrices(fam, which, len(src), len(tgt))
    with load(make_engine(GICP, knn=knn, use_sqloss=sq, **kw), GICP, src, sl, tgt, tl, cs, ct) as e:
        got, ref, (op, idx, bs, bt) = check_accumulate(e, GICP, src, tgt, qt, G.inst_id(knn, sq, which, fam, kw), knn=knn, use_sqloss=sq, **kw)
        check_given_back(e, cs, ct)
    base = O.accumulate(G.oracle_params(GICP, knn=knn, use_sqloss=sq), qt, src, bs, tgt, bt, idx, None)
    if "cauchy_a" in kw:      # the setting is read: the default's sums are far away
        assert A.moved_beyond(ref, base)
    else:                     # epsilon moves the engine's side only: its matrices carry it, the general ones came back as given
        ev = np.linalg.eigvalsh(bt[:50])
        assert np.allclose(ev[:, 0], kw["epsilon"], rtol=1e-6) and np.allclose(ev[:, 1:], 1.0, rtol=1e-9)


# ---- 2. the general kernel's split ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n_s", G.SPLIT_CASES, ids=[f"k{K}-{n}" for K, n in G.SPLIT_CASES])
def test_split_edges(K, n_s):
    """the first n_s source points, every slot live, both clouds general: sums against the oracle, which itself moves by more
    than 1000 bars when the first slot of a chunk's range, the last slot or slot 0 dies -- and the engine's sums are then out"""
    src, sl, tgt, tl, qt = G.mid_pair(n_s)
    cs, ct = G.matrices("spd", "both", n_s, len(tgt))
    with load(make_engine(GICP, knn=K, gate_sq=G.GATE_OPEN), GICP, src, sl, tgt, tl, cs, ct) as e:
        got, ref, (op, idx, bs, bt) = check_accumulate(e, GICP, src, tgt, qt, f"k{K}-{n_s}", knn=K, gate_sq=G.GATE_OPEN)
    assert idx.shape == (n_s, K) and (idx >= 0).all()
    for gone, less in G.split_removals(idx).items():
        other = O.accumulate(op, qt, src, bs, tgt, bt, less, None)
        assert A.moved_beyond(ref, other), (gone, np.abs(other - ref) / A.project_bars(ref))
        assert A.excess(got, other, A.project_bars(other))[0] > 1.0, gone


DEAD = [(1, 2999), (4, 3000)]


@pytest.mark.parametrize("K,n_s", DEAD, ids=[f"k{K}-{n}" for K, n in DEAD])
def test_half_of_the_slots_gated_out(K, n_s):
    src, sl, tgt, tl, qt = G.mid_pair(n_s)
    cs, ct = G.matrices("spd", "both", n_s, len(tgt))
    with load(make_engine(GICP, knn=K), GICP, src, sl, tgt, tl, cs, ct) as e:
        got, ref, (op, idx, bs, bt) = check_accumulate(e, GICP, src, tgt, G.far_pose(qt, G.HALF_GATE_SHIFT), f"half dead k{K}", knn=K)
    dead = (idx < 0).mean()
    print(f"dead slots: {100 * dead:.1f} %")
    assert 0.3 <= dead <= 0.7


@pytest.mark.parametrize("K,n_s", DEAD, ids=[f"k{K}-{n}" for K, n in DEAD])
def test_every_slot_dead(K, n_s):
    """a pose ten kilometres off (every neighbour beyond the gate), and a gate nothing passes: all 28 sums exactly zero"""
    src, sl, tgt, tl, qt = G.mid_pair(n_s)
    cs, ct = G.matrices("spd", "both", n_s, len(tgt))
    away = G.far_pose(qt, (0.0, 1e4, 0.0))
    for at, kw in ((away, {}), (qt, dict(gate_sq=1e-30))):
        with load(make_engine(GICP, knn=K, **kw), GICP, src, sl, tgt, tl, cs, ct) as e:
            idx, _, _ = e.correspondences(at)
            assert (idx == -1).all()
            got = e.accumulate(at)
            assert got.tobytes() == np.zeros(28).tobytes(), got
            est, info = e.solve(at)      # a zero gradient: the solve ends at its first evaluation, on the start's bits
            assert info == dict(lm_iters=0, evals=1, cost=0.0) and est.tobytes() == np.asarray(at, dtype=np.float64).tobytes(), (est, info)


@pytest.mark.parametrize("K", [1, 4])
def test_non_finite_points_with_nan_rows(K):
    """3 % of either cloud are non-finite points whose rows of cov9 are NaN: accepted (entries of non-finite points are ignored),
    handed back as NaN, the finite rows as given, and the sums are the oracle's on the finite points"""
    src, sl, tgt, tl, qt = G.mid_pair()
    cs, ct = G.matrices("spd", "both", len(src), len(tgt))
    ps, cps, bad_s = G.with_non_finite_rows(src, cs, seed=3)
    pt, cpt, bad_t = G.with_non_finite_rows(tgt, ct, seed=4)
    with load(make_engine(GICP, knn=K), GICP, ps, sl, pt, tl, cps, cpt) as e:
        assert e.cloud_size(SRC) == (len(ps), int((~bad_s).sum())) and e.cloud_size(TGT) == (len(pt), int((~bad_t).sum()))
        for which, given, bad in ((SRC, cps, bad_s), (TGT, cpt, bad_t)):
            cov, nrm, _, _ = e.covariances(which)
            assert np.isnan(cov[bad]).all() and cov[~bad].tobytes() == given[~bad].tobytes() and np.isnan(nrm).all()
        idx, _, _ = e.correspondences(qt)
        assert (idx[bad_s] == -1).all() and (idx[~bad_s] >= 0).mean() > 0.9 and not bad_t[idx[idx >= 0]].any()
        got = e.accumulate(qt)
        assert got.tobytes() == e.accumulate(qt).tobytes()
    fs, fcs = G.finite_for_oracle(ps, cps, bad_s)
    ft, fct = G.finite_for_oracle(pt, cpt, bad_t)
    op = G.oracle_params(GICP, knn=K)
    ref = O.accumulate(op, qt, fs, fcs, ft, fct, idx, None)
    G.assert_sums(got, ref, f"non-finite rows k{K}", G.oracle_distance(op, qt, fs, fcs, ft, fct, idx, None, ref))
    # a finite point next to a non-finite one carries its own row: the reference notices a slot more or less there
    row = int(np.nonzero(bad_s)[0][0]) + 1
    while bad_s[row] or idx[row, 0] < 0:
        row += 1
    less = idx.copy(); less[row, 0] = -1
    assert A.moved_beyond(ref, O.accumulate(op, qt, fs, fcs, ft, fct, less, None))


# ---- 3. Semantic clouds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", G.WHICH)
@pytest.mark.parametrize("name", list(G.SEMANTIC_FIXTURES))
def test_semantic_clouds_in_given_and_shuffled_order(name, which):
    """label-grouped device order, skipped classes: sums, solve and align against the oracle in the given order and with both
    clouds' caller order shuffled (matrices alike); the two runs agree with each other to the same bars"""
    runs = []
    for shuffled in (False, True):
        src, sl, tgt, tl, qt, ps, pt = G.semantic_case(name, shuffled)
        cs, ct = G.semantic_matrices(name, which, shuffled)
        what = f"semantic {name} {which}{' shuffled' if shuffled else ''}"
        with load(make_engine(SEM, max_outer=3), SEM, src, sl, tgt, tl, cs, ct) as e:
            check_given_back(e, cs, ct)
            got, ref, (op, idx, bs, bt) = check_accumulate(e, SEM, src, tgt, qt, what)
            assert 0.5 < (idx >= 0).mean() < 1.0 and (sl[idx[:, 0] >= 0] == tl[idx[idx >= 0]]).all()
            op.max_outer = 3
            est, info, ex = check_solve(e, what, qt, op, src, bs, tgt, bt)
            assert ex["status"] == 0 and info["lm_iters"] >= 2
            pose, st = check_align(e, what, qt, op, src, bs, tgt, bt, True)
            assert same_align(e.align(qt), (pose, st))
            check_given_back(e, cs, ct)
        # a point keeps its slots whatever the caller's order: the shuffled run's indices are the given run's, renamed
        runs.append((got, est, info, pose, st, idx, ps, pt))
    (g0, e0, i0, p0, s0, idx0, _, _), (g1, e1, i1, p1, s1, idx1, ps, pt) = runs
    live = idx1 >= 0
    assert np.array_equal(live, idx0[ps] >= 0) and np.array_equal(pt[idx1[live]], idx0[ps][live])
    assert A.excess(g1, g0, A.project_bars(g0))[0] <= 1.0, (g0, g1)
    assert (i0["lm_iters"], i0["evals"]) == (i1["lm_iters"], i1["evals"]) and max(pose_delta(e0, e1)) < G.POSE_BOUND
    assert all(s0[k] == s1[k] for k in COUNTERS[:3]) and max(pose_delta(p0, p1)) < G.POSE_BOUND


# ---- 4. solve and align on the host loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn,sq,which", G.SOLVE_CASES, ids=[G.inst_id(k, s, w, "spd") for k, s, w in G.SOLVE_CASES])
def test_solve_and_align_like_the_oracle_on_every_placement(knn, sq, which):
    """sicp_solve from a near and a far start (the far one rejects steps) and sicp_align against the oracle; lm_on_device in
    {0, 1, 2} gives the same bytes and counters: a general pair always takes the host loop"""
    src, sl, tgt, tl, qt = G.mid_pair()
    cs, ct = G.matrices("spd", which, len(src), len(tgt))
    what = G.inst_id(knn, sq, which, "spd")
    starts = {"near": G.far_pose(qt, NEAR_SHIFT), "far": G.far_start(qt)}
    got = {}
    for lm in (0, 1, 2):
        with load(make_engine(GICP, knn=knn, use_sqloss=sq, lm_on_device=lm, max_outer=3), GICP, src, sl, tgt, tl, cs, ct) as e:
            out = []
            if lm == 0:
                bs, bt = e.covariances(SRC)[0], e.covariances(TGT)[0]
                op = G.oracle_params(GICP, knn=knn, use_sqloss=sq)
                op.max_outer = 3
                for name, start in starts.items():
                    est, info, ex = check_solve(e, f"{what} {name}", start, op, src, bs, tgt, bt)
                    assert ex["status"] == 0 and "a" in ex["seq"]
                    if name == "far":
                        assert "r" in ex["seq"][:-1], ex["seq"]
                    out.append((est.tobytes(), tuple(sorted(info.items()))))
                pose, st = check_align(e, what, starts["near"], op, src, bs, tgt, bt, False)
                assert st["outer_iters"] >= 2
            else:
                for start in starts.values():
                    e.correspondences(start)
                    est, info = e.solve(start)
                    out.append((est.tobytes(), tuple(sorted(info.items()))))
                pose, st = e.align(starts["near"])
            out.append((pose.tobytes(), tuple(st[k] for k in COUNTERS)))
            got[lm] = out
    assert got[1] == got[0] and got[2] == got[0], what


def test_a_singular_system_ends_at_its_start():
    """one live pair whose two matrices are all zero: A = 0, the sums are not finite; sicp_solve ends as the oracle's trace
    does (the first evaluation fails: no iteration, one evaluation) with the start's bits, sicp_align returns"""
    src, sl, tgt, tl, qt = G.mid_pair(1)
    tgt = tgt[:1]
    z = np.zeros((1, 3, 3))
    op = G.oracle_params(GICP, knn=1, gate_sq=G.GATE_OPEN)
    for lm in (0, 1):
        with load(make_engine(GICP, knn=1, gate_sq=G.GATE_OPEN, lm_on_device=lm), GICP, src, None, tgt, None, z, z) as e:
            check_given_back(e, z, z)
            idx, _, _ = e.correspondences(qt)
            assert idx.tolist() == [[0]]
            assert not np.isfinite(e.accumulate(qt)).all()
            ex = G.expectation(op, src, z, tgt, z, idx, None, qt)
            assert ex["status"] == 3 and ex["unchanged"]
            est, info = e.solve(qt)
            assert (info["lm_iters"], info["evals"]) == (ex["lm_iters"], ex["evals"]) == (0, 1)
            assert est.tobytes() == np.asarray(qt, dtype=np.float64).tobytes()
            pose, st = e.align(qt)
            assert pose.tobytes() == np.asarray(qt, dtype=np.float64).tobytes() and st["outer_iters"] == 1, (pose, st)
            # and the handle is fine afterwards
            e.set_covariances(SRC, G.family("spd", "source", 1)); e.set_covariances(TGT, G.family("spd", "target", 1))
            e.correspondences(qt)
            assert np.isfinite(e.accumulate(qt)).all()


# ---- 5. state -------------------------------------------------------------------------------------------------------------------------------
N_STATE = 2500


def state_pair():
    src, sl, tgt, tl, qt = G.mid_pair(N_STATE)
    return src, tgt, G.far_pose(qt, NEAR_SHIFT)


def normal_form(n, seed, eps=1e-3):
    """n exactly symmetric matrices I - (1 - eps) n n^T with seeded unit normals (not the engine's own)"""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.eye(3) - (1.0 - eps) * (v[:, :, None] * v[:, None, :])


def snapshot(e, qt, align=True, **_):
    """(accumulate bits after a search at qt, align bits and counters) of a handle"""
    e.correspondences(qt)
    acc = e.accumulate(qt).tobytes()
    if not align:
        return acc, None
    pose, st = e.align(qt)
    return acc, (pose.tobytes(), tuple(st[k] for k in COUNTERS))


def fresh(qt, src, tgt, cs=None, ct=None, **kw):
    """the bits of a fresh handle put directly into a state"""
    kw.setdefault("max_outer", 2)
    with load(make_engine(GICP, **kw), GICP, src, None, tgt, None, cs, ct) as e:
        return snapshot(e, qt), cov_bytes(e)


def test_normal_form_matrices_after_general_ones_take_the_product_path_again():
    src, tgt, qt = state_pair()
    gs, gt = G.matrices("spd", "both", len(src), len(tgt))
    ns, nt = normal_form(len(src), 1), normal_form(len(tgt), 2)
    want, want_cov = fresh(qt, src, tgt, ns, nt)
    with load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None, gs, gt) as e, \
            load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None, ns, nt) as other:
        general = snapshot(e, qt)
        assert general != want
        with pytest.raises(RuntimeError):
            sicp.align_batch([e, other], np.array([qt, qt]))
        e.set_covariances(SRC, ns)
        assert snapshot(e, qt, align=False)[0] not in (general[0], want[0])        # the target's are still general
        with pytest.raises(RuntimeError):
            sicp.accumulate_batch([e, other], np.array([qt, qt]))
        e.set_covariances(TGT, nt)
        assert snapshot(e, qt) == want and cov_bytes(e) == want_cov
        res = sicp.align_batch([e, other], np.array([qt, qt]))
        for pose, st in res:
            assert (pose.tobytes(), tuple(st[k] for k in COUNTERS)) == want[1]
        e.correspondences(qt); other.correspondences(qt)
        out, _ = sicp.accumulate_batch([e, other], np.array([qt, qt]))
        assert out[0].tobytes() == want[0] and out[1].tobytes() == want[0]


def test_a_cloud_set_again_carries_the_engines_own_covariances():
    src, tgt, qt = state_pair()
    gs, gt = G.matrices("spd", "both", len(src), len(tgt))
    plain, plain_cov = fresh(qt, src, tgt)
    target_only, target_only_cov = fresh(qt, src, tgt, None, gt)
    assert plain != target_only
    with load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None, gs, gt) as e:
        both = snapshot(e, qt)
        e.set_source(src)
        assert snapshot(e, qt) == target_only and cov_bytes(e) == target_only_cov and both != target_only
        e.set_target(tgt)
        assert snapshot(e, qt) == plain and cov_bytes(e) == plain_cov
        with make_engine(GICP, max_outer=2) as other:
            load(other, GICP, src, None, tgt, None)
            res = sicp.align_batch([e, other], np.array([qt, qt]))
            assert all((p.tobytes(), tuple(s[k] for k in COUNTERS)) == plain[1] for p, s in res)


def test_gicp_without_reuse_features_recomputes_over_general_matrices():
    """reuse_features = 0: align() recomputes the covariances as the reference's does; the general matrices are gone afterwards"""
    src, tgt, qt = state_pair()
    gs, gt = G.matrices("spd", "both", len(src), len(tgt))
    with load(make_engine(GICP, max_outer=2, reuse_features=0), GICP, src, None, tgt, None) as p:
        plain = p.align(qt)
        plain_cov = cov_bytes(p)
    with load(make_engine(GICP, max_outer=2, reuse_features=0), GICP, src, None, tgt, None, gs, gt) as e, \
            load(make_engine(GICP, max_outer=2, reuse_features=0), GICP, src, None, tgt, None) as other:
        check_given_back(e, gs, gt)
        e.correspondences(qt)
        general_acc = e.accumulate(qt)
        assert same_align(e.align(qt), plain)
        assert cov_bytes(e) == plain_cov
        e.correspondences(qt); other.correspondences(qt)
        out, _ = sicp.accumulate_batch([e, other], np.array([qt, qt]))
        assert out[0].tobytes() == out[1].tobytes() == other.accumulate(qt).tobytes() != general_acc.tobytes()


def test_semantic_keeps_general_matrices_over_aligns():
    src, sl, tgt, tl, qt, _, _ = G.semantic_case("first_class_small", False)
    cs, ct = G.semantic_matrices("first_class_small", "both", False)
    with load(make_engine(SEM, max_outer=2, reuse_features=0), SEM, src, sl, tgt, tl, cs, ct) as e:
        first = e.align(qt)
        check_given_back(e, cs, ct)
        assert same_align(e.align(qt), first)
        check_given_back(e, cs, ct)
    with load(make_engine(SEM, max_outer=2, reuse_features=0), SEM, src, sl, tgt, tl) as p:
        assert not same_align(p.align(qt), first)


def test_a_shared_cloud_with_general_matrices():
    """A sets general matrices on the target that B shares: B evaluates with them, is refused by a batch, and is back on the
    product path with a fresh handle's bits once A sets matrices of the engine's form"""
    src, tgt, qt = state_pair()
    src_b = np.ascontiguousarray(G.pair20k()[0][N_STATE:2 * N_STATE])
    gt = G.family("spd", "target", len(tgt))
    nt = normal_form(len(tgt), 2)
    with make_engine(GICP, max_outer=2) as f:
        load(f, GICP, src_b, None, tgt, None, None, nt)
        want = snapshot(f, qt)
    with make_engine(GICP, max_outer=2) as a, make_engine(GICP, max_outer=2) as b, make_engine(GICP, max_outer=2) as c:
        load(a, GICP, src, None, tgt, None)
        b.set_source(src_b); b.share_cloud(TGT, a, TGT)
        load(c, GICP, src, None, tgt, None)
        b.correspondences(qt)
        before = b.accumulate(qt)
        a.set_covariances(TGT, gt)
        assert b.covariances(TGT)[0].tobytes() == gt.tobytes()
        got, ref, _ = check_accumulate(b, GICP, src_b, tgt, qt, "shared general target")
        assert A.moved_beyond(ref, before)
        with pytest.raises(RuntimeError):
            sicp.align_batch([b, c], np.array([qt, qt]))
        assert "general form" in last_error(b)
        with pytest.raises(sicp.SicpError):
            b.pose_covariance(qt)
        a.set_covariances(TGT, nt)
        assert snapshot(b, qt) == want
        res = sicp.align_batch([b, c], np.array([qt, qt]))
        assert (res[0][0].tobytes(), tuple(res[0][1][k] for k in COUNTERS)) == want[1]


@pytest.mark.parametrize("release", [False, True])
def test_a_recycled_handle_forgets_general_matrices(release):
    """sicp_destroy parks a handle whose clouds hold general matrices; the handle sicp_create hands out next, given the same
    clouds without matrices, gives the bits of the first engine's plain run -- with and without sicp_release_pool in between"""
    src, tgt, qt = state_pair()
    gs, gt = G.matrices("spd", "both", len(src), len(tgt))
    e = load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None)
    try:
        plain, plain_cov = snapshot(e, qt), cov_bytes(e)
        e.set_covariances(SRC, gs); e.set_covariances(TGT, gt)
        assert snapshot(e, qt) != plain
    finally:
        e.close()
    if release:
        assert sicp.lib().sicp_release_pool(0) == sicp.OK
    with make_engine(GICP, max_outer=2) as e2:
        load(e2, GICP, src, None, tgt, None)
        assert snapshot(e2, qt) == plain and cov_bytes(e2) == plain_cov
        with make_engine(GICP, max_outer=2) as e3:
            load(e3, GICP, src, None, tgt, None)
            sicp.align_batch([e2, e3], np.array([qt, qt]))
            e2.pose_covariance(qt)


def test_tolerances_of_the_classifier():
    src, tgt, qt = state_pair()
    n = len(src)
    gs = np.array(G.family("spd", "source", n))
    with load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None) as e, load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None) as other:
        # an asymmetry below the tolerance: accepted, handed back as the mean of the two entries
        c = gs.copy(); c[7, 0, 1] += 0.5 * G.SYMMETRY_TOL
        e.set_covariances(SRC, c)
        back = e.covariances(SRC)[0]
        want = c.copy(); want[7, 0, 1] = want[7, 1, 0] = 0.5 * (c[7, 0, 1] + c[7, 1, 0])
        assert c[7, 0, 1] != c[7, 1, 0] and back.tobytes() == want.tobytes()
        held = cov_bytes(e)
        # ten times the tolerance: refused, the point named, nothing changed
        c = gs.copy(); c[1234, 1, 2] += 10 * G.SYMMETRY_TOL * (1 + abs(c[1234, 1, 2]))
        with pytest.raises(sicp.SicpError) as err:
            e.set_covariances(SRC, c)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "point 1234 " in str(err.value) and cov_bytes(e) == held
        # 1e-10 off the engine's form, every row: of that form; re-formed within 1e-8; a batch takes the handle
        ns = normal_form(n, 1)
        noise = G.symmetrise(np.random.default_rng(5).uniform(-1e-10, 1e-10, size=(n, 3, 3)))
        e.set_covariances(SRC, ns + noise)
        back, nrm, _, _ = e.covariances(SRC)
        assert np.isfinite(nrm).all() and np.abs(back - ns).max() < G.FORM_TOL and np.allclose(np.linalg.norm(nrm, axis=1), 1.0, rtol=0, atol=1e-12)
        sicp.align_batch([e, other], np.array([qt, qt]))
        # one row 1e-6 off: the whole cloud is general, every row comes back with the bytes given
        c = ns.copy(); c[99, 0, 0] += 1e-6; c[99, 0, 1] += 1e-6; c[99, 1, 0] += 1e-6
        e.set_covariances(SRC, c)
        back, nrm, _, _ = e.covariances(SRC)
        assert back.tobytes() == c.tobytes() and np.isnan(nrm).all()
        with pytest.raises(RuntimeError):
            sicp.align_batch([e, other], np.array([qt, qt]))


@pytest.mark.parametrize("holding", ["general", "own"])
def test_refusals_change_nothing(holding):
    src, tgt, qt = state_pair()
    n = len(src)
    gs, gt = G.matrices("spd", "both", n, len(tgt))
    lib = sicp.lib()
    with load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None, *((gs, gt) if holding == "general" else (None, None))) as e:
        e.correspondences(qt)
        held, acc = cov_bytes(e), e.accumulate(qt).tobytes()

        def unchanged(what):
            assert cov_bytes(e) == held, what
            assert e.accumulate(qt).tobytes() == acc, what       # (the correspondences are still valid too)

        for which, base in ((SRC, gs), (TGT, gt)):
            c = np.array(base); c[321, 0, 2] += 1e-3
            with pytest.raises(sicp.SicpError) as err:
                e.set_covariances(which, c)
            assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "point 321 " in str(err.value) and "nothing was changed" in str(err.value)
            unchanged("non-symmetric row")
            for bad in (np.nan, np.inf):
                c = np.array(base); c[2, 1, 1] = bad
                with pytest.raises(sicp.SicpError) as err:
                    e.set_covariances(which, c)
                assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "point 2 " in str(err.value)
                unchanged("non-finite row at a finite point")
            assert lib.sicp_set_covariances(e._h, which, None) == sicp.ERR_INVALID_ARGUMENT
            unchanged("NULL")
        flat = np.ascontiguousarray(np.array(gs).reshape(-1, 9))
        for which in (-1, 2, 7):
            assert lib.sicp_set_covariances(e._h, which, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == sicp.ERR_INVALID_ARGUMENT
            unchanged("bad which")


def test_em_refuses_general_matrices_and_keeps_its_features():
    src, sl, tgt, tl, qt = G.mid_pair(N_STATE)
    gs = G.family("spd", "source", len(src))
    p = A.set_params(sicp.default_params(sicp.MODE_EM), sicp.MODE_EM, max_outer=2)
    with sicp.Engine(0, p) as e:
        e.set_confusion(synth.confusion_matrix(A.C))
        e.set_source(src, sl); e.set_target(tgt, tl)
        e.correspondences(qt)
        held, acc = cov_bytes(e), e.accumulate(qt).tobytes()
        c = np.array(e.covariances(SRC)[0]); c[1:40] = gs[1:40]        # rows 1 .. 39 are general, the rest the engine's own
        with pytest.raises(sicp.SicpError) as err:
            e.set_covariances(SRC, c)
        msg = str(err.value)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "SICP_MODE_GICP" in msg and "nothing was changed" in msg and "point " in msg
        named = int(msg.split("point ")[1].split()[0])
        assert 1 <= named < 40                                          # a general row (the device order decides which is met first)
        assert cov_bytes(e) == held and e.accumulate(qt).tobytes() == acc


def same_dict(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in a)


def test_multi_pair_entry_points_answer_with_a_status():
    src, tgt, qt = state_pair()
    gs, gt = G.matrices("spd", "both", len(src), len(tgt))
    src2 = np.ascontiguousarray(G.pair20k()[0][N_STATE:2 * N_STATE])
    with load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None, gs, None) as e, \
            load(make_engine(GICP, max_outer=2), GICP, src, None, tgt, None) as p1, \
            load(make_engine(GICP, max_outer=2), GICP, src2, None, tgt, None) as p2:
        e.correspondences(qt)
        held, acc = cov_bytes(e), e.accumulate(qt).tobytes()
        lone = [p.pose_covariance(qt) for p in (p1, p2)]
        assert not same_dict(*lone)
        with pytest.raises(RuntimeError):
            sicp.align_batch([p1, e], np.array([qt, qt]))
        assert "general form" in last_error(e) and "sicp_align" in last_error(e)
        p1.correspondences(qt)
        with pytest.raises(RuntimeError):
            sicp.accumulate_batch([p1, e], np.array([qt, qt]))
        assert "general form" in last_error(e) and "sicp_accumulate" in last_error(e)
        with pytest.raises(sicp.SicpError) as err:
            e.pose_covariance(qt)
        assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "general form" in str(err.value)
        res = sicp.pose_covariance_batch([p1, e, p2], np.array([qt, qt, qt]))
        assert [s for s, _ in res] == [sicp.OK, sicp.ERR_INVALID_ARGUMENT, sicp.OK] and "general form" in last_error(e)
        assert same_dict(res[0][1], lone[0]) and same_dict(res[2][1], lone[1])
        assert cov_bytes(e) == held and e.accumulate(qt).tobytes() == acc
        # sicp_evaluate works on such a handle, and leaves it as it was
        ev = e.evaluate(qt, 1.0)
        assert same_dict(ev, p1.evaluate(qt, 1.0)) and ev["inliers"] > 0.5 * len(src)
        assert cov_bytes(e) == held and e.accumulate(qt).tobytes() == acc
        # a lone align of the general handle still runs, and a batch of one is a lone align
        pose, st = e.align(qt)
        res = sicp.align_batch([e], np.array([qt]))
        assert res[0][0].tobytes() == pose.tobytes() and all(res[0][1][k] == st[k] for k in COUNTERS)
