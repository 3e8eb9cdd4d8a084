"""CPU tests of what tests/test_gpu_general_covariances.py stands on (tests/general_cov_cases.py): the matrix families, the
general kernel's chunk split restated, and -- on the oracle alone, with its own exact neighbours and its own I - (1 - eps) n n^T
where a cloud keeps the engine's form -- that every case's reference is finite, that the float64 oracle is so close to its
np.longdouble restatement that the bar widened by 4 x that distance is the project bar (at most a tenth of it), that the
oracle notices one slot dying at every edge of the split, that the Semantic shuffles move rows across label segments, that the
far start makes the solve reject steps, and how far the kernel's closed form is from the longdouble sums in float64."""
import numpy as np
import pytest

import accumulate_cases as A
import general_cov_cases as G
import oracle_lib as O


@pytest.fixture(scope="module")
def mid():
    """the mid-size pair with the oracle's engine-form covariances"""
    src, sl, tgt, tl, qt = G.mid_pair()
    return src, tgt, qt, G.oracle_engine_form(src), G.oracle_engine_form(tgt)


@pytest.fixture(scope="module")
def big():
    """the 20 000-point source (prefixes: the split sizes) with its 20 exact neighbours at the true pose"""
    src, sl, tgt, tl, qt = G.pair20k()
    idx20 = G.oracle_slots(src[:16385], tgt, qt, 20, gate=G.GATE_OPEN)
    idx20.setflags(write=False)
    return src, tgt, qt, idx20


def both(cs, ct, es, et):
    return (es if cs is None else cs), (et if ct is None else ct)


def check_reference(what, p, qt, src, cs, tgt, ct, idx):
    """reference finite; 4 x its distance to the longdouble restatement at most WIDENING_CAP x the project bar"""
    ref = O.accumulate(p, qt, src, cs, tgt, ct, idx, None)
    assert np.isfinite(ref).all(), what
    w = G.widening(ref, G.oracle_distance(p, qt, src, cs, tgt, ct, idx, None, ref))
    print(f"{what}: 4 x oracle distance / project bar  H {w[0]:.2e}  g {w[1]:.2e}  cost {w[2]:.2e}")
    assert max(w) <= G.WIDENING_CAP, (what, w)
    return ref


# ---- families and the split ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.FAMILIES))
def test_matrix_families(name):
    lo, hi = G.FAMILIES[name]
    for side in ("source", "target"):
        C = G.family(name, side, 3000)
        assert not C.flags.writeable and np.array_equal(C, C.transpose(0, 2, 1))
        ev = np.linalg.eigvalsh(C)
        tol = 1e-12 * hi
        if name == "indef" and side == "source":
            assert (np.abs(ev) >= lo - tol).all() and (np.abs(ev) <= hi + tol).all()
            assert (ev < 0).any(axis=1).mean() > 0.8 and ((ev < 0).any(axis=1) & (ev > 0).any(axis=1)).mean() > 0.7
        else:
            l, h = G.FAMILIES["spd"] if name == "indef" else (lo, hi)
            assert (ev >= l - max(tol, 1e-15)).all() and (ev <= h + tol).all()
        if name == "wide":
            assert ev.min() < 1e-3 and ev.max() > 9.0
        assert len({c.tobytes() for c in C}) == len(C)                     # per point distinct: a wrong row shows
        # not of the engine's form by far: (I - C) / (1 - eps) is no rank-one projector
        assert np.abs(np.linalg.eigvalsh(np.eye(3) - C)[:, 1]).min() > 100 * G.FORM_TOL
    assert not np.array_equal(G.family(name, "source", 100), G.family(name, "target", 100))
    assert np.array_equal(G.family(name, "source", 100), G.family(name, "source", 100))


def test_the_split_covers_every_slot_once():
    seen_ragged = seen_chunks = 0
    for K, n_s in G.SPLIT_CASES + [(k, 3000) for k in (1, 4, 20)]:
        total = n_s * K
        ranges = G.general_split(n_s, K)
        assert len(ranges) == G.general_chunks(n_s, K) == A.acc_geometry(total, A.slots_per_group(K))["n_chunks"]
        count = np.zeros(total, dtype=int)
        for s0, s1 in ranges:
            count[s0:s1] += 1
        assert (count == 1).all(), (K, n_s)
        per = ranges[0][1] - ranges[0][0]
        seen_chunks += len(ranges) > 1
        seen_ragged += len(ranges) > 1 and per % 256 != 0
        # a floor instead of the ceiling would lose a tail exactly where total is no multiple of the chunk count
        if len(ranges) > 1 and total % len(ranges):
            assert (total // len(ranges)) * len(ranges) < total
    assert seen_chunks >= 6 and seen_ragged >= 5
    for K, sizes in G.SPLIT_SIZES.items():     # one slot, and both sides of the first chunk boundary, at every K
        assert 1 in sizes and {1, 2} <= {G.general_chunks(n, K) for n in sizes}
        assert any(G.general_chunks(n, K) > 1 and (n * K) % G.general_chunks(n, K) for n in sizes), K
    assert {255, 256, 257} <= set(G.SPLIT_SIZES[1])   # either side of one lane stride


# ---- 1. every instantiation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn,sq,which,fam", G.INSTANTIATIONS, ids=[G.inst_id(*c) for c in G.INSTANTIATIONS])
def test_every_instantiation_has_a_sound_reference(mid, knn, sq, which, fam):
    src, tgt, qt, es, et = mid
    cs, ct = both(*G.matrices(fam, which, len(src), len(tgt)), es, et)
    p = G.oracle_params(O.MODE_GICP, knn=knn, use_sqloss=sq)
    for k, pose in enumerate((qt, A.poses_around(qt, 3, seed=5)[1])):
        idx = G.oracle_slots(src, tgt, pose, knn)
        assert (idx >= 0).mean() > 0.9
        ref = check_reference(f"{G.inst_id(knn, sq, which, fam)} pose {k}", p, pose, src, cs, tgt, ct, idx)
        assert (np.abs(ref[21:27]) > 0).all() and ref[27] > 0


@pytest.mark.parametrize("knn,sq,which,fam,kw", G.LOSS_CASES, ids=[G.inst_id(*c[:4], *c[4].items()) for c in G.LOSS_CASES])
def test_loss_and_epsilon_cases_have_a_sound_reference(knn, sq, which, fam, kw):
    src, sl, tgt, tl, qt = G.mid_pair()
    eps = kw.get("epsilon", 1e-3)
    es, et = G.oracle_engine_form(src, eps=eps), G.oracle_engine_form(tgt, eps=eps)
    cs, ct = both(*G.matrices(fam, which, len(src), len(tgt)), es, et)
    p = G.oracle_params(O.MODE_GICP, knn=knn, use_sqloss=sq, **kw)
    idx = G.oracle_slots(src, tgt, qt, knn)
    ref = check_reference(G.inst_id(knn, sq, which, fam, kw), p, qt, src, cs, tgt, ct, idx)
    base = O.accumulate(G.oracle_params(O.MODE_GICP, knn=knn, use_sqloss=sq), qt, src, cs, tgt, ct, idx, None)
    if "cauchy_a" in kw:
        assert A.moved_beyond(base, ref)
    else:   # epsilon moves the engine's side only
        e3 = G.oracle_engine_form(tgt)
        assert A.moved_beyond(O.accumulate(p, qt, src, cs, tgt, e3, idx, None), ref)


# ---- 2. the split ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,n_s", G.SPLIT_CASES, ids=[f"k{K}-{n}" for K, n in G.SPLIT_CASES])
def test_one_slot_dying_at_each_edge_of_the_split_moves_the_reference(big, K, n_s):
    src, tgt, qt, idx20 = big
    src, idx = src[:n_s], np.ascontiguousarray(idx20[:n_s, :K])
    cs, ct = G.matrices("spd", "both", n_s, len(tgt))
    p = G.oracle_params(O.MODE_GICP, knn=K, gate_sq=G.GATE_OPEN)
    ref = check_reference(f"k{K}-{n_s}", p, qt, src, cs, tgt, ct, idx)
    gone = G.split_removals(idx)
    assert len(gone) == G.general_chunks(n_s, K) + 1
    for what, less in gone.items():
        assert (less < 0).sum() == 1 and (less != idx).sum() == 1, what
        other = O.accumulate(p, qt, src, cs, tgt, ct, less, None)
        assert A.moved_beyond(ref, other), (what, np.abs(other - ref) / A.project_bars(ref))


def test_dead_slot_cases_have_a_sound_reference(mid):
    src, tgt, qt, es, et = mid
    cs, ct = G.matrices("spd", "both", len(src), len(tgt))
    for K in (1, 4):
        p = G.oracle_params(O.MODE_GICP, knn=K)
        far = G.far_pose(qt, G.HALF_GATE_SHIFT)
        idx = G.oracle_slots(src, tgt, far, K)
        assert 0.3 <= (idx < 0).mean() <= 0.7
        check_reference(f"half dead, K = {K}", p, far, src, cs, tgt, ct, idx)
        # non-finite rows: the reference on the finite points
        ps, cps, bad_s = G.with_non_finite_rows(src, cs, seed=3)
        pt, cpt, bad_t = G.with_non_finite_rows(tgt, ct, seed=4)
        assert 0.025 < bad_s.mean() < 0.035 and 0.025 < bad_t.mean() < 0.035
        assert np.isnan(cps[bad_s]).all() and np.isfinite(cps[~bad_s]).all() and not np.isfinite(ps[bad_s]).all(axis=1).any()
        fs, fcs = G.finite_for_oracle(ps, cps, bad_s)
        ft, fct = G.finite_for_oracle(pt, cpt, bad_t)
        keep_t = np.nonzero(~bad_t)[0]
        i = G.oracle_slots(fs, np.ascontiguousarray(ft[keep_t]), qt, K)
        idx = np.where(i >= 0, keep_t[np.maximum(i, 0)], -1).astype(np.int32)
        idx[bad_s] = -1
        check_reference(f"non-finite rows, K = {K}", p, qt, fs, fcs, ft, fct, idx)
    none = np.full((len(src), 4), -1, dtype=np.int32)
    assert (O.accumulate(G.oracle_params(O.MODE_GICP, knn=4), qt, src, cs, tgt, ct, none, None) == 0).all()


# ---- 3. Semantic ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.SEMANTIC_FIXTURES))
def test_semantic_shuffles_move_rows_across_label_segments(name):
    src, sl, tgt, tl, qt, ps, pt = G.semantic_case(name, True)
    src0, sl0, tgt0, tl0, qt0, i_s, i_t = G.semantic_case(name, False)
    assert np.array_equal(i_s, np.arange(len(src0))) and np.array_equal(src, src0[ps]) and np.array_equal(tl, tl0[pt])
    for lab, lab0, perm in ((sl, sl0, ps), (tl, tl0, pt)):
        assert sorted(perm.tolist()) == list(range(len(perm)))
        assert (lab != lab0).mean() > 0.4                          # a row now sits where another class sat
        # the device order groups by label: the shuffled caller order is far from any grouped order
        runs = 1 + int((lab[1:] != lab[:-1]).sum())
        assert runs > 0.4 * len(lab) and runs > 50 * len(np.unique(lab))
    for which in G.WHICH:
        cs, ct = G.semantic_matrices(name, which, True)
        cs0, ct0 = G.semantic_matrices(name, which, False)
        if cs is not None:
            assert np.array_equal(cs, cs0[ps]) and not np.array_equal(cs, cs0)
        if ct is not None:
            assert np.array_equal(ct, ct0[pt]) and not np.array_equal(ct, ct0)


@pytest.mark.parametrize("which", G.WHICH)
@pytest.mark.parametrize("name", list(G.SEMANTIC_FIXTURES))
def test_semantic_cases_have_a_sound_reference(name, which):
    refs = []
    for shuffled in (False, True):
        src, sl, tgt, tl, qt, ps, pt = G.semantic_case(name, shuffled)
        es, et = G.oracle_engine_form(src, sl), G.oracle_engine_form(tgt, tl)
        cs, ct = both(*G.semantic_matrices(name, which, shuffled), es, et)
        p = G.oracle_params(O.MODE_SEMANTIC)
        idx = G.oracle_slots(src, tgt, qt, 1, sl=sl, tl=tl, min_class_pts=p.min_class_pts)
        assert 0.5 < (idx >= 0).mean() < 1.0                        # skipped classes leave dead slots
        refs.append(check_reference(f"semantic {name}, {which}, shuffled {shuffled}", p, qt, src, cs, tgt, ct, idx))
    assert A.excess(refs[1], refs[0], A.project_bars(refs[0]))[0] <= 1.0


# ---- 4. solve -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knn,sq,which", G.SOLVE_CASES, ids=[G.inst_id(k, s, w, "spd") for k, s, w in G.SOLVE_CASES])
def test_the_far_start_makes_the_oracle_reject_steps(mid, knn, sq, which):
    src, tgt, qt, es, et = mid
    cs, ct = both(*G.matrices("spd", which, len(src), len(tgt)), es, et)
    p = G.oracle_params(O.MODE_GICP, knn=knn, use_sqloss=sq)
    start = G.far_start(qt)
    idx = G.oracle_slots(src, tgt, start, knn)
    ex = G.expectation(p, src, cs, tgt, ct, idx, None, start)
    print(f"{G.inst_id(knn, sq, which, 'spd')}: status {ex['status']} {ex['seq']}")
    assert ex["status"] == 0 and "r" in ex["seq"][:-1] and "a" in ex["seq"] and not ex["unchanged"]


def test_the_singular_system_ends_the_oracle_at_its_start():
    """one live pair, both matrices all zero: A = 0, the sums are not finite, the oracle's solve fails at its first evaluation"""
    src, sl, tgt, tl, qt = G.mid_pair(1)
    tgt = tgt[:1]
    z = np.zeros((1, 3, 3))
    p = G.oracle_params(O.MODE_GICP, knn=1, gate_sq=G.GATE_OPEN)
    idx = np.zeros((1, 1), dtype=np.int32)
    with np.errstate(all="ignore"):
        ref = O.accumulate(p, qt, src, z, tgt, z, idx, None)
    assert not np.isfinite(ref).all()
    ex = G.expectation(p, src, z, tgt, z, idx, None, qt)
    assert ex["status"] == 3 and ex["lm_iters"] == 0 and ex["evals"] == 1 and ex["unchanged"]


# ---- the kernel's closed form in float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(G.FAMILIES))
def test_closed_form_in_float64_against_the_longdouble_sums(mid, fam):
    """a = A^-1 res by cofactors, b = R^T a, c = p_s + C_s b, J = [-2b; 2 b x c] in numpy float64: equal to the oracle's literal
    Evaluate for symmetric matrices, and as close to the longdouble sums as the oracle is (figures: profiles/general_covariances)"""
    src, tgt, qt, es, et = mid
    cs, ct = G.matrices(fam, "both", len(src), len(tgt))
    pose = G.far_pose(qt, (0.05, -0.03, 0.02))
    for knn in (1, 4, 20):
        for sq in (0, 1):
            p = G.oracle_params(O.MODE_GICP, knn=knn, use_sqloss=sq)
            idx = G.oracle_slots(src, tgt, pose, knn)
            ref = O.accumulate(p, pose, src, cs, tgt, ct, idx, None)
            ld = G.accumulate_longdouble(p, pose, src, cs, tgt, ct, idx, None)
            cf = G.closed_form_float64(p, pose, src, cs, tgt, ct, idx)
            w = G.widening(ref, np.abs(cf.astype(np.longdouble) - ld).astype(np.float64))
            print(f"{fam} k{knn} sqloss {sq}: 4 x closed-form distance / project bar  H {w[0]:.2e}  g {w[1]:.2e}  cost {w[2]:.2e}")
            assert max(w) <= G.WIDENING_CAP, (fam, knn, sq, w)
            assert A.excess(cf, ref, A.project_bars(ref))[0] <= 1.0
