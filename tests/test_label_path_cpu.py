"""CPU tests of the label path's restatement (tests/label_path_ref.py) and of the cases the GPU tests use
(tests/label_path_cases.py): the restatement equals the oracle -- counts and weights bit for bit, fused labels exactly -- on
both sides of the 16-class border; its float64 sums are within 1e-13 of the same sums in longdouble at every class count, which
is what makes the GPU module's rtol 1e-12 a statement about the kernels; and the conditions that module relies on -- which
branch of the gate every slot of the planes takes, no slot at the edge of the smallest double, how many fused-label points
are too close to call, what the tight gate leaves alive -- hold for the reference alone."""
import numpy as np
import pytest

import label_path_cases as cases
import label_path_ref as L
import oracle_lib as O

K = cases.K_COV


def test_the_count_table_is_the_repeated_sum():
    for k in (1, 5, 20, 32):
        acc, want = 0.0, []
        for _ in range(k + 1):
            want.append(acc)
            acc += 1.0 / k
        assert L.hval(k).tolist() == want
    assert L.hval(20)[20] != 1.0 and L.hval(5)[5] == 1.0  # (twenty increments of 1/20 do not add up to 1: the order matters)


@pytest.mark.parametrize("C", [4, 16, 17])
def test_restatement_equals_the_oracle(C):
    src, sl, tgt, tl, qt = cases.labelled_pair(C)
    cm = cases.matrix(C)
    (scov, sc, snn, sh), (tcov, tc, tnn, th) = cases.oracle_features(C)
    # counts: from the oracle's own neighbour lists, and the oracle's doubles are the table's entries
    assert np.array_equal(L.hist_counts(sl, snn, C), sc) and np.array_equal(L.hist_counts(tl, tnn, C), tc)
    assert np.array_equal(L.hval(K)[sc], sh) and np.array_equal(L.hval(K)[tc], th)
    assert (sc.sum(axis=1) == K).all() and sc.max() > K // 2
    # weights, slot by slot on a 300-point subset: BIT FOR BIT as the reference computes them (bool gate); with the gate as a
    # double numpy's pow / exp stand against libm's, so rtol 1e-14 there (and only on normal numbers)
    idx, _ = cases.oracle_slots(C)
    rows = np.random.default_rng(C).choice(len(src), 300, replace=False)
    w_bool = L.weights(sc, tc, cm, K, qt, src, scov, tgt, tcov, idx)
    w_dbl = L.weights(sc, tc, cm, K, qt, src, scov, tgt, tcov, idx, as_bool=False)
    want_bool, want_dbl = np.zeros((300, 4)), np.zeros((300, 4))
    for a, i in enumerate(rows):
        for c in range(4):
            j = idx[i, c]
            if j < 0:
                continue
            b, v = O.gicp_probability(qt, src[i].astype(np.float64), tgt[j].astype(np.float64), scov[i], tcov[j])
            prob = O.em_prob(cm, th[j], sh[i])
            want_bool[a, c], want_dbl[a, c] = prob * float(b), prob * v
    assert (idx[rows] >= 0).sum() > 1000
    assert np.array_equal(w_bool[rows], want_bool)
    normal = want_dbl > 1e-290
    assert normal.sum() > 1000 and np.allclose(w_dbl[rows][normal], want_dbl[normal], rtol=1e-14, atol=0)
    assert (w_dbl[rows][~normal] <= 1e-290).all()
    # fused labels, at both gates
    for gate_sq in (cases.GATE_WIDE, cases.GATE_TIGHT):
        scores, want = cases.fused_reference(C, gate_sq)
        assert len(want) == len(src) - 20 and np.array_equal(L.fused_labels(scores), want)
        assert len(np.unique(want)) >= min(C, 8)


def test_every_class_reaches_both_clouds():
    for C in cases.HIST_CLASSES + (4, 11):
        _, sl, _, tl, _ = cases.labelled_pair(C)
        assert np.array_equal(np.unique(sl), np.arange(1, C + 1)) and np.array_equal(np.unique(tl), np.arange(1, C + 1)), C


@pytest.mark.parametrize("C", sorted(set(cases.HIST_CLASSES + (11,))))
def test_float64_sums_are_within_1e13_of_longdouble(C):
    """projections and label factor in longdouble against the float64 restatement: the restatement's own rounding error"""
    assert np.finfo(np.longdouble).eps < 1e-3 * np.finfo(np.float64).eps  # (x86-64's 80-bit format: 11 more bits)
    cm = cases.matrix(C)
    (_, sc, _, _), (_, tc, _, _) = cases.oracle_features(C)
    idx, _ = cases.oracle_slots(C)
    sc, idx = sc[::4], idx[::4]                      # every fourth source point and the targets its slots name
    used, slot = np.unique(idx, return_inverse=True)
    tc, slot = tc[used], slot.reshape(idx.shape)
    assert (used >= 0).all() and len(used) > 1000
    f64 = L.label_factor(L.projections(sc, cm, K), L.projections(tc, cm, K), slot)
    ext = L.label_factor(L.projections(sc, cm, K, np.longdouble), L.projections(tc, cm, K, np.longdouble), slot)
    assert ext.dtype == np.longdouble and (ext > 0).all()
    err = float(np.max(np.abs(f64.astype(np.longdouble) - ext) / ext))
    print(f"C {C}: largest relative error of the float64 label factor {err:.3g}")
    assert err < 1e-13


def test_gate_planes_put_every_slot_where_the_gpu_tests_expect_it():
    src, sl, tgt, tl, poses = cases.gate_planes()
    assert src.dtype == tgt.dtype == np.float32 and (src[:, 2] == 0).all() and (tgt[:, 2] == 0).all() and len(src) == len(tgt) == 2304
    scov, snrm, _ = O.covariances(src, sl, K, cases.EPS, 4, kdtree=True)
    tcov, tnrm, _ = O.covariances(tgt, tl, K, cases.EPS, 4, kdtree=True)
    for nrm, cov in ((snrm, scov), (tnrm, tcov)):
        assert np.array_equal(np.abs(nrm), np.tile([0.0, 0.0, 1.0], (2304, 1)))
        assert np.abs(cov - np.diag([1.0, 1.0, cases.EPS])).max() < 1e-15
    totals = dict(below=0, band_one=0, band_zero=0, above=0)
    for r0, qt in poses:
        q = O.transform_points(O.se3_matrix(qt), src)
        idx, d2 = O.knn(q, tgt, 4, kdtree=True)
        assert d2.max() <= 3.63  # inside the default distance gate of 250: every slot is live
        g, r, logp = L.gate(qt, src, scov, tgt, tcov, idx)
        assert np.abs(r - r0).max() < 0.013
        assert (g == (1.0 if r0 <= cases.GATE_LAST_ONE else 0.0)).all()
        assert not L.near_edge(logp).any()
        for k, v in cases.regime_totals(r, g).items():
            totals[k] += v
    print("slots per regime:", totals)
    assert totals == cases.GATE_TOTALS


@pytest.mark.parametrize("C", cases.FUSED_CLASSES)
def test_fused_label_cases_are_decidable_and_the_tight_gate_bites(C):
    n = int(cases.fused_pair(C)[5].sum())
    assert n == 2980
    for gate_sq in (cases.GATE_WIDE, cases.GATE_TIGHT):
        idx, _ = cases.oracle_slots(C, gate_sq, fused=True)
        live = (idx >= 0).sum(axis=1)
        scores, want = cases.fused_reference(C, gate_sq)
        assert np.array_equal(L.fused_labels(scores), want)
        _, _, gap = L.top_two(scores)
        close = float((gap < 1e-9).mean())
        print(f"C {C} gate_sq {gate_sq}: slots dropped {1 - (idx >= 0).mean():.3f}, points with 0 / 1-3 / 4 live slots "
              f"{(live == 0).sum()} / {((live > 0) & (live < 4)).sum()} / {(live == 4).sum()}, top-two gap below 1e-9: {100 * close:.2f} %")
        assert close <= 0.01
        if gate_sq == cases.GATE_TIGHT:
            assert 0.2 <= 1 - (idx >= 0).mean() <= 0.8
            assert min((live == 0).sum(), ((live > 0) & (live < 4)).sum(), (live == 4).sum()) > n // 10
            assert (want[live == 0] == 1).all()
        else:
            assert (idx >= 0).all()
