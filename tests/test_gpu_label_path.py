"""GPU tests of EM-ICP's label path -- cov_body's label counts, proj_body / proj_rows_body, em_weight_rows_body<4> /
em_weight_body / the search's weight epilogue, geometric_gate, fused_label_kernel, in job launches of one and of many -- against
tests/label_path_ref.py on both sides of every branch on the class count C and on the slots per point K:
  counts        exactly, on the engine's own neighbour lists (which equal the oracle's), C on both sides of the register
                borders (8 | 9, 16 | 17) and up to 255, 32 neighbours in one byte, non-finite points left out;
  weights       at rtol 1e-12 (atol 0) on every kernel that computes them, from the engine's reported covariances and counts:
                the restatement's own float64 error is below 1e-13 (tests/test_label_path_cpu.py), the kernels' sums are the
                same operations in the same order; as a double (quirk Q1 off) at rtol 1e-11, atol 1e-300, device pow / exp
                against numpy's;
  gate          on two planes whose slots all sit at a chosen r on either side of 1300 and 1600 and of the point where the
                literal formula turns 0: w > 0 exactly where the reference's Probability() is true;
  fused labels  exactly as the oracle's, with the distance gate wide and tight (points with 0, 1-3 and 4 live slots); with the
                gate as a double, exactly as the restatement's scores say;
  batches       align_batch of five pairs of ragged sizes at C = 17 equals the lone aligns bit for bit; so do batches of
                handles with Probability() as a double (3 and 5 pairs, C on both sides of 16) and batches that mix them with
                bool handles -- job launches of many of the kernels that hold both forms of the gate.
Every case prints its figures (run with -s); profiles/label_path/figures.txt holds them."""
import importlib

import numpy as np
import pytest

import label_path_cases as cases
import label_path_ref as L
import oracle_lib as O

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
SRC, TGT = sicp.SOURCE, sicp.TARGET
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
K = cases.K_COV
PROFILE_WEIGHT = 4   # SICP_PROFILE_WEIGHT: a handle with it runs the weight kernel behind the search, not the search's epilogue


def _engine(C, cm=True, **kw):
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = C
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    if cm:
        e.set_confusion(cases.matrix(C))
    return e


def _rel(got, want):
    """largest relative error over entries where the reference is not 0 (0 for none)"""
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]), initial=0.0))


# ---- 1. histograms ----------------------------------------------------------------------------------------------------------
HIST_CASES = [(C, K) for C in cases.HIST_CLASSES] + [(16, 5), (16, 32), (17, 5), (17, 32), (1, 32)]


@pytest.mark.parametrize("C,k_cov", HIST_CASES)
def test_label_counts_equal_the_restatement(C, k_cov):
    src, sl, _, _, _ = cases.labelled_pair(C)
    with _engine(C, cm=False, k_cov=k_cov) as e:
        e.set_source(src, sl)
        _, _, hist, nn = e.covariances(SRC, want_hist=True, want_nn=True)
    want_nn, _ = O.knn(src, src, k_cov, kdtree=True)
    want = L.hist_counts(sl, nn, C)
    print(f"C {C} k_cov {k_cov}: rows differing {int((hist != want).any(axis=1).sum())}, neighbour rows differing "
          f"{int((nn != want_nn).any(axis=1).sum())}, largest count {int(hist.max())}, classes seen {int((hist.sum(axis=0) > 0).sum())}")
    assert nn.dtype == np.int32 and np.array_equal(nn, want_nn)
    assert hist.dtype == np.uint8 and hist.shape == (len(src), C) and np.array_equal(hist, want)
    assert (hist.sum(axis=1, dtype=np.int64) == k_cov).all() and (hist.sum(axis=0, dtype=np.int64) > 0).all()
    if C == 1:
        assert (hist == k_cov).all()   # (k_cov = 32: the largest count a byte has to hold)


@pytest.mark.parametrize("C", [9, 17])
def test_label_counts_with_non_finite_points_left_out(C):
    src, sl, _, _, _ = cases.labelled_pair(C)
    bad, fin = cases.with_bad_points(src, 50, C)
    with _engine(C, cm=False) as e:
        e.set_source(bad, sl)
        assert e.cloud_size(SRC) == (len(src), len(src) - 50)
        cov, nrm, hist, nn = e.covariances(SRC, want_hist=True, want_nn=True)
    keep = np.flatnonzero(fin)
    want_nn, _ = O.knn(bad[fin], bad[fin], K, kdtree=True)
    assert np.array_equal(nn[fin], keep[want_nn])                    # caller indices, none of a dropped point
    assert np.array_equal(hist, L.hist_counts(sl, nn, C)) and (hist[fin].sum(axis=1) == K).all()
    # a point outside the index has no neighbourhood: no list, no counts, no normal
    assert (nn[~fin] == -1).all() and (hist[~fin] == 0).all() and np.isnan(cov[~fin]).all() and np.isnan(nrm[~fin]).all()
    assert np.isfinite(cov[fin]).all()


# ---- 2. weights ---------------------------------------------------------------------------------------------------------------
def _weights_of_every_path(C, knn, bool_q, src, sl, tgt, tl, qt):
    """[(path, idx, w, restatement's w, the engine's source and target covariances)]: the search's epilogue and the weight kernel behind the search where the engine has both
    (K = 4, at most 16 classes), the weight kernel alone elsewhere -- the counters say which one ran"""
    out = []
    both = C <= 16 and knn == 4
    for profile in ((0, PROFILE_WEIGHT) if both else (0,)):
        with _engine(C, knn=knn, quirk_bool_probability=bool_q, profile=profile) as e:
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            st0 = e.stats()
            idx, d2, w = e.correspondences(qt)
            st1 = e.stats()
            in_search = st1["weights_in_search"] - st0["weights_in_search"]
            launches = st1["weight_launches"] - st0["weight_launches"]
            epilogue = both and profile == 0
            assert (in_search, launches) == ((1, 0) if epilogue else (0, 1))
            scov, _, sh, _ = e.covariances(SRC, want_hist=True)
            tcov, _, th, _ = e.covariances(TGT, want_hist=True)
        want = L.weights(sh, th, cases.matrix(C), K, qt, src, scov, tgt, tcov, idx, as_bool=bool(bool_q))
        out.append(("epilogue" if epilogue else "kernel", idx, w, want, scov, tcov))
    return out


WEIGHT_CASES = [(C, 4) for C in cases.HIST_CLASSES] + [(11, 1), (11, 20), (17, 1), (17, 20)]


@pytest.mark.parametrize("C,knn", WEIGHT_CASES)
def test_weights_equal_the_restatement(C, knn):
    src, sl, tgt, tl, qt = cases.labelled_pair(C)
    want_idx, _ = cases.oracle_slots(C, cases.GATE_WIDE, knn)
    for path, idx, w, want, _, _ in _weights_of_every_path(C, knn, 1, src, sl, tgt, tl, qt):
        live = idx >= 0
        print(f"C {C} K {knn} {path}: live slots {int(live.sum())} of {live.size}, with weight 0: {int((want[live] == 0).sum())}, "
              f"largest relative error {_rel(w, want):.3g}, differing in any bit {int((w != want).sum())}")
        assert np.array_equal(idx, want_idx) and live.mean() > 0.9
        assert (w[~live] == 0).all()
        assert np.allclose(w, want, rtol=1e-12, atol=0)
        assert np.array_equal(w == 0, want == 0) and (want[live] > 0).mean() > 0.9


@pytest.mark.parametrize("C", [9, 16, 17])
def test_weights_with_the_probability_as_a_double(C):
    """quirk Q1 off: the gate is the density pow(det(2 pi A), -1/2) exp(-r / 2) itself, at the tolerance of test_gpu_surface.py's
    test_probability_as_double_branch (rtol 1e-11, atol 1e-300): device pow / exp against numpy's, a few ulps.  This pair has
    slots with r up to 1198 (weights down to 4e-262), where exp(-r / 2) turns an error of r into a relative one: A = C_t + R C_s
    R^T has condition 2 / 2e-3 = 1000, and the closed form of corr_eval differs from the reference's sequence of operations by
    6e-11 in r at r = 774 -- 3e-11 in the weight, which this test found.  The kernels now follow the reference's sequence for
    the double (corr_eval_literal), and the two paths agree bit for bit."""
    src, sl, tgt, tl, qt = cases.labelled_pair(C)
    runs = _weights_of_every_path(C, 4, 0, src, sl, tgt, tl, qt)
    for path, idx, w, want, scov, tcov in runs:
        live = idx >= 0
        _, r, _ = L.gate(qt, src, scov, tgt, tcov, idx)
        rel = np.abs(w - want) / np.maximum(want, 1e-300)
        worst = np.unravel_index(np.argmax(rel), rel.shape)
        print(f"C {C} as double, {path}: largest relative error {rel.max():.3g} at r = {r[worst]:.1f} (w = {want[worst]:.3g}), "
              f"slots above 1e-11: {int((rel > 1e-11).sum())} of {rel.size}, largest r {r.max():.1f}, smallest weight {want[live].min():.3g}")
        assert live.all() and (want > 1e-290).all() and (w <= 1.0).all()
        assert np.array_equal(w, runs[0][2])
    for path, idx, w, want, _, _ in runs:
        assert np.allclose(w, want, rtol=1e-11, atol=1e-300), path


# ---- 3. gate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", [0, PROFILE_WEIGHT], ids=["epilogue", "kernel"])
def test_gate_on_both_sides_of_its_thresholds(profile):
    src, sl, tgt, tl, poses = cases.gate_planes()
    cm = cases.matrix(4)
    by_reference = dict(below=0, band_one=0, band_zero=0, above=0)
    by_device = dict(by_reference)
    with _engine(4, profile=profile) as e:
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        scov, snrm, sh, _ = e.covariances(SRC, want_hist=True)
        tcov, tnrm, th, _ = e.covariances(TGT, want_hist=True)
        assert np.array_equal(np.abs(snrm), np.tile([0.0, 0.0, 1.0], (len(src), 1))) and np.array_equal(np.abs(tnrm), np.abs(snrm))
        for r0, qt in poses:
            st0 = e.stats()
            idx, d2, w = e.correspondences(qt)
            st1 = e.stats()
            assert st1["weights_in_search"] - st0["weights_in_search"] == (0 if profile else 1)
            assert st1["weight_launches"] - st0["weight_launches"] == (1 if profile else 0)
            assert (idx >= 0).all() and idx.shape == (2304, 4)
            g, r, logp = L.gate(qt, src, scov, tgt, tcov, idx)
            want = L.label_factor(L.projections(sh, cm, K), L.projections(th, cm, K), idx) * g
            sure = ~L.near_edge(logp)
            print(f"r {r0}: r of the slots {r.min():.4f} .. {r.max():.4f}, reference gate 1 at {int(g.sum())} of {g.size} slots, "
                  f"device w > 0 at {int((w > 0).sum())}, near the edge {int((~sure).sum())}, largest relative error {_rel(w, want):.3g}")
            assert np.abs(r - r0).max() < 0.013
            assert (~sure).mean() <= 0.01
            assert np.array_equal((w > 0)[sure], (g == 1)[sure]) and (w[sure & (g == 0)] == 0).all()
            assert np.allclose(w[sure], want[sure], rtol=1e-12, atol=0)
            for k, v in cases.regime_totals(r, g).items():
                by_reference[k] += v
            for k, v in cases.regime_totals(r, w).items():
                by_device[k] += v
    print("slots per regime, reference:", by_reference, "device:", by_device)
    assert by_reference == by_device == cases.GATE_TOTALS


# ---- 4. fused labels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate_sq", [cases.GATE_WIDE, cases.GATE_TIGHT], ids=["gate250", "tight"])
@pytest.mark.parametrize("C", cases.FUSED_CLASSES)
def test_fused_labels_equal_the_oracle(C, gate_sq):
    bad, sl, tgt, tl, qt, fin = cases.fused_pair(C)
    scores, want = cases.fused_reference(C, gate_sq)
    with _engine(C, gate_sq=gate_sq) as e:
        e.set_source(bad, sl)
        e.set_target(tgt, tl)
        got = e.fused_labels(qt)
    best, second, gap = L.top_two(scores)
    close = gap < 1e-9
    live = (cases.oracle_slots(C, gate_sq, fused=True)[0] >= 0).sum(axis=1)
    print(f"C {C} gate_sq {gate_sq}: labels differing {int((got[fin] != want).sum())} of {len(want)}, too close to call {int(close.sum())}, "
          f"points with 0 / 1-3 / 4 live slots {int((live == 0).sum())} / {int(((live > 0) & (live < 4)).sum())} / {int((live == 4).sum())}")
    assert got.dtype == np.uint32 and got.shape == (len(bad),)
    assert (~fin).sum() == 20 and (got[~fin] == 0).all()
    assert close.mean() <= 0.01
    assert np.array_equal(got[fin][~close], want[~close])
    assert ((got[fin][close] == best[close]) | (got[fin][close] == second[close])).all()
    assert (got[fin][live == 0] == 1).all() and ((live == 0).sum() > 0) == (gate_sq == cases.GATE_TIGHT)


@pytest.mark.parametrize("gate_sq", [cases.GATE_WIDE, cases.GATE_TIGHT], ids=["gate250", "tight"])
@pytest.mark.parametrize("C", [9, 17])
def test_fused_labels_with_the_probability_as_a_double(C, gate_sq):
    """quirk Q1 off: every slot's share of a class score is scaled by the density, not by 0 / 1 -- fused_label_literal_kernel
    against the restatement's scores with the gate as a double, from the engine's own covariances, counts and slots"""
    src, sl, tgt, tl, qt = cases.labelled_pair(C)
    cm = cases.matrix(C)
    with _engine(C, gate_sq=gate_sq, quirk_bool_probability=0) as e, _engine(C, gate_sq=gate_sq) as b:
        for h in (e, b):
            h.set_source(src, sl)
            h.set_target(tgt, tl)
        idx, _, _ = e.correspondences(qt)
        scov, _, sh, _ = e.covariances(SRC, want_hist=True)
        tcov, _, th, _ = e.covariances(TGT, want_hist=True)
        got, as_bool = e.fused_labels(qt), b.fused_labels(qt)
    assert np.array_equal(idx, cases.oracle_slots(C, gate_sq)[0])
    g, _, _ = L.gate(qt, src, scov, tgt, tcov, idx, as_bool=False)
    scores = L.fused_scores(L.projections(sh, cm, K), L.projections(th, cm, K), idx, g)
    want = L.fused_labels(scores)
    best, second, gap = L.top_two(scores)
    close = gap < 1e-9
    print(f"C {C} gate_sq {gate_sq} as double: labels differing {int((got != want).sum())} of {len(want)}, too close to call "
          f"{int(close.sum())}, differing from the bool's labels {int((got != as_bool).sum())}, points without a live slot {int((idx < 0).all(axis=1).sum())}")
    assert close.mean() <= 0.01
    assert np.array_equal(got[~close], want[~close])
    assert ((got[close] == best[close]) | (got[close] == second[close])).all()
    assert (got != as_bool).sum() > 0   # (the density weighs the slots differently: the branch changes labels)


# ---- 5. batches -------------------------------------------------------------------------------------------------------------------
def test_align_batch_at_17_classes_equals_the_lone_aligns():
    """five pairs in one batch (more than four: the weights stay in em_weight_jobs_kernel), sources of ragged sizes: the byte-walk
    side of cov_jobs_kernel, proj_jobs_kernel and the generic em_weight_jobs_kernel in launches of several jobs against launches of one"""
    src, sl, tgt, tl, _ = cases.labelled_pair(17)
    engines, singles = [], []
    try:
        for n in cases.BATCH_SIZES:
            e = _engine(17)
            e.set_source(src[:n], sl[:n])
            e.set_target(tgt, tl)
            engines.append(e)
            singles.append(e.align(IDENT))
        batch = sicp.align_batch(engines)
        for n, (qb, sb), (q1, s1) in zip(cases.BATCH_SIZES, batch, singles):
            print(f"n {n}: outer iterations {s1['outer_iters']} / {sb['outer_iters']}, pose bits equal {qb.tobytes() == q1.tobytes()}")
            assert qb.tobytes() == q1.tobytes() and sb["outer_iters"] == s1["outer_iters"] and s1["outer_iters"] >= 2
            assert sb["total_active"] == s1["total_active"] and sb["weight_launches"] == sb["outer_iters"] and sb["weights_in_search"] == 0
        assert len({q.tobytes() for q, _ in singles}) == len(singles)
    finally:
        for e in engines:
            e.close()


Q1_OFF_BATCHES = [   # (id, C, quirk_bool_probability per pair)
    ("epilogue_jobs", 9, (0, 0, 0)),          # at most 4 pairs: the weights come from the job search's epilogue
    ("rows4_jobs", 9, (0, 0, 0, 0, 0)),       # more: em_weight_rows4_literal_jobs_kernel
    ("generic_jobs", 17, (0, 0, 0)),          # beyond 16 classes: em_weight_literal_jobs_kernel
    ("mixed_epilogue", 16, (1, 0, 1)),        # one double handle puts the whole launch on the kernels that hold both forms:
    ("mixed_rows4", 16, (1, 0, 1, 1, 0)),     # the bool handles' weights must stay the closed form's, bit for bit
    ("mixed_generic", 17, (0, 1, 1)),
]


@pytest.mark.parametrize("C,quirks", [c[1:] for c in Q1_OFF_BATCHES], ids=[c[0] for c in Q1_OFF_BATCHES])
def test_align_batch_with_the_probability_as_a_double_equals_the_lone_aligns(C, quirks):
    """job launches of the kernels that compute Probability() as a double, and the rule that one such job in a launch
    takes the whole launch to them: per pair the batch gives the lone align's bits, whatever its neighbours in the batch are"""
    src, sl, tgt, tl, _ = cases.labelled_pair(C)
    engines, singles = [], []
    try:
        for n, q in zip(cases.BATCH_SIZES, quirks):
            e = _engine(C, quirk_bool_probability=q)
            e.set_source(src[:n], sl[:n])
            e.set_target(tgt, tl)
            engines.append(e)
            singles.append(e.align(IDENT))
        batch = sicp.align_batch(engines)
        for n, q, (qb, sb), (q1, s1) in zip(cases.BATCH_SIZES, quirks, batch, singles):
            print(f"C {C} n {n} bool {q}: outer iterations {s1['outer_iters']} / {sb['outer_iters']}, weights in search {sb['weights_in_search']}, "
                  f"weight launches {sb['weight_launches']}, pose bits equal {qb.tobytes() == q1.tobytes()}")
            assert qb.tobytes() == q1.tobytes() and sb["outer_iters"] == s1["outer_iters"] and s1["outer_iters"] >= 2
            assert sb["total_active"] == s1["total_active"] and sb["total_evals"] == s1["total_evals"]
            assert sb["weights_in_search"] + sb["weight_launches"] == sb["outer_iters"]   # the counters say which kernels ran
            assert (sb["weights_in_search"] >= 1) == (C <= 16 and len(quirks) <= 4)
        # the double really is another registration than the bool's
        if 0 in quirks and 1 not in quirks:
            with _engine(C) as b:
                b.set_source(src[:cases.BATCH_SIZES[0]], sl[:cases.BATCH_SIZES[0]])
                b.set_target(tgt, tl)
                assert b.align(IDENT)[0].tobytes() != singles[0][0].tobytes()
    finally:
        for e in engines:
            e.close()
