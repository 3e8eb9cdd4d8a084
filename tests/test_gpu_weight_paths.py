"""The EM weights must be the same bits whichever kernel writes them: em_weight_rows_body behind the search
and the K = 4 search's own epilogue (KnnArgs::w_*) -- checked against each other with np.array_equal and against the
restatement (tests/label_path_ref.py) at the tolerances of tests/test_gpu_label_path.py: rtol 1e-12 with Probability() as a
bool, rtol 1e-11 / atol 1e-300 as a double.  The shapes are tests/weight_path_cases.py's.  Streams and batches of 16 pairs
or more take the epilogue in job launches (JobCollector::fold_weights): a stream with more than 4 registrations in flight and a
batch of 16 ragged pairs give the lone aligns' poses and counters.  (The dense per-point arrays the accumulate kernel gathers
from were tried for the weight code as well and did not pay -- DESIGN.md 7 -- so there is no third path to compare.)"""
import importlib

import numpy as np
import pytest

import synth
import weight_path_cases as W

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
C_ALIGN = 11


@pytest.mark.parametrize("quirk", W.QUIRKS, ids=["bool", "double"])
@pytest.mark.parametrize("C", W.CLASSES)
def test_both_kernels_give_the_same_bits(C, quirk):
    got, want = W.run(C, quirk, reference=True)
    dead = live = 0
    worst = 0.0
    for n_t in W.N_T:
        for n_s in W.N_S:
            k0, k4 = W.key(C, quirk, n_t, n_s, 0), W.key(C, quirk, n_t, n_s, W.PROFILE_WEIGHT)
            idx, w = got[k0]                                  # the search's epilogue
            assert idx.shape == (n_s, 4) and w.shape == (n_s, 4) and np.isfinite(w).all()
            assert np.array_equal(got[k4][0], idx) and np.array_equal(got[k4][1], w), k4   # the weight kernel behind the search
            gone = idx < 0
            assert (w[gone] == 0).all() and not np.signbit(w[gone]).any()      # exactly +0.0
            ref = want[k0]
            nz = ref != 0
            worst = max(worst, float(np.max(np.abs(w[nz] - ref[nz]) / np.abs(ref[nz]), initial=0.0)))
            if quirk:
                assert np.allclose(w, ref, rtol=1e-12, atol=0), k0
                assert np.array_equal(w == 0, ref == 0), k0
            else:
                assert np.allclose(w, ref, rtol=1e-11, atol=1e-300), k0
            dead += int(gone.sum())
            live += int((~gone).sum())
    print(f"C {C} bool {quirk}: slots live {live}, gated out {dead}, largest relative error against the restatement {worst:.3g}")
    assert dead > 0 and live > 0


def _lone(p, cm, src, sl, tgt, tl):
    with sicp.Engine(0, p) as e:
        e.set_confusion(cm)
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        return e.align(IDENT)


def _same_registration(st, s1):
    for name in ("outer_iters", "total_lm_iters", "total_evals", "total_corr"):
        assert st[name] == s1[name], name
    assert s1["outer_iters"] >= 2


def test_stream_with_more_than_four_in_flight_equals_the_lone_aligns():
    """6 registrations of 2000-point pairs, 5 in flight, every one recomputing its features (SICP_SUBMIT_FRESH_FEATURES): every
    search of a registration, the first included, writes its weights itself"""
    cm = synth.confusion_matrix(C_ALIGN)
    pairs = [synth.lidar_pair(seed=40 + k, n_points=2000)[:4] for k in range(6)]
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = C_ALIGN
    with sicp.Stream(0, p, max_in_flight=5, confusion=cm) as S:
        tickets = {}
        for k, (src, sl, tgt, tl) in enumerate(pairs):
            tickets[S.submit(S.add_cloud(src, sl), S.add_cloud(tgt, tl), IDENT, fresh_features=True)] = k
        got = S.drain()
    assert len(got) == len(pairs)
    for ticket, status, qt, st in got:
        assert status == sicp.OK
        q1, s1 = _lone(p, cm, *pairs[tickets[ticket]])
        print(f"pair {tickets[ticket]}: outer {st['outer_iters']} / {s1['outer_iters']}, evaluations {st['total_evals']} / {s1['total_evals']}, "
              f"weights in search {st['weights_in_search']}, weight launches {st['weight_launches']}")
        assert qt.tobytes() == q1.tobytes()
        _same_registration(st, s1)
        assert st["weights_in_search"] == st["outer_iters"] and st["weight_launches"] == 0


def test_batch_of_sixteen_ragged_pairs_equals_the_lone_aligns():
    """16 pairs -- two job launches of 8 searches -- with sources of 2000 down to 1985 points: the batch flushes the features
    ahead of the first searches, so the weights of every search come from the job search's epilogue"""
    cm = synth.confusion_matrix(C_ALIGN)
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = C_ALIGN
    pairs = []
    for k in range(16):
        src, sl, tgt, tl = synth.lidar_pair(seed=40 + k % 4, n_points=2000)[:4]
        pairs.append((src[:2000 - k], sl[:2000 - k], tgt, tl))
    engines = []
    try:
        for src, sl, tgt, tl in pairs:
            e = sicp.Engine(0, p)
            engines.append(e)
            e.set_confusion(cm)
            e.set_source(src, sl)
            e.set_target(tgt, tl)
        batch = sicp.align_batch(engines)
        in_search = 0
        for (qb, sb), pr in zip(batch, pairs):
            q1, s1 = _lone(p, cm, *pr)
            assert qb.tobytes() == q1.tobytes()
            _same_registration(sb, s1)
            assert sb["weights_in_search"] + sb["weight_launches"] == sb["outer_iters"]
            in_search += sb["weights_in_search"]
        searches = sum(sb["outer_iters"] for _, sb in batch)
        print(f"16 pairs: weights in search {in_search} of {searches} searches")
        assert in_search == searches
    finally:
        for e in engines:
            e.close()
