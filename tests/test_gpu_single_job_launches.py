"""A stage launched by a handle for itself against the same stage collected into a job launch.

Two handles hold the same clouds.  One has profile = 0: its align() is a batch of one pair, every stage between two solves
goes into the batch's job lists.  The other has profile = 7 (search, covariance and weight timers): every stage is a launch
of its own on the handle's stream, and EM weights come from the weight kernel behind the search where the first handle's
come from the search's epilogue.  Both must give the same pose bytes and the same outer_iters, total_active and
total_lm_iters -- EM at K = 4 on both sides of 16 classes with Probability() as a bool and as a double, GICP at K = 1,
SEMANTIC with a source segment the target lacks and one too small to be searched, at source sizes below one leaf of the
search tree and off every multiple of 16, 64 and 256, against targets of other sizes.  One case also compares what the
inspection hooks (correspondences, covariances), which launch for themselves on either handle, report afterwards."""
import functools
import importlib

import numpy as np
import pytest

import synth
from test_gpu_surface import IDENT, make_engine

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
SRC, TGT = sicp.SOURCE, sicp.TARGET
PROFILE_STAGES = 7  # SICP_PROFILE_NN | SICP_PROFILE_COV | SICP_PROFILE_WEIGHT
SIZES = {61: 257, 333: 1000, 4099: 4500}  # source points: target points
MIN_CLASS_PTS = 5


@functools.lru_cache(maxsize=None)
def _scans():
    src, sl, tgt, tl, _, _ = synth.lidar_pair(seed=4, n_points=max(SIZES.values()))
    for a in (src, sl, tgt, tl):
        a.setflags(write=False)
    return src, sl, tgt, tl


def _spread(n, count):
    """`count` of n indices, evenly spread: a thinned scan, not a corner of it"""
    return np.round(np.linspace(0, n - 1, count)).astype(np.int64)


def _clouds(n_s, mode, C):
    src, sl, tgt, tl = _scans()
    si, ti = _spread(len(src), n_s), _spread(len(tgt), SIZES[n_s])
    src, sl, tgt, tl = src[si], sl[si].copy(), tgt[ti], tl[ti].copy()
    if mode == sicp.MODE_EM:  # the scan's labels folded into 1..C, three in ten moved on: every class reaches neighbourhoods
        rng = np.random.default_rng([C, n_s])
        sl = (1 + (sl + rng.integers(0, C, len(sl)) * (rng.random(len(sl)) < 0.3)) % C).astype(np.uint32)
        tl = (1 + (tl + rng.integers(0, C, len(tl)) * (rng.random(len(tl)) < 0.3)) % C).astype(np.uint32)
    elif mode == sicp.MODE_SEMANTIC:
        # three segments on both sides; label 7 on the source only; label 8 on both, the source's of MIN_CLASS_PTS points
        sl, tl = 1 + sl % 3, 1 + tl % 3
        sl[3:3 + 8 * 7:7] = 7
        sl[0:MIN_CLASS_PTS * 11:11] = 8
        tl[2:2 + 9 * 13:13] = 8
        assert (sl == 7).sum() == 8 and (tl == 7).sum() == 0 and (sl == 8).sum() == MIN_CLASS_PTS and (tl == 8).sum() == 9
        assert all((sl == c).sum() > MIN_CLASS_PTS and (tl == c).sum() > 0 for c in (1, 2, 3))
    return src, sl, tgt, tl


def _pair_of_handles(n_s, mode, C=0, **kw):
    src, sl, tgt, tl = _clouds(n_s, mode, C)
    out = []
    for profile in (0, PROFILE_STAGES):
        e = make_engine(mode, C, synth.confusion_matrix(C) if mode == sicp.MODE_EM else None, profile=profile, **kw)
        e.set_source(src, None if mode == sicp.MODE_GICP else sl)
        e.set_target(tgt, None if mode == sicp.MODE_GICP else tl)
        out.append(e)
    return out


def _aligns_agree(collected, own):
    qa, sa = collected.align(IDENT)
    qb, sb = own.align(IDENT)
    keys = ("outer_iters", "total_active", "total_lm_iters")
    print(f"pose {qa}, " + ", ".join(f"{k} {sa[k]} | {sb[k]}" for k in keys) +
          f"; own launches of the profiled handle: search {sb['nn_launches']}, covariance {sb['cov_launches']}, weight {sb['weight_launches']}")
    assert sa["nn_launches"] == 0 and sa["cov_launches"] == 0  # (collected: none of its own)
    assert sb["nn_launches"] > 0 and sb["cov_launches"] > 0
    assert qa.tobytes() == qb.tobytes()
    assert [sa[k] for k in keys] == [sb[k] for k in keys]
    assert sa["outer_iters"] >= 1 and sa["total_active"] > 0
    return qa


@pytest.mark.parametrize("n_s", sorted(SIZES))
@pytest.mark.parametrize("bool_q", [1, 0])
@pytest.mark.parametrize("C", [9, 17])
def test_em_align_collected_and_launched_alone(C, bool_q, n_s):
    a, b = _pair_of_handles(n_s, sicp.MODE_EM, C, knn=4, quirk_bool_probability=bool_q)
    with a, b:
        _aligns_agree(a, b)


@pytest.mark.parametrize("n_s", sorted(SIZES))
def test_gicp_align_collected_and_launched_alone(n_s):
    a, b = _pair_of_handles(n_s, sicp.MODE_GICP, knn=1)
    with a, b:
        _aligns_agree(a, b)


@pytest.mark.parametrize("n_s", sorted(SIZES))
def test_semantic_align_collected_and_launched_alone(n_s):
    a, b = _pair_of_handles(n_s, sicp.MODE_SEMANTIC, min_class_pts=MIN_CLASS_PTS)
    with a, b:
        _aligns_agree(a, b)


def test_hooks_after_an_align_agree_bit_for_bit():
    a, b = _pair_of_handles(4099, sicp.MODE_EM, 9, knn=4)
    with a, b:
        qt = _aligns_agree(a, b)
        before = [e.stats()["weights_in_search"] for e in (a, b)]
        ia, _, wa = a.correspondences(qt)  # the search's epilogue writes the weights ...
        ib, _, wb = b.correspondences(qt)  # ... the weight kernel behind the search does
        assert [e.stats()["weights_in_search"] - n for e, n in zip((a, b), before)] == [1, 0]
        assert (ia >= 0).any() and np.array_equal(ia, ib)
        assert wa.tobytes() == wb.tobytes() and (wa > 0).any()
        for which in (SRC, TGT):
            ca, na, ha, nna = a.covariances(which, want_hist=True, want_nn=True)
            cb, nb, hb, nnb = b.covariances(which, want_hist=True, want_nn=True)
            assert np.array_equal(nna, nnb) and np.array_equal(ha, hb)
            assert na.tobytes() == nb.tobytes() and ca.tobytes() == cb.tobytes()
