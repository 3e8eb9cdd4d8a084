"""The accumulate kernel gathers its target records from the dense per-point arrays (AccArgs::trec_dense; DESIGN.md 3.1,
"dense gathers") whenever a cloud's dense copy is current.  A stale or mis-pitched copy would give silently wrong sums, so
sicp_accumulate is checked against the oracle's literal accumulate -- on the covariances the engine reports from the 48-byte
records, i.e. the copy the gathers no longer read -- wherever the dense copy is written, re-pitched or invalidated:
target sizes around a wave, clouds of different sizes, every mode, caller-set normals, re-set clouds, recycled handles,
clouds shared inside a stream.  Tolerances are those of the existing parity tests (test_gpu_validation.py): rtol 1e-9,
atol 1e-9 x the largest entry; a lone handle, a batch and a stream agree bit for bit."""
import importlib

import numpy as np
import pytest

import oracle_lib as O
import synth
from np_ref import mat_to_qt

pytestmark = pytest.mark.gpu

sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
C = 11


def make_engine(mode, **kw):
    p = sicp.default_params(mode)
    p.num_classes = C if mode == sicp.MODE_EM else 0
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    if mode == sicp.MODE_EM:
        e.set_confusion(synth.confusion_matrix(C))
    return e


def oracle_params(mode):
    p = O.default_params(mode)
    p.num_classes = C if mode == sicp.MODE_EM else 0
    p.use_kdtree = 1
    return p


def set_clouds(e, mode, src, sl, tgt, tl):
    lab = mode != sicp.MODE_GICP
    e.set_source(src, sl if lab else None)
    e.set_target(tgt, tl if lab else None)


def assert_close(got, ref, what=""):
    print(f"{what}: max |got - ref| = {np.abs(got - ref).max():.3e}, max |ref| = {np.abs(ref).max():.3e}")
    assert np.isfinite(ref).all() and np.isfinite(got).all(), what
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max()), (what, got, ref)


def check_against_oracle(e, mode, src, tgt, qt, what, scov=None, tcov=None):
    """sicp_accumulate at qt on the handle's current clouds against the oracle on the same correspondences, weights and
    covariances; returns the 28 sums"""
    idx, d2, w = e.correspondences(qt)
    got = e.accumulate(qt)
    assert np.array_equal(got, e.accumulate(qt))
    cs = e.covariances(sicp.SOURCE)[0] if scov is None else scov
    ct = e.covariances(sicp.TARGET)[0] if tcov is None else tcov
    ref = O.accumulate(oracle_params(mode), qt, src, cs, tgt, ct, idx, w)
    assert (idx >= 0).any(), what
    assert_close(got, ref, what)
    return got


@pytest.fixture(scope="module")
def lidar20k():
    return synth.lidar_pair(seed=2, n_points=20000)


@pytest.fixture(scope="module")
def lidar_big():
    return synth.lidar_pair(seed=7, n_points=100003)


SMALL = [(sicp.MODE_GICP, n) for n in (1, 5, 63, 64, 65)] + [(sicp.MODE_EM, n) for n in (5, 63, 64, 65)]   # (EM-ICP needs K = 4 targets)


@pytest.mark.parametrize("mode,n_t", SMALL, ids=[f"{'gicp_k1' if m == sicp.MODE_GICP else 'em_k4'}-{n}" for m, n in SMALL])
def test_small_targets_around_a_wave(lidar20k, mode, n_t):
    """targets of 1, 5, 63, 64 and 65 points under 3000 source points: every gather lands in a few lines, the pitch of the
    dense arrays is tiny and odd"""
    src, sl, tgt, tl, T, _ = lidar20k
    src, sl = src[::6][:3000], sl[::6][:3000]
    pick = np.linspace(0, len(tgt) - 1, n_t).astype(int) if n_t > 1 else np.array([len(tgt) // 2])
    tg, tgl = np.ascontiguousarray(tgt[pick]), np.ascontiguousarray(tl[pick])
    with make_engine(mode, gate_sq=1e30, reuse_features=1 if n_t == 1 else 0) as e:
        set_clouds(e, mode, src, sl, tg, tgl)
        tcov = None
        if n_t == 1:
            # (one point has no PCA normal: the caller's, of the engine's form -- written by set_normals_kernel)
            v = np.array([0.6, 0.0, 0.8])
            tcov = (np.eye(3) - (1 - 1e-3) * np.outer(v, v)).reshape(1, 3, 3)
            e.set_covariances(sicp.TARGET, tcov)
        check_against_oracle(e, mode, src, tg, mat_to_qt(T), f"n_t = {n_t}", tcov=tcov)


@pytest.mark.parametrize("mode", [sicp.MODE_EM, sicp.MODE_GICP], ids=["em_k4", "gicp_k1"])
def test_full_size_target_and_different_sizes(lidar_big, mode):
    """a target of 100 003 points (not a multiple of anything) under a source of the same and of a different size; a lone
    handle and a batch of the two agree bit for bit"""
    src, sl, tgt, tl, T, _ = lidar_big
    qt = mat_to_qt(T)
    es, outs = [], []
    try:
        for n_s in (len(src), 70001):
            e = make_engine(mode)
            es.append(e)
            set_clouds(e, mode, src[:n_s], sl[:n_s], tgt, tl)
            outs.append(check_against_oracle(e, mode, src[:n_s], tgt, qt, f"{n_s} x {len(tgt)}"))
        # and a small target under the big source, in the same batch
        e = make_engine(mode)
        es.append(e)
        set_clouds(e, mode, src, sl, tgt[:30011], tl[:30011])
        outs.append(check_against_oracle(e, mode, src, tgt[:30011], qt, f"{len(src)} x 30011"))
        batch, _ = sicp.accumulate_batch(es, np.tile(qt, (len(es), 1)))
        for p in range(len(es)):
            assert np.array_equal(batch[p], outs[p]), p
    finally:
        for e in es:
            e.close()


def test_semantic_with_several_label_segments():
    """SICP_MODE_SEMANTIC: the clouds are laid out label segment by label segment, the gathers cross segment borders of the
    one dense copy"""
    src, sl, tgt, tl, T = synth.config1_pair(seed=1, n_per_label=700)
    assert len(np.unique(tl)) >= 3
    qt = mat_to_qt(synth.pose_matrix(1.0, (0, 1, 0), (0.05, 0.0, -0.02)))
    with make_engine(sicp.MODE_SEMANTIC) as e, make_engine(sicp.MODE_SEMANTIC) as e2:
        set_clouds(e, sicp.MODE_SEMANTIC, src, sl, tgt, tl)
        a = check_against_oracle(e, sicp.MODE_SEMANTIC, src, tgt, qt, "semantic")
        keep = tl != tl[0]                                   # a target without one of the labels: another segment layout
        set_clouds(e2, sicp.MODE_SEMANTIC, src, sl, tgt[keep], tl[keep])
        b = check_against_oracle(e2, sicp.MODE_SEMANTIC, src, tgt[keep], qt, "semantic, one label less")
        batch, _ = sicp.accumulate_batch([e, e2], np.tile(qt, (2, 1)))
        assert np.array_equal(batch[0], a) and np.array_equal(batch[1], b)


def test_target_normals_set_by_the_caller(lidar20k):
    """sicp_set_covariances of the engine's form rewrites the records through set_normals_kernel: the gathers must see the
    caller's normals, and the PCA ones again after the cloud is set anew"""
    src, sl, tgt, tl, T, _ = lidar20k
    src, tgt = src[:9000], tgt[:8000]
    rng = np.random.default_rng(5)
    v = rng.normal(size=(len(tgt), 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ct = np.eye(3)[None] - (1 - 1e-3) * v[:, :, None] * v[:, None, :]
    qt = mat_to_qt(T)
    with make_engine(sicp.MODE_GICP, reuse_features=1) as e:
        e.set_source(src); e.set_target(tgt)
        pca = check_against_oracle(e, sicp.MODE_GICP, src, tgt, qt, "PCA normals")
        e.set_covariances(sicp.TARGET, ct)
        own = check_against_oracle(e, sicp.MODE_GICP, src, tgt, qt, "caller normals", tcov=ct)
        assert not np.array_equal(own, pca)
        e.set_target(tgt)
        assert np.array_equal(check_against_oracle(e, sicp.MODE_GICP, src, tgt, qt, "PCA normals again"), pca)


@pytest.mark.parametrize("mode", [sicp.MODE_EM, sicp.MODE_GICP], ids=["em_k4", "gicp_k1"])
def test_smaller_cloud_after_a_larger_one(lidar20k, mode):
    """a handle whose target is replaced by a smaller one (the buffers stay, the pitch changes), and a handle that takes its
    clouds from the pool after a larger cloud was released into it"""
    src, sl, tgt, tl, T, _ = lidar20k
    qt = mat_to_qt(T)
    small = slice(0, 7001)
    with make_engine(mode) as e:
        set_clouds(e, mode, src, sl, tgt, tl)
        check_against_oracle(e, mode, src, tgt, qt, "large")
        e.set_target(tgt[small], tl[small] if mode != sicp.MODE_GICP else None)
        want = check_against_oracle(e, mode, src, tgt[small], qt, "small after large, same handle")
        e.set_target(tgt[1000:8001], tl[1000:8001] if mode != sicp.MODE_GICP else None)   # the same size, other points
        check_against_oracle(e, mode, src, tgt[1000:8001], qt, "same size, other points")
    # the clouds of the closed handle are in the pool now
    with make_engine(mode) as e:
        set_clouds(e, mode, src, sl, tgt[small], tl[small])
        got = check_against_oracle(e, mode, src, tgt[small], qt, "small after large, recycled clouds")
        assert np.array_equal(got, want)


def test_stream_with_shared_clouds_and_fresh_features():
    """a chain of registrations in one stream -- every cloud is one pair's source and the next pair's target, of its own
    size, half of the registrations recompute the features of both their clouds (SICP_SUBMIT_FRESH_FEATURES) while others
    are in flight: every pose is bit-equal to a lone handle's"""
    cm = synth.confusion_matrix(C)
    sizes = [6000, 4501, 7003, 5000, 6500, 3999, 7003, 5200, 6100]
    scans = []
    for k, n in enumerate(sizes):
        s, l, *_ = synth.lidar_pair(seed=20, n_points=8000, motion=(0.3 * k, 0.5 * k))   # one street, nine places
        scans.append((np.ascontiguousarray(s[:n]), np.ascontiguousarray(l[:n])))
    p = sicp.default_params(sicp.MODE_EM)
    p.num_classes = C
    with sicp.Stream(0, p, max_in_flight=4, confusion=cm) as S:
        ids = [S.add_cloud(*sc) for sc in scans]
        tickets = {}
        for rep in range(2):
            for k in range(len(scans) - 1):
                tickets[S.submit(ids[k + 1], ids[k], IDENT, fresh_features=(k + rep) % 2 == 0)] = k
        got = S.drain()
    assert len(got) == len(tickets)
    lone = {}
    for ticket, status, qt, st in got:
        assert status == sicp.OK
        k = tickets[ticket]
        if k not in lone:
            with make_engine(sicp.MODE_EM) as e:
                e.set_source(*scans[k + 1]); e.set_target(*scans[k])
                lone[k] = e.align(IDENT)
        assert np.array_equal(qt, lone[k][0]), (k, qt, lone[k][0])
        assert st["total_evals"] == lone[k][1]["total_evals"], k
