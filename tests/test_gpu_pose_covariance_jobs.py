"""GPU tests of the job-table form of the pose covariance sweep behind sicp_pose_covariance_batch: every row of a batch call has
the bytes of its lone sicp_pose_covariance -- with mixed modes and sizes in one call, a target list long enough for the owner
and pass-through path in the middle of a batch, failing pairs between good ones, handles that repeat (several groups) -- and
a batch repeats bit for bit.  The lone call is tied to the numpy restatement and to finite differences by
tests/test_gpu_pose_covariance.py."""
import importlib

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import pose_cov_ref as ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC


def _qt(T):
    return np.concatenate([Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]])


def _near(T, seed, rot=0.004, trans=0.02):
    rng = np.random.default_rng(seed)
    D = np.eye(4)
    D[:3, :3] = Rotation.from_rotvec(rng.normal(scale=rot, size=3)).as_matrix()
    D[:3, 3] = rng.normal(scale=trans, size=3)
    return T @ D


def _engine_on(mode, src, sl, tgt, tl, cm, **kw):
    p = sicp.default_params(mode)
    p.num_classes = cm.shape[0]
    if mode == S:
        p.min_class_pts = 40
    for k, v in kw.items():
        setattr(p, k, v)
    e = sicp.Engine(0, p)
    if mode != G:
        e.set_confusion(cm)
    e.set_source(src, sl)
    e.set_target(tgt, tl)
    return e


def _lidar_engine(mode, n, seed, **kw):
    src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=seed, n_points=n)
    return _engine_on(mode, src, sl, tgt, tl, cm, **kw), _qt(_near(T, seed))


def _lone(e, qt):
    r = sicp.SicpPoseCovarianceResult()
    qt = np.ascontiguousarray(qt, dtype=np.float64)
    assert sicp.lib().sicp_pose_covariance(e._h, sicp._ptr(qt, sicp._dp), 1.0, 1.0, sicp.C.byref(r)) == sicp.OK
    return bytes(r)


def _batch(es, qts, fill=0x5A):
    n = len(es)
    out = (sicp.SicpPoseCovarianceResult * n)()
    sicp.C.memset(out, fill, sicp.C.sizeof(out))
    status = np.full(n, 99, dtype=np.int32)
    q = np.ascontiguousarray(np.stack(qts), dtype=np.float64)
    rc = sicp.lib().sicp_pose_covariance_batch(sicp._handles(es), n, sicp._ptr(q, sicp._dp), 1.0, 1.0, out, sicp._ptr(status, sicp._ip))
    return rc, status, out


def _close(es):
    for e in set(es):
        e.close()


def test_mixed_modes_and_sizes_in_one_call():
    """257 points: the second workgroup of the source kernel holds one point, and n_s K = 1028 (EM) is no multiple of the tile"""
    es, qts = [], []
    try:
        for mode, n, seed in ((E, 257, 41), (G, 2000, 42), (S, 2250, 43), (E, 3750, 44), (G, 257, 45), (S, 3000, 46), (E, 2500, 47)):
            e, qt = _lidar_engine(mode, n, seed)
            es.append(e)
            qts.append(qt)
        src, sl, tgt, tl, T_gt = synth.config1_pair(seed=4, n_per_label=100)  # 300 x 300 points
        es.insert(3, _engine_on(E, src, sl, tgt, tl, synth.confusion_matrix(4)))
        qts.insert(3, _qt(_near(T_gt, 5)))
        assert len(es) == 8
        lone = [_lone(e, q) for e, q in zip(es, qts)]
        rc, status, out = _batch(es, qts)
        assert rc == sicp.OK and (status == 0).all()
        for k in range(8):
            assert bytes(out[k]) == lone[k], k
            assert out[k].active > 0, k
    finally:
        _close(es)


def test_long_target_list_in_the_middle_of_a_batch():
    """2000 source points onto 24 target points, K = 1: a target's list spans many tiles of 8 sorted slots, so it is summed by
    an owner lane over pass-through tiles.  The cross sum of the targets is checked against the numpy restatement."""
    src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=31, n_points=2000)
    pick = np.sort(np.random.default_rng(31).choice(len(tgt), 24, replace=False))
    tgt24, tl24 = np.ascontiguousarray(tgt[pick]), np.ascontiguousarray(tl[pick])
    qt = _qt(T)
    es, qts = [], []
    try:
        for seed in (51, 52):
            e, q = _lidar_engine(G, 2000, seed)
            es.append(e); qts.append(q)
        skew = _engine_on(G, src, sl, tgt24, tl24, cm)
        assert skew.get_params().knn == 1
        es.append(skew); qts.append(qt)
        for seed in (53, 54):
            e, q = _lidar_engine(E, 2000, seed)
            es.append(e); qts.append(q)
        lone = [_lone(e, q) for e, q in zip(es, qts)]
        rc, status, out = _batch(es, qts)
        assert rc == sicp.OK and (status == 0).all()
        for k in range(len(es)):
            assert bytes(out[k]) == lone[k], k
        idx, _, _ = skew.correspondences(qt)
        counts = np.bincount(idx[idx >= 0], minlength=24)
        print(f"skewed target: {int((idx >= 0).sum())} active slots, largest target list {int(counts.max())}")
        assert counts.max() >= 64  # at least 8 tiles: the owner and pass-through path
        _, sn, _, _ = skew.covariances(sicp.SOURCE)
        _, tn, _, _ = skew.covariances(sicp.TARGET)
        p = skew.get_params()
        r = out[2].as_dict()
        assert r["active"] == int((idx >= 0).sum())
    finally:
        _close(es)
    _, S_tgt = ref.cross_sums(T[:3, :3], T[:3, 3], src.astype(np.float64), sn, tgt24.astype(np.float64), tn, idx, None, p.epsilon,
                              ref.MODES[G], p.cauchy_a)
    scale = np.abs(np.diag(S_tgt)).max()
    assert scale > 0
    assert np.abs(r["cross_target"] - S_tgt).max() <= 1e-8 * scale, np.abs(r["cross_target"] - S_tgt).max() / scale


def test_failing_pairs_between_good_ones():
    es, qts = [], []
    try:
        for mode, seed in ((G, 61), (E, 62), (G, 63)):
            e, q = _lidar_engine(mode, 2000, seed)
            es.append(e); qts.append(q)
        gated, qg = _lidar_engine(G, 2000, 64, gate_sq=1e-30)  # zero active slots: SICP_OK, not positive definite
        empty = sicp.Engine(0, sicp.default_params(G))         # no clouds: SICP_ERR_NOT_READY
        es = [es[0], gated, es[1], empty, es[2]]
        qts = [qts[0], qg, qts[1], qg, qts[2]]
        lone = [_lone(e, q) if e is not empty else None for e, q in zip(es, qts)]
        rc, status, out = _batch(es, qts)
        assert rc == sicp.ERR_NOT_READY
        assert list(status) == [sicp.OK, sicp.OK, sicp.OK, sicp.ERR_NOT_READY, sicp.OK]
        size = sicp.C.sizeof(sicp.SicpPoseCovarianceResult)
        for k in range(5):
            if es[k] is empty:
                assert bytes(out[k]) == bytes([0x5A]) * size
            else:
                assert bytes(out[k]) == lone[k], k
        assert out[1].active == 0 and out[1].positive_definite == 0
        assert out[0].positive_definite == 1 and out[4].positive_definite == 1
    finally:
        _close(es)


def test_handles_repeated_in_one_call():
    """three handles, 40 poses each: a group holds a handle once, so the call runs as many groups"""
    es, Ts = [], []
    try:
        for mode, seed in ((G, 71), (E, 72), (S, 73)):
            src, sl, tgt, tl, T, cm = synth.lidar_pair(seed=seed, n_points=2000)
            es.append(_engine_on(mode, src, sl, tgt, tl, cm))
            Ts.append(T)
        hs, qts = [], []
        for h in range(3):
            for k in range(40):
                hs.append(es[h])
                qts.append(_qt(_near(Ts[h], 1000 * h + k)))
        lone = [_lone(e, q) for e, q in zip(hs, qts)]
        assert len(set(lone[:40])) == 40  # (the poses differ: so do the results)
        rc, status, out = _batch(hs, qts)
        assert rc == sicp.OK and (status == 0).all()
        for k in range(120):
            assert bytes(out[k]) == lone[k], k
        # interleaved: the groups are other ones, the rows are not
        order = np.random.default_rng(7).permutation(120)
        rc, status, out = _batch([hs[i] for i in order], [qts[i] for i in order])
        assert rc == sicp.OK and (status == 0).all()
        for k, i in enumerate(order):
            assert bytes(out[k]) == lone[i], (k, i)
    finally:
        _close(es)


def test_a_batch_repeats_bit_for_bit():
    es, qts = [], []
    try:
        for mode, n, seed in ((E, 3000, 81), (G, 2000, 82), (S, 2500, 83), (E, 257, 84)):
            e, q = _lidar_engine(mode, n, seed)
            es.append(e); qts.append(q)
        _, s1, o1 = _batch(es, qts)
        _, s2, o2 = _batch(es, qts, fill=0xA5)
        assert (s1 == 0).all() and (s2 == 0).all()
        assert bytes(o1) == bytes(o2)
    finally:
        _close(es)
