"""GPU tests of sicp_bootstrap_batch: many pairs in one call give, pair by pair, the bits of sicp_bootstrap on a fresh
handle -- with mixed sizes and motions, shared clouds, failing pairs among good ones, scoring cut into several chunks --
refusals write nothing, the poses feed align_batch, and kitti_eval_headless -B writes them as its init rows."""
import ctypes as C
import importlib
import subprocess

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import synth
from test_host_shims import build_example, write_pcd

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])


def _mat(qt):
    T = np.eye(4)
    T[:3, :3] = Rotation.from_quat(qt[:4]).as_matrix()
    T[:3, 3] = qt[4:]
    return T


def _delta(A, B):
    D = np.linalg.inv(A) @ B
    return np.degrees(np.linalg.norm(Rotation.from_matrix(D[:3, :3]).as_rotvec())), np.linalg.norm(D[:3, 3])


_pairs = {}


def _pair(n, seed, motion):
    key = (n, seed, motion)
    if key not in _pairs:
        src, _, tgt, _, T, _ = synth.lidar_pair(seed=seed, n_points=n, motion=motion)
        _pairs[key] = (src, tgt, T)
    return _pairs[key]


def _engine(src=None, tgt=None, mode=sicp.MODE_GICP):
    e = sicp.Engine(0, sicp.default_params(mode))
    if src is not None:
        e.set_source(src)
    if tgt is not None:
        e.set_target(tgt)
    return e


def _lone(src, tgt, params=None):
    with _engine(src, tgt) as e:
        return e.bootstrap(params)


INFO_KEYS = ("n_source_keypoints", "n_target_keypoints", "max_neighbours", "best_iteration")


def _same(batch_item, lone):
    st, qt, info = batch_item
    lq, li = lone
    assert st == sicp.OK
    assert np.array_equal(qt.view(np.uint64), lq.view(np.uint64)), (qt, lq)
    for k in INFO_KEYS:
        assert info[k] == li[k], k
    assert np.float64(info["best_error"]).view(np.uint64) == np.float64(li["best_error"]).view(np.uint64)


MIXED = [(20000, 3, (1.0, 2.0)), (50000, 4, (2.0, 30.0)), (100000, 3, (4.0, 120.0)), (20000, 6, (3.0, 60.0)),
         (50000, 7, (1.0, 10.0)), (100000, 8, (2.0, 5.0))]


def test_mixed_batch_is_bit_identical_to_lone_calls():
    data = [_pair(*m) for m in MIXED]
    lone = [_lone(s, t) for s, t, _ in data]
    es = [_engine(s, t, mode) for (s, t, _), mode in zip(data, (sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_GICP) * 2)]
    try:
        res = sicp.bootstrap_batch(es)
        for r, l in zip(res, lone):
            _same(r, l)
        # the stage times are the batch's, the same in every info
        assert len({r[2]["t_total_ms"] for r in res}) == 1
        # a batch of one is the lone call; the same handle twice in one batch
        _same(sicp.bootstrap_batch([es[2]])[0], lone[2])
        twice = sicp.bootstrap_batch([es[0], es[0]])
        _same(twice[0], lone[0]); _same(twice[1], lone[0])
    finally:
        for e in es:
            e.close()


def test_shared_clouds_give_the_bits_of_separate_uploads():
    scans, _, _ = synth.lidar_sequence(seed=5, n_scans=5, n_points=20000, step=(1.0, 20.0))
    shared, separate = [], []
    try:
        for i in range(4):  # pair i: scan i + 1 onto scan i
            e = _engine()
            if i == 0:
                e.set_target(scans[0][0])
            else:
                e.share_cloud(sicp.TARGET, shared[i - 1], sicp.SOURCE)
            e.set_source(scans[i + 1][0])
            shared.append(e)
            separate.append(_engine(scans[i + 1][0], scans[i][0]))
        a = sicp.bootstrap_batch(shared)
        b = sicp.bootstrap_batch(separate)
        for i, (ra, rb) in enumerate(zip(a, b)):
            _same(ra, (rb[1], rb[2]))
        _same(a[1], _lone(scans[2][0], scans[1][0]))
    finally:
        for e in shared + separate:
            e.close()


def test_failing_pairs_do_not_stop_the_others_and_change_nothing():
    good = [_pair(20000, 3, (1.0, 2.0)), _pair(20000, 6, (3.0, 60.0))]
    tiny = np.array([[0, 0, 0], [0.1, 0, 0], [40, 40, 40]], np.float32)
    tgt = good[0][1]
    # a source with one point far out on the negative side (the box filter is signed): its voxel grid overflows int32
    wide = np.concatenate([good[1][0], np.array([[-4e5, -4e5, -4e5]], np.float32)])
    es = [_engine(*good[0][:2]), _engine(tiny, tgt), _engine(None, tgt), _engine(*good[1][:2]), _engine(wide, tgt)]
    try:
        res = sicp.bootstrap_batch(es)
        assert [r[0] for r in res] == [sicp.OK, sicp.ERR_TOO_FEW_POINTS, sicp.ERR_NOT_READY, sicp.OK, sicp.ERR_INVALID_ARGUMENT]
        assert res[4][1] is None and "pair 4" in res[4][2]["error"] and "overflows int32" in res[4][2]["error"]
        assert res[1][1] is None and "pair 1" in res[1][2]["error"]
        assert res[2][1] is None and "pair 2" in res[2][2]["error"]
        _same(res[0], _lone(*good[0][:2]))
        _same(res[3], _lone(*good[1][:2]))
        # the C call answers the first failing pair's code, with per-pair statuses
        p = sicp.default_bootstrap_params()
        out = np.empty((5, 7))
        st = np.zeros(5, dtype=np.int32)
        rc = sicp.lib().sicp_bootstrap_batch(sicp._handles(es), 5, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)),
                                             st.ctypes.data_as(C.POINTER(C.c_int32)), None)
        assert rc == sicp.ERR_TOO_FEW_POINTS and list(st) == [r[0] for r in res]
        # nothing on any handle changed: align() gives the bits of a fresh handle
        es[2].set_source(good[0][0])
        for e, (s, t) in zip((es[0], es[2], es[3]), ((good[0][0], good[0][1]), (good[0][0], tgt), (good[1][0], good[1][1]))):
            with _engine(s, t) as f:
                qa, sa = e.align(IDENT)
                qf, sf = f.align(IDENT)
            assert np.array_equal(qa, qf) and sa["outer_iters"] == sf["outer_iters"]
    finally:
        for e in es:
            e.close()


def test_refusals_write_nothing():
    src, tgt, _ = _pair(20000, 3, (1.0, 2.0))
    with _engine(src, tgt) as e, _engine(src, tgt) as fresh:
        hs = (C.c_void_p * 2)(e._h.value, None)
        for n, handles, p in ((0, hs, sicp.default_bootstrap_params()), (2, hs, sicp.default_bootstrap_params()),
                              (1, hs, sicp.default_bootstrap_params(nr_samples=2))):
            out = np.full((2, 7), 5.0)
            st = np.full(2, 42, dtype=np.int32)
            rc = sicp.lib().sicp_bootstrap_batch(handles, n, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_double)),
                                                 st.ctypes.data_as(C.POINTER(C.c_int32)), None)
            assert rc == sicp.ERR_INVALID_ARGUMENT
            assert (out == 5.0).all() and (st == 42).all()
        assert "nr_samples" in sicp.lib().sicp_last_error(e._h).decode()
        with pytest.raises(sicp.SicpError) as ex:
            sicp.bootstrap_batch([e], sicp.default_bootstrap_params(nr_samples=2))
        assert ex.value.status == sicp.ERR_INVALID_ARGUMENT
        qa, sa = e.align(IDENT)
        qf, sf = fresh.align(IDENT)
    assert np.array_equal(qa, qf) and sa["outer_iters"] == sf["outer_iters"]


def test_scoring_in_several_chunks_is_bit_identical():
    # 40 pairs x 2000 hypotheses x ~1-2K source keypoints: well over the 32 Mi search outputs of one chunk
    p = sicp.default_bootstrap_params(max_iterations=2000)
    distinct = [_pair(5000, 10 + i, (1.0 + 0.5 * i, 15.0 * i)) for i in range(8)]
    lone = [_lone(s, t, p) for s, t, _ in distinct]
    es = [_engine(*distinct[i % 8][:2]) for i in range(40)]
    try:
        nq = sum(l[1]["n_source_keypoints"] for l in lone) * 5
        assert nq * 2000 > 32 * 2 ** 20
        res = sicp.bootstrap_batch(es, p)
        for i, r in enumerate(res):
            _same(r, lone[i % 8])
    finally:
        for e in es:
            e.close()


def test_batch_poses_feed_align_batch():
    data = [_pair(20000, 3, (4.0, yaw)) for yaw in (60.0, 120.0, 180.0)]
    es = [_engine(s, t) for s, t, _ in data]
    try:
        res = sicp.bootstrap_batch(es)
        inits = []
        for (st, qb, info), (_, _, T) in zip(res, data):
            assert st == sicp.OK
            rot, tr = _delta(T, _mat(qb))
            assert rot < 5.0 and tr < 1.0, (rot, tr, info)
            inits.append(qb)
        aligned = sicp.align_batch(es, np.array(inits))
        for (qa, _), e, (_, _, T) in zip(aligned, es, data):
            qg = np.r_[Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3]]
            qr, _ = e.align(qg)
            rot, tr = _delta(_mat(qr), _mat(qa))
            assert np.radians(rot) < 1e-4 and tr < 1e-3
    finally:
        for e in es:
            e.close()


def test_kitti_eval_headless_bootstrap_rows(tmp_path):
    exe = build_example(tmp_path, "kitti_eval_headless")
    # 40 deg of yaw and 4/3 m per scan: 120 deg between the scans of a stride-3 pair
    scans, poses, cm = synth.lidar_sequence(seed=5, n_scans=7, n_points=20000, step=(4.0 / 3.0, 40.0))
    d = tmp_path / "seq"
    d.mkdir()
    for k, (p, l) in enumerate(scans):
        write_pcd(str(d / f"{k:06d}.pcd"), p, l, binary=True)
    gt = str(tmp_path / "poses.txt")
    np.savetxt(gt, poses[:, :3, :].reshape(len(scans), 12), fmt="%.17g")
    cmf = str(tmp_path / "cm.txt")
    np.savetxt(cmf, cm, fmt="%.17g")

    def rows(prefix, name):
        return [[float(v) for v in line.split(",")] for line in open(prefix + name) if line.strip()]

    plain, boot = str(tmp_path / "plain_"), str(tmp_path / "boot_")
    for prefix, extra in ((plain, []), (boot, ["-B"])):
        r = subprocess.run([exe, "-s", str(d), "-t", gt, "-m", cmf, "-o", prefix] + extra, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
    init = rows(boot, "initkitti.csv")
    assert [(int(r[0]), int(r[1])) for r in init] == [(0, 3), (3, 6)]
    for r in init:
        a, b = int(r[0]), int(r[1])
        qt, _ = _lone(scans[b][0], scans[a][0])
        assert np.allclose(np.array(r[22:38]).reshape(4, 4), _mat(qt), rtol=0, atol=1e-12)
        assert int(r[38]) == 0
    em_plain, em_boot = rows(plain, "EMICPkitti.csv"), rows(boot, "EMICPkitti.csv")
    assert max(r[2] for r in em_plain) > 1e-2  # from the identity, 120 deg is out of reach
    assert max(r[2] for r in em_boot) < 1e-4
    # -b 2: the same init rows from one batch of two
    boot2 = str(tmp_path / "boot2_")
    r = subprocess.run([exe, "-s", str(d), "-t", gt, "-m", cmf, "-o", boot2, "-B", "-b", "2"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    for name in ("initkitti.csv", "EMICPkitti.csv", "se3GICPkitti.csv"):
        one = [line.split(",") for line in open(boot + name) if line.strip()]
        two = [line.split(",") for line in open(boot2 + name) if line.strip()]
        assert len(one) == len(two)
        for ra, rb in zip(one, two):
            assert ra[:5] == rb[:5] and ra[6:] == rb[6:]
