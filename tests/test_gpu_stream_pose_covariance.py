"""GPU tests of SICP_SUBMIT_POSE_COVARIANCE / sicp_stream_take_pose_covariance: a flagged registration of a stream hands back
the bytes sicp_pose_covariance gives on a lone handle at the registration's final pose, in all three modes, next to fused
labels and fresh features, with slots that are used again and with non-finite points; the registration itself (pose,
counters) is that of a lone align(); a take works once, only for flagged tickets, and a refused take keeps the entry."""
import ctypes
import importlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
COUNTERS = ("outer_iters", "total_lm_iters", "total_evals", "total_corr")
SS, ST = 0.01, 0.02

_seq = {}


def _scans(n_points):
    """seven consecutive scans of one drive (5000 points each), or their first 2000 points' worth, computed once"""
    if "full" not in _seq:
        _seq["full"], _, _seq["cm"] = synth.lidar_sequence(seed=5, n_scans=7, n_points=5000)
    if n_points == 5000:
        return _seq["full"], _seq["cm"]
    return [(np.ascontiguousarray(p[::2][:n_points]), np.ascontiguousarray(l[::2][:n_points])) for p, l in _seq["full"]], _seq["cm"]


def _params(mode):
    p = sicp.default_params(mode)
    p.num_classes = 11
    if mode == sicp.MODE_SEMANTIC:
        p.min_class_pts = 40
    return p


def _take_raw(S, ticket, ss=SS, st=ST, out=True):
    r = sicp.SicpPoseCovarianceResult()
    ctypes.memset(ctypes.byref(r), 0x5A, ctypes.sizeof(r))
    rc = sicp.lib().sicp_stream_take_pose_covariance(S._s, ticket, ss, st, ctypes.byref(r) if out else None)
    return rc, bytes(r), r


def _lone(mode, cm, src, tgt):
    """a fresh engine: align() from the identity, then the pose covariance at its result"""
    e = sicp.Engine(0, _params(mode))
    if mode == sicp.MODE_EM:
        e.set_confusion(cm)
    e.set_source(*src)
    e.set_target(*tgt)
    q, st = e.align(IDENT)
    r = sicp.SicpPoseCovarianceResult()
    qq = np.ascontiguousarray(q, dtype=np.float64)
    assert sicp.lib().sicp_pose_covariance(e._h, sicp._ptr(qq, sicp._dp), SS, ST, ctypes.byref(r)) == sicp.OK
    return e, q, st, bytes(r), r


def test_em_stream_with_mixed_flags_and_reused_slots():
    scans, cm = _scans(5000)
    cov_on = lambda k: k % 2 == 0
    lab_on = lambda k: k % 3 == 0
    with sicp.Stream(0, _params(sicp.MODE_EM), max_in_flight=4, confusion=cm) as S:
        ids = [S.add_cloud(*sc) for sc in scans]
        tickets = {}
        for k in range(6):
            t = S.submit(ids[k + 1], ids[k], IDENT, fused_labels=lab_on(k), fresh_features=k in (1, 4), pose_covariance=cov_on(k))
            tickets[t] = k
        got = S.drain()
        covs, labels = {}, {}
        for t, k in tickets.items():
            if lab_on(k):
                labels[k] = S.take_labels(t, len(scans[k + 1][0]))
            rc, raw, r = _take_raw(S, t)
            if cov_on(k):
                assert rc == sicp.OK, k
                covs[k] = (raw, r)
                assert _take_raw(S, t)[0] == sicp.ERR_NOT_READY  # once
            else:
                assert rc == sicp.ERR_NOT_READY, k  # not flagged
                assert raw == bytes([0x5A]) * len(raw)
    assert len(got) == 6
    for ticket, status, qt, st in got:
        assert status == sicp.OK
        k = tickets[ticket]
        e, q1, s1, want, _ = _lone(sicp.MODE_EM, cm, scans[k + 1], scans[k])
        with e:
            assert np.array_equal(qt, q1), k
            for key in COUNTERS:
                assert st[key] == s1[key], (k, key)
            if cov_on(k):
                assert covs[k][0] == want, k
                assert covs[k][1].positive_definite == 1 and covs[k][1].active > 0
            if lab_on(k):
                assert np.array_equal(labels[k], e.fused_labels(q1)), k


def test_take_right_after_the_poll_that_returned_the_registration():
    scans, cm = _scans(5000)
    with sicp.Stream(0, _params(sicp.MODE_EM), max_in_flight=2, confusion=cm) as S:
        a, b = S.add_cloud(*scans[0]), S.add_cloud(*scans[1])
        t = S.submit(b, a, IDENT, pose_covariance=True)
        got = S.poll(wait=1)
        assert [g[0] for g in got] == [t] and got[0][1] == sicp.OK
        r = S.take_pose_covariance(t, SS, ST)
        assert r["positive_definite"] and r["active"] > 0
        with pytest.raises(sicp.SicpError) as err:
            S.take_pose_covariance(t, SS, ST)
        assert err.value.status == sicp.ERR_NOT_READY
    e, _, _, _, want = _lone(sicp.MODE_EM, cm, scans[1], scans[0])
    with e:
        assert np.array_equal(r["covariance"], want.as_dict()["covariance"])


@pytest.mark.parametrize("mode", [sicp.MODE_GICP, sicp.MODE_SEMANTIC])
def test_gicp_and_semantic_streams(mode):
    scans, cm = _scans(2000)
    gicp = mode == sicp.MODE_GICP
    clouds = [(p, None) if gicp else (p, l) for p, l in scans]
    with sicp.Stream(0, _params(mode), max_in_flight=4) as S:
        ids = [S.add_cloud(*sc) for sc in clouds]
        tickets = {S.submit(ids[k + 1], ids[k], IDENT, pose_covariance=True): k for k in range(4)}
        got = S.drain()
        raws = {}
        for t, k in tickets.items():
            rc, raw, _ = _take_raw(S, t)
            assert rc == sicp.OK, k
            raws[k] = raw
    assert len(got) == 4
    for ticket, status, qt, st in got:
        assert status == sicp.OK
        k = tickets[ticket]
        e, q1, s1, want, r = _lone(mode, cm, clouds[k + 1], clouds[k])
        with e:
            assert np.array_equal(qt, q1), k
            for key in COUNTERS:
                assert st[key] == s1[key], (k, key)
            assert raws[k] == want, k
            assert r.active > 0


def test_non_finite_points_in_source_and_target():
    scans, cm = _scans(5000)
    bad = scans[1][0].copy()
    bad[::97] = np.nan
    three = [scans[0], (bad, scans[1][1]), scans[2]]
    with sicp.Stream(0, _params(sicp.MODE_EM), max_in_flight=2, confusion=cm) as S:
        ids = [S.add_cloud(*sc) for sc in three]
        tickets = {S.submit(ids[k + 1], ids[k], IDENT, pose_covariance=True): k for k in range(2)}  # the scan as source, then as target
        got = S.drain()
        taken = {k: _take_raw(S, t) for t, k in tickets.items()}
    assert len(got) == 2
    for ticket, status, qt, _ in got:
        k = tickets[ticket]
        e, q1, _, want, r = _lone(sicp.MODE_EM, cm, three[k + 1], three[k])
        with e:
            assert status == sicp.OK and np.array_equal(qt, q1), k
            rc, raw, mine = taken[k]
            assert rc == sicp.OK and raw == want, k
            assert mine.active == r.active > 0


def test_raw_flags_and_bad_take_arguments():
    scans, _ = _scans(2000)
    lib = sicp.lib()
    q = np.ascontiguousarray(IDENT)
    qp = q.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    with sicp.Stream(0, _params(sicp.MODE_GICP), max_in_flight=2) as S:
        a, b = S.add_cloud(scans[0][0]), S.add_cloud(scans[1][0])
        tk = ctypes.c_int64(0)
        for flags in (4, 16, 8 | 4, 8 | 16, 1 << 31):  # unknown bits stay refused
            assert lib.sicp_stream_submit_ex(S._s, b, a, qp, flags, ctypes.byref(tk)) == sicp.ERR_INVALID_ARGUMENT, flags
        assert lib.sicp_stream_submit_ex(S._s, b, a, qp, 8, ctypes.byref(tk)) == sicp.OK  # any mode
        got = S.drain()
        assert [(g[0], g[1]) for g in got] == [(tk.value, sicp.OK)]
        # a refused take writes nothing and keeps the entry
        for ss, st, out in ((-1.0, 1.0, True), (1.0, float("nan"), True), (float("inf"), 1.0, True), (1.0, 1.0, False)):
            rc, raw, _ = _take_raw(S, tk.value, ss, st, out)
            assert rc == sicp.ERR_INVALID_ARGUMENT, (ss, st, out)
            assert raw == bytes([0x5A]) * len(raw)
        rc, raw, r = _take_raw(S, tk.value)
        assert rc == sicp.OK and r.positive_definite == 1
        assert _take_raw(S, tk.value)[0] == sicp.ERR_NOT_READY
    e, _, _, want, _ = _lone(sicp.MODE_GICP, None, (scans[1][0], None), (scans[0][0], None))
    with e:
        assert raw == want
