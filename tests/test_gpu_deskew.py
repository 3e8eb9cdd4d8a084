"""GPU tests of sicp_deskew: the points and the counts equal tests/deskew_ref.py fed the table the call hands back -- integers
equal, floats bit-equal -- on every case of tests/deskew_cases.py, whatever the handle's mode, slot and device layout; the table
equals the numpy composition within a few ulps; a deskewed dst is the cloud set_cloud of the moved arrays would make; a call without
dst leaves the handle as it was; every refusal leaves the outputs as they were; a scan skewed by a known twist comes back."""
import importlib

import numpy as np
import pytest

import deskew_cases
import deskew_ref as R
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
INV, NR, FEW = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _deskew(e, which, c, **kw):
    return e.deskew(which, c["times"], c["knot_time"], c["knot_qt"], c["ref_qt"], **kw)


def _run(c, mode=E, which=SRC):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return _deskew(e, which, c)


def _same(out, ref):
    for k in R.COUNTS:
        print(k, out["info"][k], ref[k])
    for k in R.COUNTS:
        assert out["info"][k] == ref[k], k
    assert out["points"].dtype == np.float32 and out["points"].shape == ref["points"].shape
    diff = np.flatnonzero((out["points"].view(np.uint32) != ref["points"].view(np.uint32)).any(axis=1))
    print("points that differ:", len(diff), diff[:8])
    assert out["points"].tobytes() == ref["points"].tobytes()


def _bytes(out):
    return out["points"].tobytes() + out["knots"].tobytes() + repr([out["info"][k] for k in R.COUNTS]).encode()


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", deskew_cases.NAMES)
def test_result_equals_the_restatement(name):
    """1, 63, 64, 65 and 257 points and one workgroup and one point past the largest launch; 2, 3, 33 and 1024 knots; times sorted,
    shuffled, all equal, on the first, an interior and the last knot, below and above the range, NaN and infinite; points that are
    not finite; equal consecutive knots; raw quaternions that change sign; a half-turn; the three kinds of ref_qt; no labels"""
    c = deskew_cases.case(name)
    out = _run(c)
    _same(out, deskew_cases.reference(name, out["knots"]))
    assert out["info"]["t_total_ms"] > 0


@pytest.mark.parametrize("name", ["n257", "knots1024", "sign_flip", "half_turn", "ref_knot", "ref_unrelated"])
def test_the_knot_table_equals_the_numpy_composition(name):
    """K_k = ref^-1 T_k: two quaternion scalings, an inverse and a product -- a quaternion component is a sum of four products of
    numbers <= 1 (error <= 4 eps) renormalised to first order (2 eps more), a translation component a 3 x 3 rotation (each entry a
    few eps) times a vector of the pose's magnitude M plus a vector of that magnitude: about a dozen roundings of numbers <= 2 M
    in a row, twice (inverse, product).  48 eps max(1, M) covers it with room; a wrong order or sign is off by O(1)."""
    c = deskew_cases.case(name)
    out = _run(c)
    want = R.compose_knots(c["knot_qt"], c["ref_qt"])
    M = max(1.0, np.abs(c["knot_qt"][:, 4:]).max(), 0.0 if c["ref_qt"] is None else np.abs(c["ref_qt"][4:]).max())
    err = np.abs(out["knots"] - want).max()
    print("pose magnitude", M, "largest difference", err, "in eps M", err / (np.finfo(np.float64).eps * M))
    assert err <= 48 * np.finfo(np.float64).eps * M
    assert ((out["knots"][1:, :4] * out["knots"][:-1, :4]).sum(axis=1) >= 0).all()


def test_twist_knots_equal_the_definition():
    rng = np.random.default_rng(11)
    for nk in (2, 3, 33, 1024):
        delta = R.se3_exp(rng.normal(size=6) * [2, 2, 2, 0.3, 0.3, 0.3])
        kt, kq = sicp.deskew_twist_knots(delta, 3.0, 3.1, nk)
        wt, wq = R.twist_knots(delta, 3.0, 3.1, nk)
        assert kt.tobytes() == wt.tobytes()  # (t0 + s (t1 - t0): two roundings, no libm)
        assert np.abs(kq - wq).max() < 1e-13, nk
    kt, kq = sicp.deskew_twist_knots(delta, 0.0, 1.0)
    assert len(kt) == 33 and kq.shape == (33, 7)
    bad = delta.copy()
    bad[:4] *= 1.001
    nan = delta.copy()
    nan[5] = np.nan
    for args in ((bad, 0.0, 1.0, 33), (nan, 0.0, 1.0, 33), (delta, 1.0, 1.0, 33), (delta, 2.0, 1.0, 33), (delta, 0.0, np.inf, 33),
                 (delta, 0.0, 1.0, 1), (delta, 0.0, 1.0, 1025)):
        with pytest.raises(sicp.SicpError) as err:
            sicp.deskew_twist_knots(*args)
        assert err.value.status == INV


def _labelled_pair():
    src, sl, tgt, tl, T = synth.config1_pair()
    return src, sl, tgt, tl, np_ref.mat_to_qt(T)


def _scan_case(n, seed=3, nk=33):
    """times and a trajectory for a cloud of n points"""
    rng = np.random.default_rng(seed)
    kt, kq = deskew_cases.trajectory(nk, deskew_cases.CAR, seed)
    return dict(times=np.sort(rng.uniform(deskew_cases.T0, deskew_cases.T1, n)), knot_time=kt, knot_qt=kq, ref_qt=None)


def test_the_same_bytes_on_every_mode_slot_and_layout():
    c = deskew_cases.case("bad_points")
    want = None
    for mode, which in ((E, SRC), (E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
        got = _bytes(_run(c, mode, which))
        want = want or got
        assert got == want, (mode, which)
    # before and after an align() has put the clouds on the device in the mode's layout
    src, sl, tgt, tl, qt = _labelled_pair()
    cs, ct = _scan_case(len(src)), _scan_case(len(tgt), 4)
    want = None
    for mode in (E, S, G):
        with _engine(mode) as e:
            if mode != G:
                e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            before = _bytes(_deskew(e, SRC, cs)), _bytes(_deskew(e, TGT, ct))
            e.align(qt)
            after = _bytes(_deskew(e, SRC, cs)), _bytes(_deskew(e, TGT, ct))
        want = want or before
        assert before == want and after == want, mode
    ref = R.deskew(src, cs["times"], cs["knot_time"], R.compose_knots(cs["knot_qt"]))
    assert ref["n_moved"] == len(src)


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("launch_shape", "shuffled", "bad_times"):
        c = deskew_cases.case(name)
        with _engine(E) as e:
            e.set_source(c["xyz"], c["labels"])
            a = _bytes(_deskew(e, SRC, c))
            b = _bytes(_deskew(e, SRC, c))
            assert _deskew(e, SRC, c, want_points=False)["points"] is None
        assert a == b == _bytes(_run(c)), name


# ---- dst ------------------------------------------------------------------------------------------------------------------------
def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


def _answers(e, qt):
    """what a handle says about its source: size, registration, correspondences"""
    pose, st = e.align(qt)
    idx, d2, w = e.correspondences(qt)
    return e.cloud_size(SRC), idx.tobytes(), d2.tobytes(), w.tobytes(), pose.tobytes(), _drop_times(st)


@pytest.mark.parametrize("mode", [E, S])
def test_a_deskewed_dst_equals_set_cloud_of_the_moved_arrays(mode):
    """with points that are not finite and times that are not: they leave the index exactly as set_cloud would leave them out"""
    src, sl, tgt, tl, qt = _labelled_pair()
    src = src.copy()
    src[[5, 900], [0, 2]] = [np.nan, np.inf]
    c = _scan_case(len(src))
    c["times"][[7, 1300]] = [np.nan, -np.inf]
    cm = synth.confusion_matrix(11)
    with _engine(mode) as host, _engine(mode) as other, _engine(mode) as holder, _engine(mode) as place:
        for e in (host, other, place):
            e.set_confusion(cm)
            e.set_target(tgt, tl)
        holder.set_source(src, sl)
        out = _deskew(holder, SRC, c, dst=other, dst_which=SRC)  # into another handle
        ref = R.deskew(src, c["times"], c["knot_time"], out["knots"])
        _same(out, ref)
        assert ref["n_moved"] == len(src) - 4 and ref["n_bad_time"] == 2
        host.set_source(ref["points"], sl)
        want = _answers(host, qt)
        assert want[0] == (len(src), len(src) - 4)
        assert other.n[SRC] == len(src) and holder.cloud_size(SRC) == (len(src), len(src) - 2)
        assert _answers(other, qt) == want
        # in place, after an align() on the skewed cloud
        place.set_source(src, sl)
        place.align(qt)
        again = _deskew(place, SRC, c, dst=place)
        assert _bytes(again) == _bytes(out)
        assert _answers(place, qt) == want
        # from the target slot into the source slot of the same handle
        place.set_target(src, sl)
        _deskew(place, TGT, c, dst=place, dst_which=SRC)
        place.set_target(tgt, tl)
        assert _answers(place, qt) == want


def test_a_dst_without_labels_and_no_moved_point():
    c = deskew_cases.case("no_labels")
    with _engine(G) as e, _engine(G) as other, _engine(G) as host:
        e.set_source(c["xyz"])
        other.set_target(c["xyz"][:50])
        out = _deskew(e, SRC, c, dst=other, dst_which=SRC)
        host.set_source(out["points"])
        host.set_target(c["xyz"][:50])
        assert other.cloud_size(SRC) == (200, 200)
        a, b = other.align(IDENT), host.align(IDENT)
        assert a[0].tobytes() == b[0].tobytes() and _drop_times(a[1]) == _drop_times(b[1])
        # every time is bad: nothing is left to index
        nowhen = dict(c, times=np.full(200, np.nan))
        with pytest.raises(sicp.SicpError) as err:
            _deskew(e, SRC, nowhen, dst=other, dst_which=TGT)
        assert err.value.status == FEW and "dst keeps its cloud" in sicp.lib().sicp_last_error(e._h).decode()
        assert other.cloud_size(TGT) == (50, 50)
        out = _deskew(e, SRC, nowhen)  # without dst a result like any other
        assert out["info"]["n_bad_time"] == 200 and (out["points"].view(np.uint32) == 0x7FC00000).all()


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def test_the_handle_is_untouched():
    src, sl, tgt, tl, qt = _labelled_pair()
    cs, ct = _scan_case(len(src)), _scan_case(len(tgt), 4)
    res = []
    for with_deskew in (False, True):
        with _engine(E) as e, _engine(E) as other:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            if with_deskew:
                assert _deskew(e, SRC, cs)["info"]["n_moved"] == len(src)  # before anything is on the device in a layout
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_deskew:
                _deskew(e, SRC, cs)
                _deskew(e, TGT, ct, dst=other, dst_which=SRC)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            second = e.align(qt)
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                        _drop_times(second[1])))
    assert res[0] == res[1]


# ---- refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points, n_knots):
        self.xyz = [np.full(4 * max(n_points, 1), SENTINEL, np.uint8) for _ in range(3)]
        self.knots = np.full(56 * max(n_knots, 1), SENTINEL, np.uint8)
        self.info = sicp.SicpDeskewInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, e, which, times, n_knots, kt, kq, ref=None, dst=None, dst_which=SRC):
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        ptr = lambda a: None if a is None else a.ctypes.data_as(dp)
        return sicp.lib().sicp_deskew(None if e is None else e._h, which, ptr(times), n_knots, ptr(kt), ptr(kq), ptr(ref),
                                      None if dst is None else dst._h, dst_which, *(a.ctypes.data_as(fp) for a in self.xyz),
                                      self.knots.ctypes.data_as(dp), C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.xyz + [self.knots]) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = deskew_cases.case("bad_points")
    n, nk = len(c["xyz"]), len(c["knot_time"])
    t, kt, kq = c["times"], c["knot_time"], c["knot_qt"]

    def changed(a, where, value):
        b = a.copy()
        b[where] = value
        return b

    long_kt, long_kq = deskew_cases.trajectory(1025, deskew_cases.CAR, 1)
    with _engine(G) as a, _engine(S) as sem_nolab, _engine(E) as other:
        a.set_source(c["xyz"], c["labels"])
        sem_nolab.set_source(c["xyz"])
        other.set_source(c["xyz"][:40], c["labels"][:40])
        refused = [
            ("NULL handle", INV, (None, SRC, t, nk, kt, kq)),
            ("NULL times", INV, (a, SRC, None, nk, kt, kq)),
            ("NULL knot_time", INV, (a, SRC, t, nk, None, kq)),
            ("NULL knot_qt", INV, (a, SRC, t, nk, kt, None)),
            ("which 2", INV, (a, 2, t, nk, kt, kq)),
            ("which -1", INV, (a, -1, t, nk, kt, kq)),
            ("dst_which 2", INV, (a, SRC, t, nk, kt, kq, None, other, 2)),
            ("dst_which -1", INV, (a, SRC, t, nk, kt, kq, None, other, -1)),
            ("one knot", INV, (a, SRC, t, 1, kt, kq)),
            ("no knot", INV, (a, SRC, t, 0, kt, kq)),
            ("1025 knots", INV, (a, SRC, t, 1025, long_kt, long_kq)),
            ("a knot time nan", INV, (a, SRC, t, nk, changed(kt, 4, np.nan), kq)),
            ("a knot time inf", INV, (a, SRC, t, nk, changed(kt, nk - 1, np.inf), kq)),
            ("knot times equal", INV, (a, SRC, t, nk, changed(kt, 4, kt[3]), kq)),
            ("knot times descending", INV, (a, SRC, t, nk, changed(kt, 4, kt[2]), kq)),
            ("a knot pose nan", INV, (a, SRC, t, nk, kt, changed(kq, (9, 5), np.nan))),
            ("a knot pose inf", INV, (a, SRC, t, nk, kt, changed(kq, (9, 1), np.inf))),
            ("a knot pose not unit", INV, (a, SRC, t, nk, kt, changed(kq, (0, slice(0, 4)), kq[0, :4] * (1 + 3e-6)))),
            ("a knot pose zero", INV, (a, SRC, t, nk, kt, changed(kq, (32, slice(0, 4)), 0.0))),
            ("ref nan", INV, (a, SRC, t, nk, kt, kq, changed(kq[3], 6, np.nan))),
            ("ref not unit", INV, (a, SRC, t, nk, kt, kq, changed(kq[3], slice(0, 4), kq[3, :4] * (1 - 3e-6)))),
            ("ref not unit, with dst", INV, (a, SRC, t, nk, kt, kq, changed(kq[3], slice(0, 4), kq[3, :4] * 2), other, SRC)),
            ("slot without a cloud", NR, (a, TGT, t, nk, kt, kq)),
            ("SEMANTIC handle, cloud never uploaded", NR, (sem_nolab, SRC, t, nk, kt, kq)),
            ("no moved point with dst", FEW, (a, SRC, np.full(n, np.nan), nk, kt, kq, None, other, SRC)),
        ]
        for what, code, args in refused:
            raw = _Raw(n, 1025)
            assert raw.call(*args) == code, what
            assert raw.untouched(), what
        assert other.cloud_size(SRC) == (40, int(np.isfinite(c["xyz"][:40]).all(axis=1).sum()))
        assert a.cloud_size(SRC) == (200, 194)
        # a quaternion within 1e-6 of unit is accepted and used normalised: the same table but for the scaling's last bit, which
        # the translations magnify by the pose's magnitude (the bound of test_the_knot_table_equals_the_numpy_composition)
        near = changed(kq, (slice(None), slice(0, 4)), kq[:, :4] * (1 + 5e-7))
        exact = _deskew(a, SRC, c)
        assert np.abs(a.deskew(SRC, t, kt, near)["knots"] - exact["knots"]).max() <= 48 * np.finfo(np.float64).eps * np.abs(kq[:, 4:]).max()
        # a raw call that succeeds writes everything
        raw = _Raw(n, nk)
        assert raw.call(a, SRC, t, nk, kt, kq) == sicp.OK
        got = np.stack([v.view(np.float32) for v in raw.xyz], axis=1)
        assert got.tobytes() == exact["points"].tobytes() and raw.knots.view(np.float64).tobytes() == exact["knots"].tobytes()
        assert raw.info.n_moved == 192 and raw.info.n_points == 200 and raw.info.t_total_ms > 0


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_a_scan_skewed_by_a_known_twist_comes_back():
    """the street scan of tests/synth.py as the sensor at rest at t1 would see it; the raw scan of a sensor moving at a constant
    twist measured the same physical points at their own times: p_raw = T(t)^-1 T(t1) p.  Deskewed with the knots of that twist
    it matches the unskewed scan within the header's bound for 33 knots -- |p| (sqrt(3) / 432) Theta^3 (1 + Theta^2) +
    (L / 2) tan(Theta / 4) with Theta and L of one interval -- plus the float32 roundings: the raw scan's (half an ulp of each
    of its coordinates, turned: at most sqrt(3) / 2 ulp of the largest) and the result's (half an ulp)."""
    src, sl, tgt, tl, T, cm = synth.lidar_pair(n_points=6000, n_az=300)
    clean = tgt.astype(np.float64)
    n, nk = len(clean), 33
    xi = np.array([3.0, 0.1, 0.02, 0.005, -0.01, 0.1])  # 30 m/s, 1 rad/s over 0.1 s
    t0, t1 = 7.0, 7.1
    az = np.arctan2(clean[:, 1], clean[:, 0])
    s = (az + np.pi) / (2 * np.pi)  # the revolution: firing time by azimuth
    times = t0 + s * (t1 - t0)
    delta = R.se3_exp(xi)
    raw = np.empty_like(clean)
    for i in range(n):
        M = R.mul(R.inverse(R.se3_exp((times[i] - t0) / (t1 - t0) * xi)), delta)
        raw[i] = R._rot(M[:4]) @ clean[i] + M[4:]
    raw32 = raw.astype(np.float32)
    skew = np.linalg.norm(raw32 - tgt, axis=1)
    assert skew.max() > 2.0  # metres at road speed
    kt, kq = sicp.deskew_twist_knots(delta, t0, t1, nk)
    with _engine(E) as e, _engine(E) as fixed:
        e.set_confusion(cm)
        e.set_target(tgt, tl)
        e.set_source(raw32, tl)
        skewed = e.evaluate(IDENT, 1.0)
        out = e.deskew(SRC, times, kt, kq, dst=fixed, dst_which=SRC)
        fixed.set_confusion(cm)
        fixed.set_target(tgt, tl)
        deskewed = fixed.evaluate(IDENT, 1.0)
    theta, L = np.linalg.norm(xi[3:]) / (nk - 1), np.linalg.norm(R.se3_exp(xi / (nk - 1))[4:])
    far = np.abs(raw32).max()
    bound = np.linalg.norm(raw, axis=1) * np.sqrt(3) / 432 * theta**3 * (1 + theta**2) + 0.5 * L * np.tan(theta / 4)
    ulps = (np.sqrt(3) / 2 + 0.5) * np.spacing(np.float32(far)).astype(np.float64)
    err = np.abs(out["points"].astype(np.float64) - clean).max(axis=1)
    print("skew max", skew.max(), "error max", err.max(), "bound max", (bound + ulps).max(), "worst error / bound", (err / (bound + ulps)).max())
    print("inlier rmse skewed", skewed["inlier_rmse"], "deskewed", deskewed["inlier_rmse"], "inliers", skewed["inliers"], deskewed["inliers"])
    assert out["info"]["n_moved"] == n and out["info"]["n_clamped_lo"] == 0 and out["info"]["n_clamped_hi"] == 0
    assert (err <= bound + ulps).all()
    assert deskewed["inlier_rmse"] < skewed["inlier_rmse"] and deskewed["inliers"] == n
