"""GPU tests of sicp_camera_image / sicp_camera_labels / sicp_camera_unproject: every image, every per-point array, every point of
an unprojected frame and every count equals tests/camera_ref.py fed the matrices sicp_camera_matrices hands back -- byte for
byte -- on seeded clouds, on the points that sit on pixel edges, the image's borders, the depth bounds and the view gate, with
points and depths that are not finite, for the winner's tie rule, every window and both depth types; the same bytes on every
mode, slot and layout; a dst is the cloud set_cloud of the same arrays would make; two cameras in place are the restatement
twice; a call without dst leaves the handle as it was; every refusal leaves the outputs as they were."""
import importlib

import numpy as np
import pytest

import camera_cases
import camera_ref as R
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
INV, NR, FEW = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(c, **kw):
    return sicp.default_camera_params(**dict(c["p"], **kw))


def _same(name, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    diff = np.flatnonzero(got.reshape(-1).view(np.uint8) != want.reshape(-1).view(np.uint8))
    print(name, "bytes that differ:", len(diff), diff[:8])
    return len(diff) == 0


def _same_image(out, ref):
    for k in R.COUNTS:
        print(k, out["info"][k], ref[k])
    ok = [_same(k, out[k], ref[k]) for k in R.IMAGES + R.PER_POINT]
    for k in R.COUNTS:
        assert out["info"][k] == ref[k], k
    assert all(ok), [k for k, o in zip(R.IMAGES + R.PER_POINT, ok) if not o]


def _same_labels(out, ref):
    for k in R.LABEL_COUNTS:
        print(k, out["info"][k], ref[k])
    ok = _same("labels", out["labels"], ref["labels"]), _same("state", out["state"], ref["state"])
    for k in R.LABEL_COUNTS:
        assert out["info"][k] == ref[k], k
    for k in R.COUNTS:
        assert out["info"][k] == ref["image"][k], k
    assert all(ok)


def _check_both(e, which, c, **kw):
    """image and labels of the cloud in the slot against the restatement"""
    p = _params(c, **kw)
    mat = sicp.camera_matrices(c["qt"])
    img = e.camera_image(which, p, c["qt"], per_point=True)
    ref_i = R.image(c["xyz"], c["labels"], p, mat)
    _same_image(img, ref_i)
    lab = e.camera_labels(which, c["pixel_label"], p, c["qt"])
    ref_l = R.labels(c["xyz"], c["labels"], c["pixel_label"], p, mat)
    _same_labels(lab, ref_l)
    return img, lab, ref_i, ref_l


# ---- byte equality --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(camera_cases.RANDOM))
def test_seeded_clouds(name):
    """16 x 12, 64 x 48 and 9 x 8 pixels, 2 000 - 20 000 points (more than one workgroup, no multiple of one), with and without a
    lens and a pose, NaN / Inf points mixed in, windows 1, 3, 5 and 15"""
    c = camera_cases.random_case(name)
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert ref_i["n_pixels_hit"] > 50 and 0 < ref_i["n_kept"] < ref_i["n_finite"] < len(c["xyz"]) and ref_i["n_outside"] > 0
        assert min(ref_l["n_labelled"], ref_l["n_occluded"], ref_l["n_unclassed"]) > 0
        assert img["info"]["t_total_ms"] > 0
        lean = e.camera_image(SRC, _params(c), c["qt"])
        assert "pixel" not in lean and lean["index"].tobytes() == ref_i["index"].tobytes()


@pytest.mark.parametrize("window", [1, 3, 5, 7, 9, 11, 13, 15])
def test_every_window(window):
    c = camera_cases.random_case("w16h12_lens_pose")
    with _engine(G) as e:
        e.set_target(c["xyz"], c["labels"])
        _check_both(e, TGT, c, window=window)


def test_points_on_pixel_edges_borders_and_bounds():
    c, want = camera_cases.edges_case()
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
    assert img["pixel"].tolist() == want.tolist()


def test_the_winner():
    c = camera_cases.winner_case()
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert img["visible"].tolist() == [0, 0, 0, 1, 0, 1, 0, 0] and img["index"][6, 8] == 3 and img["index"][6, 3] == 5
        c = camera_cases.crowd_case()
        e.set_source(c["xyz"], c["labels"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert img["count"].max() == 3000 and img["visible"].sum() == 1 and lab["info"]["n_occluded"] > 1000


def test_two_walls_and_a_cloud_without_labels():
    c, wall = camera_cases.walls_case()
    with _engine(G) as e:
        e.set_source(c["xyz"], c["labels"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert lab["info"]["n_occluded"] > 200 and (lab["labels"][lab["state"] == 2] == 2).all()
        e.set_source(c["xyz"])
        c["labels"] = None
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert not img["label"].any() and (lab["labels"][lab["state"] != 1] == 0).all() and (lab["labels"][lab["state"] == 1] == 7).all()
    c = camera_cases.case(np.full((5, 3), np.nan, np.float32), None, **camera_cases.EDGE_P)
    with _engine(G) as e:
        e.set_source(c["xyz"])
        img, lab, ref_i, ref_l = _check_both(e, SRC, c)
        assert img["info"]["n_finite"] == 0 and (img["index"] == -1).all() and np.isnan(img["u"]).all()


@pytest.mark.parametrize("name", list(camera_cases.FRAMES))
def test_depth_frames(name):
    """uint16 with 0 and 65535, float with NaN / Inf / negative / zero, both depth bounds; 0, 1, 20 and 64 iterations; with and without
    lens and pose; 9 x 8, 16 x 12, 64 x 48 and one 640 x 480 frame"""
    f = camera_cases.frame_case(name)
    p = sicp.default_camera_params(**f["p"])
    ref = R.unproject(f["depth"], p, sicp.camera_matrices(f["qt"]))
    with _engine(G) as e:
        out = e.camera_unproject(f["depth"], p, f["qt"])
    print("valid", out["info"]["n_valid"], ref["n_valid"])
    ok = _same("xyz", out["xyz"], ref["xyz"]), _same("valid", out["valid"], ref["valid"])
    assert all(ok)
    assert out["info"]["n_valid"] == ref["n_valid"] and out["info"]["n_points"] == f["depth"].size
    assert 0 < ref["n_valid"] < f["depth"].size


# ---- invariance -----------------------------------------------------------------------------------------------------------------
def _bytes(e, which, c):
    p = _params(c)
    img = e.camera_image(which, p, c["qt"], per_point=True)
    lab = e.camera_labels(which, c["pixel_label"], p, c["qt"])
    return b"".join(img[k].tobytes() for k in R.IMAGES + R.PER_POINT) + lab["labels"].tobytes() + lab["state"].tobytes() + \
        repr([img["info"][k] for k in R.COUNTS] + [lab["info"][k] for k in R.LABEL_COUNTS]).encode()


def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


HALF = np.sqrt(0.5)
LOOK_Y = np.array([-HALF, 0, 0, HALF, 5.3, 1.5, 1.5])  # at the edge of the cloud of synth.config1_pair, looking along +y through it
LOOK_X = np.array([0, HALF, 0, HALF, 1.5, 5.6, 1.2])   # a second camera looking along +x


def _street_case(src, sl, **kw):
    p = dict(width=32, height=24, fx=12.0, fy=12.0, cx=15.5, cy=11.5, max_depth=60.0, window=3, **kw)
    return camera_cases.case(src, sl, LOOK_Y, seed=9, **p)


def test_the_same_bytes_on_every_mode_and_slot():
    c = camera_cases.random_case("w64h48")
    want = None
    for mode, which in ((E, SRC), (E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
        with _engine(mode) as e:
            e.set_cloud(which, c["xyz"], c["labels"])
            got = _bytes(e, which, c)
            assert got == _bytes(e, which, c)
        want = want or got
        assert got == want, (mode, which)


@pytest.mark.parametrize("mode", [E, S, G])
def test_before_and_after_an_align_and_the_handle_is_untouched(mode):
    """the calls give the same bytes before and after an align() has laid the clouds out, and an align() after them returns what it
    returned without them"""
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    c = _street_case(src, sl)
    frame = camera_cases.frame_case("f32_w16h12_lens_pose")
    res = []
    for with_calls in (False, True):
        with _engine(mode) as e, _engine(mode) as other:
            if mode != G:
                e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            before = _bytes(e, SRC, c) if with_calls else None
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_calls:
                after = _bytes(e, SRC, c)
                assert before == after
                e.camera_labels(TGT, c["pixel_label"], _params(c), c["qt"], dst=other, dst_which=SRC)
                e.camera_unproject(frame["depth"], sicp.default_camera_params(**frame["p"]), frame["qt"])
                e.camera_unproject(frame["depth"], sicp.default_camera_params(**frame["p"]), frame["qt"], dst=other, dst_which=TGT)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            second = e.align(qt)
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                        _drop_times(second[1])))
    assert res[0] == res[1]
    ref = R.labels(src, sl, c["pixel_label"], R.params(**c["p"]), R.matrices(c["qt"]))
    assert ref["image"]["n_pixels_hit"] > 100 and ref["n_occluded"] > 50


# ---- dst ------------------------------------------------------------------------------------------------------------------------
def _answers(e, qt):
    """what a handle says about its source: size, the labels' effect on a registration, correspondences"""
    pose, st = e.align(qt)
    idx, d2, w = e.correspondences(qt)
    return e.cloud_size(SRC), idx.tobytes(), d2.tobytes(), w.tobytes(), pose.tobytes(), _drop_times(st)


@pytest.mark.parametrize("mode", [E, S])
def test_relabelled_dst_and_two_cameras_equal_set_cloud_of_the_restated_arrays(mode):
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    src = src.copy()
    src[[5, 900], [0, 2]] = [np.nan, np.inf]
    c = _street_case(src, sl)
    pl = np.random.default_rng(12).choice(np.array([0, 1, 2, 4], np.uint32), (24, 32))
    qt2 = LOOK_X  # the second camera, with another picture
    pl2 = np.random.default_rng(13).choice(np.array([0, 3, 5, 6], np.uint32), (24, 32))
    cm = synth.confusion_matrix(11)
    p = _params(c)
    rp = R.params(**c["p"])
    ref = R.labels(src, sl, pl, rp, sicp.camera_matrices(c["qt"]))
    ref2 = R.labels(src, ref["labels"], pl2, rp, sicp.camera_matrices(qt2))
    print("first camera:", ref["n_labelled"], ref["n_occluded"], "second:", ref2["n_labelled"], ref2["n_occluded"])
    assert ref["n_labelled"] > 100 and ref2["n_labelled"] > 100 and (ref["labels"] != sl).sum() > 100 and (ref2["labels"] != ref["labels"]).sum() > 100
    with _engine(mode) as host, _engine(mode) as other, _engine(mode) as holder, _engine(mode) as place:
        for e in (host, other, place):
            e.set_confusion(cm)
            e.set_target(tgt, tl)
        holder.set_source(src, sl)
        out = holder.camera_labels(SRC, pl, p, c["qt"], dst=other, dst_which=SRC)  # into another handle
        _same_labels(out, ref)
        host.set_source(src, ref["labels"])
        want = _answers(host, qt)
        assert want[0] == (len(src), len(src) - 2)
        assert other.n[SRC] == len(src) and holder.cloud_size(SRC) == (len(src), len(src) - 2)
        assert _answers(other, qt) == want
        # in place, after an align() on the old labels; then the second camera on top of the first
        place.set_source(src, sl)
        place.align(qt)
        out1 = place.camera_labels(SRC, pl, p, c["qt"], dst=place)
        assert out1["labels"].tobytes() == ref["labels"].tobytes()
        assert _answers(place, qt) == want
        out2 = place.camera_labels(SRC, pl2, p, qt2, dst=place)
        _same_labels(out2, ref2)
        host.set_source(src, ref2["labels"])
        assert _answers(place, qt) == _answers(host, qt)
        # the new labels are the slot's: a picture of class 0 hands them back
        again = place.camera_labels(SRC, np.zeros_like(pl), p, c["qt"])
        assert again["labels"].tobytes() == ref2["labels"].tobytes() and again["info"]["n_labelled"] == 0
        # from the target slot into the source slot of the same handle
        place.set_target(src, sl)
        place.camera_labels(TGT, pl, p, c["qt"], dst=place, dst_which=SRC)
        place.set_target(tgt, tl)
        host.set_source(src, ref["labels"])
        assert _answers(place, qt) == _answers(host, qt)


@pytest.mark.parametrize("mode,dtype", [(E, np.uint16), (S, np.float32)])
def test_unprojected_dst_equals_set_cloud_of_the_restated_arrays(mode, dtype):
    W, H = 64, 48
    p = sicp.default_camera_params(**dict(camera_cases.intrinsics(W, H), **camera_cases.LENS))
    depth = camera_cases.depth_u16(W, H, 3) if dtype == np.uint16 else camera_cases.depth_f32(W, H, 4)
    label = np.random.default_rng(6).integers(1, 6, (H, W)).astype(np.uint32)
    ref = R.unproject(depth, p, sicp.camera_matrices(camera_cases.QT))
    # the target: the frame's valid points, pushed a little
    ok = ref["valid"].reshape(-1).astype(bool)
    tgt, tl = ref["xyz"][ok] + np.float32(0.02), label.reshape(-1)[ok]
    qt = np.array([0, 0, 0, 1, 0.01, 0, 0], dtype=np.float64)
    cm = synth.confusion_matrix(11)
    with _engine(mode) as host, _engine(mode) as other, _engine(mode) as place:
        for e in (host, other, place):
            e.set_confusion(cm)
            e.set_target(tgt, tl)
        out = host.camera_unproject(depth, p, camera_cases.QT, label, dst=other, dst_which=SRC)  # into another handle
        assert out["xyz"].tobytes() == ref["xyz"].tobytes()
        assert other.n[SRC] == W * H and other.cloud_size(SRC) == (W * H, ref["n_valid"])
        host.set_source(ref["xyz"], label.reshape(-1))
        want = _answers(host, qt)
        assert want[0] == (W * H, ref["n_valid"])
        assert _answers(other, qt) == want
        # into the handle's own slot, over a cloud it has aligned; without reading the points back
        place.set_source(tgt, tl)
        place.align(qt)
        lean = place.camera_unproject(depth, p, camera_cases.QT, label, dst=place, dst_which=SRC, want_points=False)
        assert "xyz" not in lean and lean["info"]["n_valid"] == ref["n_valid"]
        assert _answers(place, qt) == want
    # without a label image the cloud has none
    with _engine(G) as host, _engine(G) as other:
        for e in (host, other):
            e.set_target(tgt)
        host.camera_unproject(depth, p, camera_cases.QT, dst=other, dst_which=SRC)
        host.set_source(ref["xyz"])
        assert _answers(other, qt) == _answers(host, qt)
        img = other.camera_image(SRC, p, camera_cases.QT)
        assert not img["label"].any() and img["info"]["n_pixels_hit"] > 0.5 * ref["n_valid"]


def test_no_finite_point_and_no_valid_pixel():
    c = camera_cases.random_case("w16h12")
    p = _params(c)
    with _engine(G) as e, _engine(G) as other, _engine(G) as nothing:
        other.set_target(c["xyz"][:600])
        nothing.set_source(np.full((4, 3), np.nan, np.float32))
        with pytest.raises(sicp.SicpError) as err:
            nothing.camera_labels(SRC, c["pixel_label"], p, dst=other, dst_which=TGT)
        assert err.value.status == FEW and "dst keeps its cloud" in sicp.lib().sicp_last_error(nothing._h).decode()
        assert nothing.camera_labels(SRC, c["pixel_label"], p)["info"]["n_finite"] == 0
        with pytest.raises(sicp.SicpError) as err:
            e.camera_unproject(np.zeros((12, 16), np.uint16), p, dst=other, dst_which=TGT)
        assert err.value.status == FEW and "dst keeps its cloud" in sicp.lib().sicp_last_error(e._h).decode()
        assert other.cloud_size(TGT) == (600, 600 - int((~np.isfinite(c["xyz"][:600]).all(axis=1)).sum()))
        out = e.camera_unproject(np.full((12, 16), np.nan, np.float32), p)
        assert out["info"]["n_valid"] == 0 and np.isnan(out["xyz"]).all() and not out["valid"].any()


def test_the_memory_limit_answers_as_a_status():
    """no new slab is allowed and a 2048 x 2048 frame needs 50 MB of scratch and, in dst, a cloud of 4 M points.  Granted (the arena
    happened to have room) -> dst holds the frame.  Refused -> a status; dst holds its old cloud when the call's scratch was
    refused, and what sicp_set_cloud of the frame leaves under the same limit -- the points staged -- when dst's own buffers were;
    either way both handles go on working, and with the limit lifted the same call goes through"""
    c = camera_cases.random_case("w16h12")
    W = H = 2048
    p = sicp.default_camera_params(**camera_cases.intrinsics(W, H))
    depth = np.full((H, W), 2000, np.uint16)
    small = camera_cases.frame_case("u16_w16h12")
    sp = sicp.default_camera_params(**small["p"])
    want = R.unproject(small["depth"], sp, sicp.camera_matrices(None))
    with _engine(G) as e, _engine(G) as other:
        other.set_source(c["xyz"][:600])
        size = other.cloud_size(SRC)
        sicp.set_memory_limit(0, max(sicp.memory_reserved(0), 1))
        try:
            e.camera_unproject(depth, p, dst=other, dst_which=SRC, want_points=False)
            status = sicp.OK
        except sicp.SicpError as err:
            status = err.status
        finally:
            sicp.set_memory_limit(0, 0)
        print("status", status, "dst", other.cloud_size(SRC), "before", size)
        assert status in (sicp.OK, sicp.ERR_OUT_OF_MEMORY)
        if status == sicp.OK:
            assert other.cloud_size(SRC) == (W * H, W * H)
        else:
            assert other.cloud_size(SRC) in (size, (W * H, W * H))
            assert sicp.lib().sicp_last_error(e._h).decode() != ""
        # smaller work goes on, on both handles
        out = e.camera_unproject(small["depth"], sp, dst=other, dst_which=SRC)
        assert out["xyz"].tobytes() == want["xyz"].tobytes() and other.cloud_size(SRC) == (small["depth"].size, want["n_valid"])
        # and with the limit lifted the frame goes through
        e.camera_unproject(depth, p, dst=other, dst_which=SRC, want_points=False)
        assert other.cloud_size(SRC) == (W * H, W * H)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """the C calls with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points, n_pixels):
        self.img = [np.full(4 * n_pixels, SENTINEL, np.uint8) for _ in range(7)]
        self.pt = [np.full(4 * n_points, SENTINEL, np.uint8) for _ in range(6)]
        self.un = [np.full(4 * n_pixels, SENTINEL, np.uint8) for _ in range(4)]
        self.info = sicp.SicpCameraInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    @staticmethod
    def _p(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))

    def image(self, e, which, p, qt=None):
        i, t = self.img, self.pt
        return sicp.lib().sicp_camera_image(None if e is None else e._h, which, None if p is None else C.byref(p), self._p(qt, C.c_double),
                                            self._p(i[0], C.c_int32), self._p(i[1], C.c_float), self._p(i[2], C.c_float),
                                            self._p(i[3], C.c_float), self._p(i[4], C.c_float), self._p(i[5], C.c_uint32),
                                            self._p(i[6], C.c_uint32), self._p(t[0], C.c_int32), self._p(t[1], C.c_float),
                                            self._p(t[2], C.c_float), self._p(t[3], C.c_uint8), C.byref(self.info))

    def labels(self, e, which, p, pl, qt=None, dst=None, dst_which=SRC):
        return sicp.lib().sicp_camera_labels(None if e is None else e._h, which, None if p is None else C.byref(p), self._p(qt, C.c_double),
                                             self._p(pl, C.c_uint32), None if dst is None else dst._h, dst_which,
                                             self._p(self.pt[4], C.c_uint32), self._p(self.pt[5], C.c_uint8), C.byref(self.info))

    def unproject(self, e, p, d16, df, qt=None, label=None, dst=None, dst_which=SRC):
        u = self.un
        return sicp.lib().sicp_camera_unproject(None if e is None else e._h, None if p is None else C.byref(p), self._p(qt, C.c_double),
                                                self._p(d16, C.c_uint16), self._p(df, C.c_float), self._p(label, C.c_uint32),
                                                None if dst is None else dst._h, dst_which, self._p(u[0], C.c_float),
                                                self._p(u[1], C.c_float), self._p(u[2], C.c_float), self._p(u[3], C.c_uint8),
                                                C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.img + self.pt + self.un) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = camera_cases.random_case("w16h12")
    n, W, H = len(c["xyz"]), 16, 12
    pl = c["pixel_label"]
    d16, df = camera_cases.depth_u16(W, H, 1), camera_cases.depth_f32(W, H, 2)
    good = dict(c["p"])
    bad_params = [dict(width=7), dict(width=4097), dict(height=7), dict(height=4097), dict(fx=0.0), dict(fy=-1.0), dict(fx=np.nan),
                  dict(fy=np.inf), dict(cx=np.nan), dict(cy=np.inf), dict(k1=np.nan), dict(k2=np.inf), dict(p1=np.nan), dict(p2=-np.inf),
                  dict(k3=np.nan), dict(min_depth=0.0), dict(min_depth=-1.0), dict(min_depth=np.nan), dict(max_depth=np.inf),
                  dict(max_depth=0.3), dict(max_depth=np.nan), dict(max_tan_sq=0.0), dict(max_tan_sq=np.nan), dict(depth_scale=0.0),
                  dict(depth_scale=np.nan), dict(undistort_iterations=-1), dict(undistort_iterations=65), dict(window=0), dict(window=4),
                  dict(window=17), dict(occlusion_abs=-0.1), dict(occlusion_abs=np.nan), dict(occlusion_rel=-0.1), dict(occlusion_rel=np.nan)]
    bad_qt = [np.array(q, dtype=np.float64) for q in ([0, 0, 0, 0, 1, 2, 3], [0, 0, 0, 1, np.nan, 0, 0], [np.inf, 0, 0, 1, 0, 0, 0])]
    with _engine() as e, _engine() as other, _engine() as empty:
        e.set_source(c["xyz"], c["labels"])
        other.set_source(c["xyz"][:100], c["labels"][:100])
        size = other.cloud_size(SRC)
        p = sicp.default_camera_params(**good)
        before = _bytes(e, SRC, c)
        raw = _Raw(n, W * H)

        def refused(status, want=INV, holder=e, text="sicp_camera"):
            assert status == want
            assert raw.untouched()
            if holder is not None:
                msg = sicp.lib().sicp_last_error(holder._h).decode()
                print(msg)
                assert text in msg
            assert other.cloud_size(SRC) == size

        for kw in bad_params:
            q = sicp.default_camera_params(**dict(good, **kw))
            refused(raw.image(e, SRC, q))
            refused(raw.labels(e, SRC, q, pl, dst=other))
            refused(raw.unproject(e, q, d16, None, dst=other))
        for qt in bad_qt:
            refused(raw.image(e, SRC, p, qt), text="camera_qt")
            refused(raw.labels(e, SRC, p, pl, qt, dst=other), text="camera_qt")
            refused(raw.unproject(e, p, None, df, qt, dst=other), text="camera_qt")
        refused(raw.labels(e, SRC, p, None, dst=other), text="pixel_label is NULL")
        refused(raw.unproject(e, p, d16, df, dst=other), text="exactly one")
        refused(raw.unproject(e, p, None, None, dst=other), text="exactly one")
        refused(raw.image(e, SRC, None))
        refused(raw.labels(e, SRC, None, pl))
        refused(raw.unproject(e, None, d16, None))
        for which in (-1, 2):
            refused(raw.image(e, which, p), text="which")
            refused(raw.labels(e, which, p, pl, dst=other), text="which")
            refused(raw.labels(e, SRC, p, pl, dst=other, dst_which=which), text="dst_which")
            refused(raw.unproject(e, p, d16, None, dst=other, dst_which=which), text="dst_which")
        refused(raw.image(e, TGT, p), want=NR, text="holds no cloud")
        refused(raw.labels(e, TGT, p, pl, dst=other), want=NR, text="holds no cloud")
        refused(raw.image(empty, SRC, p), want=NR, holder=empty, text="holds no cloud")
        refused(raw.image(None, SRC, p), holder=None)
        refused(raw.labels(None, SRC, p, pl), holder=None)
        refused(raw.unproject(None, p, d16, None), holder=None)
        refused(raw.unproject(e, p, np.zeros((H, W), np.uint16), None, dst=other), want=FEW, text="dst keeps its cloud")
        # the calls go through with the same arguments, and the handle answers as before; unproject needs no cloud
        assert raw.image(e, SRC, p, bad_qt[0] + [0, 0, 0, 1, 0, 0, 0]) == sicp.OK and raw.labels(e, SRC, p, pl) == sicp.OK
        assert raw.unproject(empty, p, d16, None) == sicp.OK
        assert not raw.untouched()
        assert _bytes(e, SRC, c) == before
