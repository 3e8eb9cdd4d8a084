"""GPU tests of sicp_range_image / sicp_range_labels: every image, every per-point array and every count equals
tests/range_ref.py fed the tables sicp_range_tables hands back -- byte for byte -- at every shape, on the points that sit on
sector edges, row edges, the view's borders, the vertical axis and the range bounds, with points that are not finite, for the
winner's tie rules and every rule of the vote; the same bytes on every mode, slot and layout; a relabelled dst is the cloud
set_cloud of the same arrays would make; a call without dst leaves the handle as it was; every refusal leaves the outputs as
they were; a box room painted by its walls gets its walls back."""
import importlib

import numpy as np
import pytest

import np_ref
import range_cases
import range_ref as R
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
INV, NR, FEW = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS
PER_POINT = ("pixel", "visible")
ORIGIN = (5.3, 5.6, 1.3)  # a sensor inside the cloud of synth.config1_pair: its points surround it


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(c, **kw):
    return sicp.default_range_params(**dict(c["p"], **kw))


def _image(e, which, c, **kw):
    p = _params(c, **kw)
    return e.range_image(which, p, c["origin"], c["beam"]), p


def _ref_image(c, p):
    return R.image(c["xyz"], c["labels"], p, sicp.range_tables(p, c["beam"]), c["origin"])


def _same_image(out, ref):
    for k in R.COUNTS:
        print(k, out["info"][k], ref[k])
    for k in R.COUNTS:
        assert out["info"][k] == ref[k], k
    for k in R.IMAGES + PER_POINT:
        assert out[k].dtype == ref[k].dtype and out[k].shape == ref[k].shape, k
        diff = np.flatnonzero(out[k].reshape(-1).view(np.uint8) != ref[k].reshape(-1).view(np.uint8))
        print(k, "bytes that differ:", len(diff), diff[:8])
    for k in R.IMAGES + PER_POINT:
        assert out[k].tobytes() == ref[k].tobytes(), k
    assert out["range"].tobytes() == np.sqrt(ref["range_sq"]).tobytes()


def _run_image(c, mode=E, which=SRC, **kw):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return _image(e, which, c, **kw)


def _check_image(c, **kw):
    out, p = _run_image(c, **kw)
    ref = _ref_image(c, p)
    _same_image(out, ref)
    return out, ref


def _vote(e, which, c, pixel_label, **kw):
    p = _params(c, **kw)
    return e.range_labels(which, pixel_label, p, c["origin"], c["beam"]), p


def _same_vote(out, ref):
    print("voted", out["info"]["n_voted"], ref["n_voted"], "unvoted", out["info"]["n_unvoted"], ref["n_unvoted"])
    for k in ("labels", "votes"):
        diff = np.flatnonzero(out[k] != ref[k])
        print(k, "entries that differ:", len(diff), diff[:8])
    assert out["labels"].dtype == np.uint32 and out["votes"].dtype == np.uint8
    assert out["labels"].tobytes() == ref["labels"].tobytes()
    assert out["votes"].tobytes() == ref["votes"].tobytes()
    assert out["info"]["n_voted"] == ref["n_voted"] and out["info"]["n_unvoted"] == ref["n_unvoted"]
    for k in R.COUNTS:
        assert out["info"][k] == ref["image"][k], k


def _check_vote(e, c, pixel_label, which=SRC, **kw):
    out, p = _vote(e, which, c, pixel_label, **kw)
    ref = R.vote(c["xyz"], c["labels"], pixel_label, p, sicp.range_tables(p, c["beam"]), c["origin"])
    _same_vote(out, ref)
    return out, ref


# ---- the projection -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(range_cases.SHAPES))
def test_every_shape_direction_and_shift(name):
    """one row, two rows, a width whose half and a height that are no powers of two, the largest tables in LDS; clockwise on and
    off; col_shift 0, 1, W / 2, W - 1"""
    c = range_cases.shape_case(name)
    W = c["p"]["width"]
    hit = set()
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        for clockwise in (0, 1):
            for shift in (0, 1, W // 2, W - 1):
                out, p = _image(e, SRC, c, clockwise=clockwise, col_shift=shift)
                ref = _ref_image(c, p)
                _same_image(out, ref)
                hit.add(out["index"].tobytes())
                assert ref["n_pixels_hit"] > 0 and 0 < ref["n_kept"] < len(c["xyz"]) and ref["n_outside_fov"] > 0
    assert len(hit) == 8
    assert out["info"]["t_total_ms"] > 0


def test_points_on_every_edge():
    """dy = 0 with dx > 0 and dx < 0, dx = 0, the diagonals at W = 8 m, the floats next to each; dz = 0 on a row edge at
    elevation 0; the top and bottom of the view; the vertical axis above and below; r2 equal to each bound"""
    for W, H in ((16, 2), (24, 4), (64, 6)):
        c = range_cases.edges_case(W, H)
        for clockwise in (0, 1):
            out, ref = _check_image(c, clockwise=clockwise)
        x = c["xyz"]
        i_min = np.flatnonzero((x == [0.5, 0, 0]).all(axis=1))[0]
        i_max = np.flatnonzero((x == [8, 0, 0]).all(axis=1))[0]
        assert out["pixel"][i_min] >= 0 and out["pixel"][i_max] == -1  # min_range is inside, max_range is not
        up, down = (np.flatnonzero((x == [0, 0, z]).all(axis=1))[0] for z in (5.0, -5.0))
        assert out["pixel"][up] == -1 and out["pixel"][down] == -1  # D = 0: above and below every view
        on_edge = np.flatnonzero((x[:, 2] == 0) & (out["pixel"] >= 0))
        assert len(on_edge) > 20 and (out["pixel"][on_edge] // W == H // 2 - 1).all()  # on an inner edge: the row above it
    c = range_cases.edges_origin_case()
    out, ref = _check_image(c)
    origin = np.flatnonzero((c["xyz"] == 0).all(axis=1))[0]
    assert out["pixel"][origin] >= 0 and out["visible"][origin] == 1


def test_point_sets():
    """one point; every point out of range; NaN / Inf points mixed in (with an origin and a beam table); no finite point"""
    out, ref = _check_image(range_cases.one_point_case())
    assert out["info"]["n_pixels_hit"] == 1 and out["visible"].tolist() == [1] and out["count"].sum() == 1
    out, ref = _check_image(range_cases.all_dropped_case())
    assert out["info"]["n_kept"] == 0 and (out["index"] == -1).all() and (out["pixel"] == -1).all() and not out["count"].any()
    c = range_cases.mixed_case()
    out, ref = _check_image(c)
    bad = ~np.isfinite(c["xyz"]).all(axis=1)
    assert bad.sum() == 5 and out["info"]["n_finite"] == len(bad) - 5
    assert (out["pixel"][bad] == -1).all() and not out["visible"][bad].any()
    nothing, _ = _check_image(range_cases.not_finite_only_case())
    assert nothing["info"]["n_finite"] == 0 and (nothing["index"] == -1).all()
    # without per-point outputs and without labels
    with _engine(G) as e:
        e.set_target(c["xyz"])
        p = _params(c)
        lean = e.range_image(TGT, p, c["origin"], c["beam"], per_point=False)
        assert "pixel" not in lean and not lean["label"].any()
        assert lean["index"].tobytes() == ref["index"].tobytes()


def test_the_winner():
    """duplicated points and points of equal r2 in one pixel: the smaller caller index; a nearer point that comes later wins"""
    c = range_cases.winner_case()
    out, ref = _check_image(c)
    assert out["visible"].tolist() == [1, 0, 0, 0, 0, 0, 1, 1, 0, 1, 0]
    assert sorted(out["index"][out["index"] >= 0].tolist()) == [0, 6, 7, 9]
    assert sorted(out["count"][out["count"] > 0].tolist()) == [2, 2, 3, 4]
    # the same with points that are not finite in front of them: the indices are the caller's
    shifted = range_cases.case(np.concatenate([np.full((2, 3), np.nan, np.float32), c["xyz"]]), np.concatenate([[9, 9], c["labels"]]), **c["p"])
    out, ref = _check_image(shifted)
    assert sorted(out["index"][out["index"] >= 0].tolist()) == [2, 8, 9, 11]
    c, near = range_cases.crowd_case()
    out, ref = _check_image(c)
    assert out["info"]["n_pixels_hit"] == 1 and out["count"].max() == 2000 and out["visible"].sum() == 1
    assert out["index"].max() == min(near, 1500) and out["visible"][min(near, 1500)] == 1


# ---- the vote -------------------------------------------------------------------------------------------------------------------
def test_the_image_own_labels_come_back():
    """S = 1, k = 1 with pixel_label = the image's own label: every visible point gets its label back, an occluded point its
    winner's iff within max_dist_sq"""
    c = range_cases.vote_case()
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        img, p = _image(e, SRC, c, window=1, k=1, max_dist_sq=4.0)
        out, ref = _check_vote(e, c, img["label"], window=1, k=1, max_dist_sq=4.0)
    vis = img["visible"] == 1
    assert (out["labels"][vis] == c["labels"][vis]).all() and (out["votes"][vis] == 1).all()
    occ = np.flatnonzero((img["pixel"] >= 0) & ~vis)
    w = img["index"].reshape(-1)[img["pixel"][occ]]
    e3 = c["xyz"][occ] - c["xyz"][w]
    d2 = (e3[:, 0] * e3[:, 0] + e3[:, 1] * e3[:, 1]) + e3[:, 2] * e3[:, 2]
    near = d2.astype(np.float64) < 4.0
    assert near.sum() > 50 and (~near).sum() > 50
    assert (out["labels"][occ[near]] == c["labels"][w[near]]).all() and (out["votes"][occ[near]] == 1).all()
    assert (out["labels"][occ[~near]] == c["labels"][occ[~near]]).all() and (out["votes"][occ[~near]] == 0).all()
    gone = img["pixel"] < 0
    assert gone.sum() > 0 and (out["labels"][gone] == c["labels"][gone]).all() and not out["votes"][gone].any()


@pytest.mark.parametrize("window", [1, 3, 5, 7])
def test_every_window_and_k(window):
    """S = 1, 3, 5, 7 with k = 1, 5, 16 (and the list lengths between: 2, 3, 4, 8, 9) on a picture of classes 0 .. 3: k larger than
    the candidates, windows across the column seam and at rows 0 and H - 1, neighbours all of class 0, ties everywhere"""
    c = range_cases.vote_case()
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        for k in (1, 2, 3, 4, 5, 8, 9, 16):
            out, ref = _check_vote(e, c, c["pixel_label"], window=window, k=k)
            inview = ref["image"]["pixel"] >= 0
            assert (ref["neighbours"][inview] < k).any() or window * window > k  # k exceeds what a window holds at S = 1, 3
            assert ((out["votes"] == 0) & inview).any() and (out["votes"] > 0).any()
        # the seam and the border rows were voted over
        W, H = c["p"]["width"], c["p"]["height"]
        col, row = ref["image"]["pixel"] % W, ref["image"]["pixel"] // W
        for sel in (col == 0, col == W - 1, row == 0, row == H - 1):
            assert (inview & sel & (out["votes"] > 0)).any()


def test_a_beam_table_an_origin_and_points_that_are_not_finite():
    c = range_cases.mixed_case()
    rng = np.random.default_rng(3)
    pl = rng.integers(0, 5, (7, 40)).astype(np.uint32)
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        out, ref = _check_vote(e, c, pl, window=3, k=5, max_dist_sq=25.0)
    bad = ~np.isfinite(c["xyz"]).all(axis=1)
    assert not out["labels"][bad].any() and not out["votes"][bad].any()


@pytest.mark.parametrize("clockwise", [0, 1])
def test_ties_of_distance_and_of_votes(clockwise):
    """P alone in its pixel, A one column to one side and B two columns to the other, across the seam, both at d2 = 10 exactly"""
    c = range_cases.tie_case(clockwise)
    with _engine() as e:
        e.set_source(c["xyz"], c["labels"])
        img, p = _image(e, SRC, c)
        pix = img["pixel"]
        W = 16
        assert pix.tolist() == ([15, 14, 1] if clockwise else [0, 1, 14])  # P on the seam's side, B beyond it
        pl = np.zeros((1, W), np.uint32)
        pl[0, pix[1]], pl[0, pix[2]] = 9, 7
        off = (pix - pix[0] + W // 2) % W - W // 2  # window columns of A and B: +-1 and -+2
        first = 9 if off[1] < off[2] else 7  # the class of the neighbour the window visits first
        assert first == (9 if clockwise else 7)
        # k = 2: P (class 0) and the first visited of the two at equal d2
        out, ref = _check_vote(e, c, pl, k=2)
        assert (out["labels"][0], out["votes"][0]) == (first, 1)
        # k = 3: one vote each, the smaller label wins, whichever came first
        out, ref = _check_vote(e, c, pl, k=3)
        assert (out["labels"][0], out["votes"][0]) == (7, 1)
        assert (out["labels"][1], out["votes"][1]) == (9, 1) and (out["labels"][2], out["votes"][2]) == (7, 1)
        # d2 equal to max_dist_sq: excluded -- P is left with itself, of class 0, and keeps its label
        out, ref = _check_vote(e, c, pl, k=3, max_dist_sq=10.0)
        assert (out["labels"][0], out["votes"][0]) == (1, 0) and out["info"]["n_unvoted"] == 1
        out, ref = _check_vote(e, c, pl, k=3, max_dist_sq=float(np.nextafter(np.float32(10.0), np.float32(11.0))))
        assert (out["labels"][0], out["votes"][0]) == (7, 1)
        # all neighbours of class 0: rule 12
        out, ref = _check_vote(e, c, np.zeros((1, W), np.uint32), k=3)
        assert out["labels"].tolist() == [1, 2, 3] and not out["votes"].any() and out["info"]["n_voted"] == 0
        # infinity takes every occupied pixel of the window
        out, ref = _check_vote(e, c, pl, k=16, max_dist_sq=np.inf)
        assert out["votes"].tolist() == [1, 1, 1]


def test_a_cloud_without_labels():
    c = range_cases.vote_case(labelled=False)
    with _engine(G) as e:
        e.set_target(c["xyz"])
        out, ref = _check_vote(e, c, c["pixel_label"], which=TGT)
        assert (out["labels"][out["votes"] == 0] == 0).all() and (out["labels"] > 0).any()
        img, p = _image(e, TGT, c)
        assert not img["label"].any()


# ---- invariance -----------------------------------------------------------------------------------------------------------------
def _bytes(img, lab):
    return b"".join(img[k].tobytes() for k in R.IMAGES + PER_POINT) + lab["labels"].tobytes() + lab["votes"].tobytes() + \
        repr([img["info"][k] for k in R.COUNTS] + [lab["info"]["n_voted"], lab["info"]["n_unvoted"]]).encode()


def _both(e, which, c):
    img, p = _image(e, which, c)
    lab, _ = _vote(e, which, c, c["pixel_label"])
    return _bytes(img, lab)


def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


def test_the_same_bytes_on_every_mode_slot_and_layout_and_the_handle_is_untouched():
    c = range_cases.vote_case()
    c["xyz"][[3, 77]] = np.nan
    want = None
    for mode, which in ((E, SRC), (E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
        with _engine(mode) as e:
            e.set_cloud(which, c["xyz"], c["labels"])
            got = _both(e, which, c)
            assert got == _both(e, which, c)
        want = want or got
        assert got == want, (mode, which)
    # before and after an align() has put the clouds on the device in the mode's layout; what align() reads stays as it was
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    cs = dict(range_cases.case(src, sl, origin=ORIGIN, width=32, height=8, fov_up=1.2, fov_down=-1.2, max_range=60.0), pixel_label=None)
    cs["pixel_label"] = np.random.default_rng(8).integers(0, 4, (8, 32)).astype(np.uint32)
    want = None
    for mode in (E, S, G):
        res = []
        for with_calls in (False, True):
            with _engine(mode) as e, _engine(mode) as other:
                if mode != G:
                    e.set_confusion(synth.confusion_matrix(11))
                e.set_source(src, sl)
                e.set_target(tgt, tl)
                before = _both(e, SRC, cs) if with_calls else None
                first = e.align(qt)
                idx, d2, w = e.correspondences(qt)
                stats = e.stats()
                if with_calls:
                    after = _both(e, SRC, cs)
                    _vote(e, SRC, cs, cs["pixel_label"])
                    e.range_labels(TGT, cs["pixel_label"], _params(cs), dst=other, dst_which=SRC)
                    assert e.stats() == stats
                    i2, d22, w2 = e.correspondences(qt)
                    assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
                    want = want or before
                    assert before == want and after == want, mode
                second = e.align(qt)
                res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                            _drop_times(second[1])))
        assert res[0] == res[1], mode
    assert R.image(src, sl, R.params(**cs["p"]), R.tables(R.params(**cs["p"])), ORIGIN)["n_pixels_hit"] > 50


# ---- dst ------------------------------------------------------------------------------------------------------------------------
def _answers(e, qt):
    """what a handle says about its source: size, labels' effect on a registration, correspondences"""
    pose, st = e.align(qt)
    idx, d2, w = e.correspondences(qt)
    return e.cloud_size(SRC), idx.tobytes(), d2.tobytes(), w.tobytes(), pose.tobytes(), _drop_times(st)


@pytest.mark.parametrize("mode", [E, S])
def test_a_relabelled_dst_equals_set_cloud_of_the_same_arrays(mode):
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    src = src.copy()
    src[[5, 900], [0, 2]] = [np.nan, np.inf]
    c = range_cases.case(src, sl, origin=ORIGIN, width=32, height=8, fov_up=1.2, fov_down=-1.2, max_range=60.0, window=3, k=3, max_dist_sq=0.25)
    pl = np.random.default_rng(12).choice(np.array([0, 1, 2, 4], np.uint32), (8, 32))
    cm = synth.confusion_matrix(11)
    with _engine(mode) as host, _engine(mode) as other, _engine(mode) as holder, _engine(mode) as place:
        for e in (host, other, place):
            e.set_confusion(cm)
            e.set_target(tgt, tl)
        holder.set_source(src, sl)
        p = _params(c)
        out = holder.range_labels(SRC, pl, p, ORIGIN, dst=other, dst_which=SRC)  # into another handle
        ref = R.vote(src, sl, pl, p, sicp.range_tables(p), ORIGIN)
        _same_vote(out, ref)
        assert (ref["labels"] != sl).sum() > 100 and ref["n_voted"] > 500
        host.set_source(src, ref["labels"])
        want = _answers(host, qt)
        assert want[0] == (len(src), len(src) - 2)
        assert other.n[SRC] == len(src) and holder.cloud_size(SRC) == (len(src), len(src) - 2)
        assert _answers(other, qt) == want
        # the new labels are the slot's: a vote of class 0 everywhere hands them back
        again = other.range_labels(SRC, np.zeros((8, 32), np.uint32), p, ORIGIN)
        assert again["labels"].tobytes() == ref["labels"].tobytes() and not again["votes"].any()
        # in place, after an align() on the old labels
        place.set_source(src, sl)
        place.align(qt)
        out2 = place.range_labels(SRC, pl, p, ORIGIN, dst=place)
        assert out2["labels"].tobytes() == out["labels"].tobytes()
        assert _answers(place, qt) == want
        # from the target slot into the source slot of the same handle
        place.set_target(src, sl)
        place.range_labels(TGT, pl, p, ORIGIN, dst=place, dst_which=SRC)
        place.set_target(tgt, tl)
        assert _answers(place, qt) == want


def test_a_dst_from_a_cloud_without_labels_and_no_finite_point():
    c = range_cases.vote_case(labelled=False, n=600)
    with _engine(G) as e, _engine(E) as other, _engine(G) as nothing:
        e.set_source(c["xyz"])
        p = _params(c)
        out = e.range_labels(SRC, c["pixel_label"], p, dst=other, dst_which=TGT)
        assert other.cloud_size(TGT) == (600, 600)
        back = other.range_labels(TGT, np.zeros_like(c["pixel_label"]), p)  # a labelled cloud now
        assert back["labels"].tobytes() == out["labels"].tobytes() and out["labels"].any()
        nothing.set_source(np.full((4, 3), np.nan, np.float32))
        with pytest.raises(sicp.SicpError) as err:
            nothing.range_labels(SRC, c["pixel_label"], p, dst=other, dst_which=TGT)
        assert err.value.status == FEW and "dst keeps its cloud" in sicp.lib().sicp_last_error(nothing._h).decode()
        assert other.cloud_size(TGT) == (600, 600)
        assert nothing.range_labels(SRC, c["pixel_label"], p)["info"]["n_unvoted"] == 4


# ---- refusals -------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """the C calls with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points, n_pixels):
        self.img = [np.full(4 * n_pixels, SENTINEL, np.uint8) for _ in range(7)]
        self.pt = [np.full(4 * n_points, SENTINEL, np.uint8) for _ in range(4)]
        self.info = sicp.SicpRangeInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    @staticmethod
    def _p(a, t):
        return None if a is None else a.ctypes.data_as(C.POINTER(t))

    def image(self, e, which, p, beam=None, origin=None):
        i = self.img
        return sicp.lib().sicp_range_image(None if e is None else e._h, which, None if p is None else C.byref(p), self._p(beam, C.c_double),
                                           self._p(origin, C.c_float), self._p(i[0], C.c_int32), self._p(i[1], C.c_float),
                                           self._p(i[2], C.c_float), self._p(i[3], C.c_float), self._p(i[4], C.c_float),
                                           self._p(i[5], C.c_uint32), self._p(i[6], C.c_uint32), self._p(self.pt[0], C.c_int32),
                                           self._p(self.pt[1], C.c_uint8), C.byref(self.info))

    def labels(self, e, which, p, pl, beam=None, origin=None, dst=None, dst_which=SRC):
        return sicp.lib().sicp_range_labels(None if e is None else e._h, which, None if p is None else C.byref(p), self._p(beam, C.c_double),
                                            self._p(origin, C.c_float), self._p(pl, C.c_uint32), None if dst is None else dst._h, dst_which,
                                            self._p(self.pt[2], C.c_uint32), self._p(self.pt[3], C.c_uint8), C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.img + self.pt) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = range_cases.vote_case(n=400, W=16, H=4)
    n, W, H = len(c["xyz"]), 16, 4
    pl = c["pixel_label"]
    good = dict(c["p"])
    down = np.array([0.1, 0.0, -0.2, -0.4])
    bad_params = [dict(width=17, col_shift=0), dict(width=14, col_shift=0), dict(height=0), dict(height=257), dict(fov_up=-0.1, fov_down=-0.1),
                  dict(fov_up=-0.5, fov_down=-0.1), dict(fov_up=np.pi / 2), dict(fov_down=-np.pi / 2), dict(fov_up=np.nan),
                  dict(min_range=-0.5), dict(max_range=0.25), dict(max_range=np.inf), dict(clockwise=2), dict(col_shift=16),
                  dict(col_shift=-1), dict(window=4), dict(window=9), dict(k=0), dict(k=17), dict(max_dist_sq=-1.0),
                  dict(max_dist_sq=np.nan)]
    with _engine() as e, _engine() as other, _engine() as empty:
        e.set_source(c["xyz"], c["labels"])
        other.set_source(c["xyz"][:100], c["labels"][:100])
        p = sicp.default_range_params(**good)
        before = _both(e, SRC, c)
        raw = _Raw(n, W * H)

        def refused(status, want=INV, holder=e, text="sicp_range"):
            assert status == want
            assert raw.untouched()
            if holder is not None:
                msg = sicp.lib().sicp_last_error(holder._h).decode()
                print(msg)
                assert text in msg
            assert other.cloud_size(SRC) == (100, 100)

        for kw in bad_params:
            q = sicp.default_range_params(**dict(good, **kw))
            refused(raw.image(e, SRC, q))
            refused(raw.labels(e, SRC, q, pl, dst=other))
        for beam in (down[::-1].copy(), np.array([0.1, 0.1, 0.0, -0.1]), np.array([0.1, np.nan, 0.0, -0.1]), np.array([1.5, 0.5, 0.0, -0.1])):
            refused(raw.image(e, SRC, p, beam=beam))
            refused(raw.labels(e, SRC, p, pl, beam=beam, dst=other))
        refused(raw.image(e, SRC, p, origin=np.array([0, np.inf, 0], np.float32)))
        refused(raw.labels(e, SRC, p, None, dst=other), text="pixel_label is NULL")
        refused(raw.image(e, SRC, None))
        refused(raw.labels(e, SRC, None, pl))
        for which in (-1, 2):
            refused(raw.image(e, which, p), text="which")
            refused(raw.labels(e, which, p, pl, dst=other), text="which")
            refused(raw.labels(e, SRC, p, pl, dst=other, dst_which=which), text="dst_which")
        refused(raw.image(e, TGT, p), want=NR, text="holds no cloud")
        refused(raw.labels(e, TGT, p, pl, dst=other), want=NR, text="holds no cloud")
        refused(raw.image(empty, SRC, p), want=NR, holder=empty, text="holds no cloud")
        refused(raw.image(None, SRC, p), holder=None)
        refused(raw.labels(None, SRC, p, pl), holder=None)
        # the calls go through with the same arguments, and the handle answers as before
        assert raw.image(e, SRC, p, beam=down) == sicp.OK and raw.labels(e, SRC, p, pl, beam=down) == sicp.OK
        assert not raw.untouched()
        assert _both(e, SRC, c) == before


# ---- a sanity case with meaning -------------------------------------------------------------------------------------------------
def test_a_box_room_gets_its_walls_back():
    """every pixel's class painted from the face its point lies on: range_labels gives every point its face's class wherever
    the point's window shows one class only, and the points it does not are those the restatement names -- all of them within
    one window of a corner"""
    c = range_cases.room_case()
    W, H = c["p"]["width"], c["p"]["height"]
    face = c["face"]
    with _engine(G) as e:
        e.set_source(c["xyz"])
        img, p = _image(e, SRC, c)
        assert img["info"]["n_pixels_hit"] == W * H and img["visible"].all()  # one ray per pixel, every ray in its own pixel
        assert (img["index"].reshape(-1) == np.arange(W * H)).all()
        pl = face[img["index"]]
        out, ref = _check_vote(e, c, pl)
    wrong = out["labels"] != face
    # pixels whose window shows a second class
    f2 = face.reshape(H, W)
    mixed = np.zeros((H, W), dtype=bool)
    for wr in range(-2, 3):
        for wc in range(-2, 3):
            rows = np.clip(np.arange(H) + wr, 0, H - 1)
            mixed |= np.roll(f2, -wc, axis=1)[rows] != f2
    expected = int((ref["labels"] != face).sum())
    print("points:", W * H, "near a corner:", int(mixed.sum()), "mislabelled:", int(wrong.sum()), "the restatement's:", expected)
    assert wrong.sum() == expected
    assert not (wrong & ~mixed.reshape(-1)).any()
    assert mixed.sum() < 0.25 * W * H and wrong.sum() < 0.5 * mixed.sum()
    assert (out["votes"][~mixed.reshape(-1)] >= 1).all() and out["info"]["n_unvoted"] == ref["n_unvoted"]
