"""GPU tests of sicp_segment_ground: the per-point arrays, the cell table and info equal tests/ground_ref.py exactly -- integers
equal, doubles bit-equal, NaN where the restatement has NaN -- on every case of tests/ground_cases.py, whatever the handle's
mode, slot and device layout; two calls give the same bytes; the call leaves the handle as it was; every refusal leaves the
outputs as they were; the capacity rule; dst is set_cloud of the selection; a memory-limit refusal leaves the handle usable; and
the recipe segment_ground(select = 1, dst) -> cluster on the sloped street without labels."""
import importlib

import numpy as np
import pytest

import cluster_ref
import ground_cases
import ground_ref
import np_ref
import plane_cases
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
INTS = ("ground", "cell", "status", "n_members", "n_ground", "n_fit")
DOUBLES = ("height", "normal", "centroid", "lambda_min", "lpr")
DTYPES = dict(ground=np.uint8, cell=np.int32, height=np.float64, status=np.uint8, n_members=np.int32, n_ground=np.int32, n_fit=np.int32,
              normal=np.float64, centroid=np.float64, lambda_min=np.float64, lpr=np.float64)
INV, NR, FEW, OOM = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS, sicp.ERR_OUT_OF_MEMORY


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(kw, **over):
    kw = dict(kw, **over)
    return sicp.default_ground_params(ignore=kw.pop("ignore"), **kw)


def _call(e, which, c, **kw):
    return e.segment_ground(which, _params(c["params"], **kw.pop("over", {})), c["mask"], c["origin"], c["ring_edge"], **kw)


def _run(c, mode=E, which=SRC):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return _call(e, which, c)


def _canon(a):
    """a double array's bytes with every NaN the same NaN"""
    a = np.array(a, np.float64)
    a[np.isnan(a)] = np.nan
    return a.tobytes()


def _same(out, ref):
    info = out["info"]
    for k in ground_ref.COUNTS:
        print(k, info[k], ref[k])
    print("n_ground", info["n_ground"], ref["n_ground_total"], "cells", info["cells"], ref["cells"])
    for k in ground_ref.COUNTS:
        assert info[k] == ref[k], k
    assert info["n_ground"] == ref["n_ground_total"] and info["cells"] == ref["cells"]
    for k in INTS + DOUBLES:
        assert out[k].dtype == DTYPES[k] and out[k].shape == ref[k].shape, k
    for k in INTS:
        assert out[k].tobytes() == ref[k].astype(DTYPES[k]).tobytes(), (k, np.flatnonzero(out[k] != ref[k])[:10])
    for k in DOUBLES:
        assert (np.isnan(out[k]) == np.isnan(ref[k])).all(), k
        assert _canon(out[k]) == _canon(ref[k]), (k, np.argwhere(~((out[k] == ref[k]) | np.isnan(ref[k])))[:10])


def _bytes(out):
    if "info" in out:
        counts = [int(out["info"][k]) for k in ground_ref.COUNTS] + [int(out["info"]["n_ground"])] + list(out["info"]["cells"])
    else:
        counts = [int(out[k]) for k in ground_ref.COUNTS] + [int(out["n_ground_total"])] + list(out["cells"])
    return b"".join(np.ascontiguousarray(out[k]).astype(DTYPES[k]).tobytes() for k in INTS) + b"".join(_canon(out[k]) for k in DOUBLES) + repr(counts).encode()


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ground_cases.NAMES)
def test_result_equals_the_restatement(name):
    """cells of 1 to 4 097 members around the wave width; n_lpr beyond the cell, at 1 and at 64; n_iter at 1 and 8; equal heights,
    degenerate Q, -0.0 beside +0.0; points on ring edges, sector boundaries and the origin; R x S at 1 x 4 and 64 x 256, a caller's
    ring table; points at th_dist, at lpr + th_seeds and at the max_below bound and an ulp either side; every status; the height's
    fallback; non-finite points, ignored labels with a mask, no labels; a sensor origin; no candidate at all; the sloped street; and
    262 145 + 4 097 points"""
    out = _run(ground_cases.case(name))
    _same(out, ground_cases.reference(name))
    assert out["info"]["t_total_ms"] > 0 and out["info"]["n_selected"] == 0


def test_the_tables_are_the_restatements():
    for kw, edge in ((dict(), None), (dict(n_rings=64, n_sectors=256, min_range=0.0, max_range=123.456), None),
                     (dict(n_rings=3, n_sectors=6, elevation_rings=1), np.array(ground_cases.RING_EDGE)),
                     (dict(n_rings=1, n_sectors=4, min_range=1.0, max_range=21.0, elevation_rings=0), None)):
        p = sicp.default_ground_params(**kw)
        got = sicp.ground_tables(p, edge)
        want = ground_ref.make_tables(p.n_rings, p.n_sectors, p.min_range, p.max_range, edge)
        for k in ("edge2", "cos_half", "sin_half"):
            assert got[k].tobytes() == want[k].tobytes(), (kw, k)


def test_the_same_bytes_on_every_mode_slot_and_layout():
    """a SEMANTIC handle groups the cloud by label: three interleaved labels, one of them on five points"""
    for name in ("interleaved", "nan_mix"):
        c = ground_cases.case(name)
        want = _bytes(ground_cases.reference(name))
        for mode, which in ((E, SRC), (E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
            assert _bytes(_run(c, mode, which)) == want, (name, mode, which)


def _pair():
    src, sl, tgt, tl, T = synth.config1_pair()
    return src, sl, tgt, tl, np_ref.mat_to_qt(T)


def _pair_setup(src):
    """a grid that suits whatever the pair's cloud is: the sensor over its middle, everything a candidate"""
    lo, hi = src.min(axis=0).astype(np.float64), src.max(axis=0).astype(np.float64)
    origin = np.array([(lo[0] + hi[0]) / 2, (lo[1] + hi[1]) / 2, hi[2]])
    reach = float(np.hypot(hi[0] - lo[0], hi[1] - lo[1]))
    kw = dict(ground_ref.DEFAULTS, n_rings=4, n_sectors=8, min_range=0.0, max_range=reach, sensor_height=float(hi[2] - lo[2]), elevation_rings=0,
              th_dist=0.05, th_seeds=0.1, ignore=(2,))
    return kw, origin


def test_a_laid_out_cloud_gives_the_same_bytes():
    """before and after an align() has put the clouds on the device in the mode's layout, on an EM and on a SEMANTIC handle"""
    src, sl, tgt, tl, qt = _pair()
    kw, origin = _pair_setup(src)
    ref = ground_ref.segment_ground(src, sl, None, origin, None, **kw)
    assert ref["cells"][ground_ref.GROUND] > 0 and 0 < ref["n_candidates"] < len(src)
    want = _bytes(ref)
    p = _params(kw)
    for mode in (E, S):
        with _engine(mode) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            assert _bytes(e.segment_ground(SRC, p, sensor_origin=origin)) == want, mode
            e.align(qt)
            assert _bytes(e.segment_ground(SRC, p, sensor_origin=origin)) == want, mode
            assert e.segment_ground(TGT, p, sensor_origin=origin)["info"]["n_points"] == len(tgt)


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("street", "cell_sizes", "statuses"):
        c = ground_cases.case(name)
        with _engine(E) as e:
            e.set_source(c["xyz"], c["labels"])
            a = _bytes(_call(e, SRC, c))
            b = _bytes(_call(e, SRC, c))
        assert a == b == _bytes(_run(c)), name


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


def test_the_handle_is_untouched():
    src, sl, tgt, tl, qt = _pair()
    kw, origin = _pair_setup(src)
    p = _params(kw)
    res = []
    for with_ground in (False, True):
        with _engine(E) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            if with_ground:
                assert e.segment_ground(SRC, p, sensor_origin=origin)["info"]["n_candidates"] > 0  # before anything is on the device in a layout
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_ground:
                e.segment_ground(SRC, p, sensor_origin=origin)
                e.segment_ground(TGT, p, sensor_origin=origin)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            second = e.align(qt)
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                        _drop_times(second[1])))
    assert res[0] == res[1]


# ---- refusals and capacity ----------------------------------------------------------------------------------------------------
SENTINEL = 0x5A
WIDTH = dict(ground=1, cell=4, height=8, status=1, n_members=4, n_ground=4, n_fit=4, normal=24, centroid=24, lambda_min=8, lpr=8)


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points, capacity=16, tables=True):
        rows = max(capacity, 1)
        self.bufs = {k: np.full(w * (max(n_points, 1) if k in ground_ref.POINT_ARRAYS else rows), SENTINEL, np.uint8) for k, w in WIDTH.items()}
        self.out = sicp.SicpGroundOut()
        self.out.capacity = capacity
        types = dict(sicp.SicpGroundOut._fields_)
        for k, a in self.bufs.items():
            if tables or k in ground_ref.POINT_ARRAYS:
                setattr(self.out, k, a.ctypes.data_as(types[k]))
        self.info = sicp.SicpGroundInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, e, which, params, mask=None, origin=None, ring_edge=None, dst=None, dst_which=SRC):
        bp, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
        ptr = lambda a, t: None if a is None else np.ascontiguousarray(a).ctypes.data_as(t)  # noqa: E731
        self.keep = [None if a is None else np.ascontiguousarray(a) for a in (mask, origin, ring_edge)]
        return sicp.lib().sicp_segment_ground(None if e is None else e._h, which, None if params is None else C.byref(params),
                                              ptr(self.keep[0], bp), ptr(self.keep[1], dp), ptr(self.keep[2], dp),
                                              None if dst is None else dst._h, dst_which, C.byref(self.out), C.byref(self.info))

    def view(self, k):
        return self.bufs[k].view(DTYPES[k])

    def arrays_untouched(self):
        return all((a == SENTINEL).all() for a in self.bufs.values())

    def untouched(self):
        return self.arrays_untouched() and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = ground_cases.case("nan_mix")
    n = len(c["xyz"])
    small = ground_cases.SMALL

    def P(**kw):
        return sicp.default_ground_params(**dict(small, **kw))

    nan, inf = float("nan"), float("inf")
    many, neg = P(), P()
    many.n_ignore, neg.n_ignore = 17, -1
    none = np.zeros(n, np.uint8)
    doubles = ("min_range", "max_range", "sensor_height", "max_below", "th_seeds", "th_dist", "min_cos", "max_elevation", "max_thickness")
    with _engine(G) as a, _engine(G) as nolab, _engine(S) as sem_nolab, _engine(E) as other:
        a.set_source(c["xyz"], c["labels"])
        nolab.set_source(c["xyz"])
        sem_nolab.set_source(c["xyz"])
        other.set_source(c["xyz"][:40], c["labels"][:40])
        refused = [
            ("NULL handle", INV, (None, SRC, P())),
            ("NULL params", INV, (a, SRC, None)),
            ("which 2", INV, (a, 2, P())),
            ("which -1", INV, (a, -1, P())),
            ("dst_which 2", INV, (a, SRC, P(select=1), None, None, None, other, 2)),
            ("origin nan", INV, (a, SRC, P(), None, [0.0, nan, 0.0])),
            ("origin inf", INV, (a, SRC, P(), None, [inf, 0.0, 0.0])),
            *[(f"{k} nan", INV, (a, SRC, P(**{k: nan}))) for k in doubles],
            *[(f"{k} inf", INV, (a, SRC, P(**{k: inf}))) for k in doubles],
            ("min_range negative", INV, (a, SRC, P(min_range=-0.5))),
            ("max_range == min_range", INV, (a, SRC, P(min_range=3.0, max_range=3.0))),
            ("max_range < min_range", INV, (a, SRC, P(min_range=3.0, max_range=2.0))),
            ("ring_edge not ascending", INV, (a, SRC, P(), None, None, [1.0, 2.0, 2.0, 5.0, 9.0])),
            ("ring_edge descending", INV, (a, SRC, P(), None, None, [1.0, 2.0, 1.5, 5.0, 9.0])),
            ("ring_edge negative", INV, (a, SRC, P(), None, None, [-1.0, 2.0, 3.0, 5.0, 9.0])),
            ("ring_edge nan", INV, (a, SRC, P(), None, None, [1.0, 2.0, nan, 5.0, 9.0])),
            ("R 0", INV, (a, SRC, P(n_rings=0, elevation_rings=0))),
            ("R 65", INV, (a, SRC, P(n_rings=65))),
            ("S 2", INV, (a, SRC, P(n_sectors=2))),
            ("S 7", INV, (a, SRC, P(n_sectors=7))),
            ("S 258", INV, (a, SRC, P(n_sectors=258))),
            ("n_lpr 0", INV, (a, SRC, P(n_lpr=0))),
            ("n_lpr 65", INV, (a, SRC, P(n_lpr=65))),
            ("n_iter 0", INV, (a, SRC, P(n_iter=0))),
            ("n_iter 9", INV, (a, SRC, P(n_iter=9))),
            ("min_points 2", INV, (a, SRC, P(min_points=2))),
            ("min_cos 0", INV, (a, SRC, P(min_cos=0.0))),
            ("min_cos above 1", INV, (a, SRC, P(min_cos=1.0000001))),
            ("th_dist 0", INV, (a, SRC, P(th_dist=0.0))),
            ("th_seeds negative", INV, (a, SRC, P(th_seeds=-0.1))),
            ("max_thickness negative", INV, (a, SRC, P(max_thickness=-0.1))),
            ("elevation_rings -1", INV, (a, SRC, P(elevation_rings=-1))),
            ("elevation_rings R + 1", INV, (a, SRC, P(elevation_rings=5))),
            ("n_ignore 17", INV, (a, SRC, many)),
            ("n_ignore -1", INV, (a, SRC, neg)),
            ("no labels, a label ignored", INV, (nolab, SRC, P(ignore=(3,)))),
            ("select 3", INV, (a, SRC, P(select=3), None, None, None, other)),
            ("select -1", INV, (a, SRC, P(select=-1), None, None, None, other)),
            ("select without dst", INV, (a, SRC, P(select=1))),
            ("slot without a cloud", NR, (a, TGT, P())),
            ("SEMANTIC handle, cloud never uploaded", NR, (sem_nolab, SRC, P())),
            ("empty selection with dst", FEW, (a, SRC, P(select=2), none, None, None, other, SRC)),
        ]
        for what, code, args in refused:
            raw = _Raw(n)
            assert raw.call(*args) == code, what
            assert raw.untouched(), what
        raw = _Raw(n, capacity=-1)
        assert raw.call(a, SRC, P()) == INV and raw.untouched()
        assert other.cloud_size(SRC)[0] == 40  # (the empty selection left dst alone)
        # the accepted forms: a cloud without labels, min_cos = 1 exactly, dst with select = 0 left alone, no mask no candidates
        _same(nolab.segment_ground(SRC, P()), ground_ref.segment_ground(c["xyz"], None, None, None, None, **dict(ground_ref.DEFAULTS, **small)))
        assert a.segment_ground(SRC, P(min_cos=1.0))["info"]["n_cells"] == 16
        assert a.segment_ground(SRC, P(), dst=other)["info"]["n_selected"] == 0 and other.cloud_size(SRC)[0] == 40
        empty = a.segment_ground(SRC, P(), none)
        assert empty["info"]["n_candidates"] == 0 and empty["info"]["cells"] == [16, 0, 0, 0, 0, 0] and not empty["ground"].any()
        # a raw call that succeeds writes everything
        raw = _Raw(n)
        assert raw.call(a, SRC, _params(c["params"])) == sicp.OK
        ref = ground_cases.reference("nan_mix")
        for k in INTS:
            assert raw.view(k).tobytes() == ref[k].astype(DTYPES[k]).tobytes(), k
        for k in DOUBLES:
            assert _canon(raw.view(k)) == _canon(ref[k].ravel()), k
        assert raw.info.n_ground == ref["n_ground_total"] and raw.info.n_cells == 16


def test_capacity_follows_the_cluster_rule():
    c = ground_cases.case("nan_mix")
    ref = ground_cases.reference("nan_mix")
    n = len(c["xyz"])
    p = _params(c["params"])
    with _engine(E) as e, _engine(E) as other:
        e.set_source(c["xyz"], c["labels"])
        other.set_source(c["xyz"][:40], c["labels"][:40])
        # too small with cell arrays: info written, nothing else -- not dst either
        raw = _Raw(n, capacity=15)
        assert raw.call(e, SRC, _params(c["params"], select=1), dst=other) == INV
        assert raw.arrays_untouched() and raw.info.n_cells == 16 and raw.info.n_ground == ref["n_ground_total"] and raw.info.n_selected == 0
        assert "16 cells" in sicp.lib().sicp_last_error(e._h).decode() and other.cloud_size(SRC)[0] == 40
        # no cell arrays: capacity plays no part
        raw = _Raw(n, capacity=0, tables=False)
        assert raw.call(e, SRC, p) == sicp.OK
        assert raw.view("ground").tobytes() == ref["ground"].tobytes() and _canon(raw.view("height")) == _canon(ref["height"])
        assert (raw.bufs["status"] == SENTINEL).all()
        # exactly enough
        raw = _Raw(n, capacity=16)
        assert raw.call(e, SRC, p) == sicp.OK
        assert raw.view("status").tobytes() == ref["status"].tobytes() and raw.view("n_fit").tolist() == ref["n_fit"].tolist()


# ---- dst ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("select", (1, 2))
def test_dst_is_set_cloud_of_the_selection(select):
    """into another handle and in place (after an align() has laid the cloud out): the slot answers segment_ground -- with a
    label ignored, so the labels count -- and cluster as a handle does that was handed the selected points"""
    c = ground_cases.case("nan_mix")
    ref = ground_cases.run_reference(c, select=select)
    sel = ref["selected"]
    assert 0 < len(sel) < ref["n_finite"]
    again = dict(c["params"], ignore=(2,))
    want = ground_ref.segment_ground(c["xyz"][sel], c["labels"][sel], None, None, None, **again)
    cp = sicp.default_cluster_params(tolerance=0.5, min_points=3)
    with _engine(S) as host, _engine(S) as holder, _engine(S) as other, _engine(E) as place:
        host.set_target(c["xyz"][sel], c["labels"][sel])
        want_clusters = host.cluster(TGT, cp)
        holder.set_source(c["xyz"], c["labels"])
        out = _call(holder, SRC, c, over=dict(select=select), dst=other, dst_which=TGT)
        _same(out, ref)
        assert out["info"]["n_selected"] == len(sel) == other.n[TGT]
        assert other.cloud_size(TGT) == (len(sel), len(sel)) and holder.cloud_size(SRC) == (len(c["xyz"]), ref["n_finite"])
        _same(other.segment_ground(TGT, _params(again)), want)
        got = other.cluster(TGT, cp)
        assert got["cluster_id"].tobytes() == want_clusters["cluster_id"].tobytes()
        # in place
        place.set_confusion(synth.confusion_matrix(11))
        place.set_source(c["xyz"], c["labels"])
        place.set_target(c["xyz"], c["labels"])
        place.align(np.array([0, 0, 0, 1, 0, 0, 0], np.float64))
        out = _call(place, SRC, c, over=dict(select=select), dst=place)
        _same(out, ref)
        assert place.cloud_size(SRC) == (len(sel), len(sel)) and place.cloud_size(TGT)[0] == len(c["xyz"])
        _same(place.segment_ground(SRC, _params(again)), want)


def test_a_memory_limit_refusal_leaves_the_handle_usable():
    """no new slab is allowed while the call needs scratch for 266 K points: refused -> nothing written and the next call
    answers; granted (the arena happened to have room) -> the answer"""
    c = ground_cases.case("big")
    ref = ground_cases.reference("big")
    n = len(c["xyz"])
    p = _params(c["params"])
    with _engine(G) as e:
        e.set_source(c["xyz"])
        raw = _Raw(n, capacity=512)
        sicp.set_memory_limit(0, max(sicp.memory_reserved(0), 1))
        try:
            st = raw.call(e, SRC, p)
        finally:
            sicp.set_memory_limit(0, 0)
        assert st in (sicp.OK, OOM)
        if st == OOM:
            assert raw.untouched() and e.cloud_size(SRC)[0] == n
        _same(e.segment_ground(SRC, p), ref)


# ---- the recipe ---------------------------------------------------------------------------------------------------------------
def test_removing_the_ground_separates_the_objects_of_a_sloped_street():
    """INTEGRATION.md, "Ground of a cloud": segment_ground(select = 1, dst = other) -> other.cluster separates what stands on a
    street that one plane cannot hold; the heights are the restatement's"""
    xyz, truth = ground_cases.sloped_street()
    c = ground_cases.case("street")
    ref = ground_cases.run_reference(c, select=1)
    rest = xyz[ref["selected"]]
    parts = cluster_ref.cluster(rest, None, **plane_cases.RECIPE_CLUSTER)
    print("ground removed:", parts["n_clusters"], "clusters, the largest of", parts["max_cluster_points"], "of", len(rest))
    assert parts["n_clusters"] > 1 and parts["max_cluster_points"] < 0.4 * len(rest)
    cp = sicp.default_cluster_params(**{k: v for k, v in plane_cases.RECIPE_CLUSTER.items() if k != "ignore"})
    with _engine(G) as e, _engine(G) as other:
        e.set_source(xyz)
        out = _call(e, SRC, c, over=dict(select=1), dst=other, dst_which=SRC)
        _same(out, ref)
        ground = out["ground"] != 0
        assert (ground & truth).sum() >= 0.95 * truth.sum() and (ground & truth).sum() >= 0.95 * ground.sum()
        assert out["info"]["n_selected"] == len(rest)
        got = other.cluster(SRC, cp)
        assert (got["info"]["n_clusters"], got["info"]["max_cluster_points"]) == (parts["n_clusters"], parts["max_cluster_points"])
        assert got["count"].tolist() == parts["count"].tolist()
