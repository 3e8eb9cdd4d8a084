"""GPU tests of sicp_segment_planes: plane_id, the plane table and info equal tests/plane_ref.py exactly -- integers equal,
doubles bit-equal -- on every case of tests/plane_cases.py, whatever the handle's mode, slot and device layout; two calls give
the same bytes; the call leaves the handle as it was; every refusal leaves the outputs as they were; the capacity rule; and
the recipe plane_id -> filter(mask, dst) -> cluster on a street scan without labels."""
import importlib

import numpy as np
import pytest

import cluster_ref
import np_ref
import plane_cases
import plane_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
ARRAYS = ("plane_id", "coeff", "count", "hyp_index", "hyp_count", "centroid", "rms")
DTYPES = dict(plane_id=np.int32, coeff=np.float64, count=np.int32, hyp_index=np.int32, hyp_count=np.int32, centroid=np.float64, rms=np.float64)
COUNTS = ("n_points", "n_finite", "n_candidates", "n_assigned", "n_planes", "rounds", "n_invalid_hypotheses")
INV, NR, FEW = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(kw, **over):
    kw = dict(kw, **over)
    return sicp.default_plane_params(ignore=kw.pop("ignore"), axis=kw.pop("axis"), **kw)


def _run(c, mode=E, which=SRC):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return e.segment_planes(which, _params(c["params"]), c["mask"])


def _same(out, ref):
    for k in COUNTS:
        print(k, out["info"][k], ref[k])
    for k in ("count", "hyp_index", "hyp_count"):
        print(k, out[k].tolist(), ref[k].tolist())
    for k in COUNTS:
        assert out["info"][k] == ref[k], k
    for k in ARRAYS:
        assert out[k].dtype == DTYPES[k] and out[k].shape == ref[k].shape, k
        assert out[k].tobytes() == ref[k].tobytes(), (k, out[k], ref[k])


def _bytes(out):
    info = out["info"] if "info" in out else out
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ARRAYS) + repr([int(info[k]) for k in COUNTS]).encode()


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", plane_cases.NAMES)
def test_result_equals_the_restatement(name):
    """the street scan with and without refinement, free, about z and about y; the room corner whose fourth round stops at
    min_inliers; exactly three points; the score kernel's tile less one, exactly, plus one and several tiles with holes; H at 1,
    around the hypothesis group and at the maximum; clouds without a plane; the lattice where every hypothesis ties; a point at t
    and one ulp beyond; non-finite points; ignored labels with a mask; three interleaved labels; no labels"""
    out = _run(plane_cases.case(name))
    _same(out, plane_cases.reference(name))
    assert out["info"]["t_total_ms"] > 0


def test_the_same_bytes_on_every_mode_slot_and_layout():
    """a SEMANTIC handle groups the cloud by label: three interleaved labels, one of them on five points"""
    for name in ("interleaved", "nan_mix"):
        c = plane_cases.case(name)
        want = _bytes(plane_cases.reference(name))
        for mode, which in ((E, SRC), (E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
            assert _bytes(_run(c, mode, which)) == want, (name, mode, which)


def _pair():
    src, sl, tgt, tl, T = synth.config1_pair()
    return src, sl, tgt, tl, np_ref.mat_to_qt(T)


PAIR_PLANE = dict(plane_ref.DEFAULTS, distance_threshold=0.05, num_hypotheses=96, max_planes=3, min_inliers=30)


def test_a_laid_out_cloud_gives_the_same_bytes():
    """before and after an align() has put the clouds on the device in the mode's layout, on an EM and on a SEMANTIC handle"""
    src, sl, tgt, tl, qt = _pair()
    ref = plane_ref.segment_planes(src, sl, None, **PAIR_PLANE)
    want = _bytes(ref)
    p = _params(PAIR_PLANE)
    for mode in (E, S):
        with _engine(mode) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            assert _bytes(e.segment_planes(SRC, p)) == want, mode
            e.align(qt)
            assert _bytes(e.segment_planes(SRC, p)) == want, mode
            assert e.segment_planes(TGT, p)["info"]["n_candidates"] == len(tgt)


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("street_refine1_z", "room_corner", f"tile_{plane_cases.TILE_SIZES[3]}"):
        c = plane_cases.case(name)
        with _engine(E) as e:
            e.set_source(c["xyz"], c["labels"])
            a = _bytes(e.segment_planes(SRC, _params(c["params"]), c["mask"]))
            b = _bytes(e.segment_planes(SRC, _params(c["params"]), c["mask"]))
        assert a == b == _bytes(_run(c)), name


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


def test_the_handle_is_untouched():
    src, sl, tgt, tl, qt = _pair()
    p = _params(PAIR_PLANE)
    res = []
    for with_planes in (False, True):
        with _engine(E) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            if with_planes:
                assert e.segment_planes(SRC, p)["info"]["n_candidates"] > 0  # before anything is on the device in a layout
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_planes:
                e.segment_planes(SRC, p)
                e.segment_planes(TGT, p)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            second = e.align(qt)
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                        _drop_times(second[1])))
    assert res[0] == res[1]


# ---- refusals and capacity ----------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points, capacity=sicp.PLANE_MAX_PLANES, tables=True):
        self.capacity, self.tables = capacity, tables
        rows = max(capacity, 1)
        self.pid = np.full(4 * max(n_points, 1), SENTINEL, np.uint8)
        self.bufs = {k: np.full(w * rows, SENTINEL, np.uint8) for k, w in (("coeff", 32), ("count", 4), ("hyp_index", 4), ("hyp_count", 4),
                                                                         ("centroid", 24), ("rms", 8))}
        self.info = sicp.SicpPlaneInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, e, which, params, mask=None):
        bp, dp, ip = (C.POINTER(t) for t in (C.c_uint8, C.c_double, C.c_int32))
        b = self.bufs
        t = (lambda k, ty: b[k].ctypes.data_as(ty)) if self.tables else (lambda k, ty: None)
        return sicp.lib().sicp_segment_planes(
            None if e is None else e._h, which, None if params is None else C.byref(params), None if mask is None else mask.ctypes.data_as(bp),
            self.pid.ctypes.data_as(ip), self.capacity, t("coeff", dp), t("count", ip), t("hyp_index", ip), t("hyp_count", ip), t("centroid", dp),
            t("rms", dp), C.byref(self.info))

    def arrays_untouched(self):
        return (self.pid == SENTINEL).all() and all((a == SENTINEL).all() for a in self.bufs.values())

    def untouched(self):
        return self.arrays_untouched() and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = plane_cases.case("nan_mix")
    n = len(c["xyz"])
    P = sicp.default_plane_params
    nan, inf = float("nan"), float("inf")
    many, neg = P(), P()
    many.n_ignore, neg.n_ignore = 17, -1
    two = np.zeros(n, np.uint8)
    two[[3, 8]] = 1
    none = np.zeros(n, np.uint8)
    with _engine(G) as a, _engine(G) as nolab, _engine(S) as sem_nolab, _engine(E) as pair:
        a.set_source(c["xyz"], c["labels"])
        nolab.set_source(c["xyz"])
        sem_nolab.set_source(c["xyz"])
        pair.set_source(c["xyz"][[0, 2]], c["labels"][[0, 2]])
        refused = [
            ("NULL handle", INV, (None, SRC, P())),
            ("NULL params", INV, (a, SRC, None)),
            ("which 2", INV, (a, 2, P())),
            ("which -1", INV, (a, -1, P())),
            ("t zero", INV, (a, SRC, P(distance_threshold=0.0))),
            ("t negative", INV, (a, SRC, P(distance_threshold=-0.1))),
            ("t nan", INV, (a, SRC, P(distance_threshold=nan))),
            ("t inf", INV, (a, SRC, P(distance_threshold=inf))),
            ("axis nan", INV, (a, SRC, P(axis=(0, nan, 1), min_cos=0.5))),
            ("axis inf", INV, (a, SRC, P(axis=(inf, 0, 1), min_cos=0.5))),
            ("axis, min_cos 0", INV, (a, SRC, P(axis=(0, 0, 1)))),
            ("axis, min_cos above 1", INV, (a, SRC, P(axis=(0, 0, 1), min_cos=1.0000001))),
            ("axis, min_cos negative", INV, (a, SRC, P(axis=(0, 0, 1), min_cos=-0.5))),
            ("axis, min_cos nan", INV, (a, SRC, P(axis=(0, 0, 1), min_cos=nan))),
            ("min_cos without an axis", INV, (a, SRC, P(min_cos=0.5))),
            ("H 0", INV, (a, SRC, P(num_hypotheses=0))),
            ("H 4097", INV, (a, SRC, P(num_hypotheses=4097))),
            ("max_planes 0", INV, (a, SRC, P(max_planes=0))),
            ("max_planes 17", INV, (a, SRC, P(max_planes=17))),
            ("min_inliers 2", INV, (a, SRC, P(min_inliers=2))),
            ("refine 2", INV, (a, SRC, P(refine=2))),
            ("refine -1", INV, (a, SRC, P(refine=-1))),
            ("n_ignore 17", INV, (a, SRC, many)),
            ("n_ignore -1", INV, (a, SRC, neg)),
            ("no labels, a label ignored", INV, (nolab, SRC, P(ignore=(3,)))),
            ("slot without a cloud", NR, (a, TGT, P())),
            ("SEMANTIC handle, cloud never uploaded", NR, (sem_nolab, SRC, P())),
            ("two points", FEW, (pair, SRC, P(min_inliers=3))),
            ("two candidates", FEW, (a, SRC, P(min_inliers=3), two)),
            ("no candidate", FEW, (a, SRC, P(min_inliers=3), none)),
            ("every label ignored", FEW, (a, SRC, P(ignore=(1, 2, 3)))),
        ]
        for what, code, args in refused:
            raw = _Raw(n)
            assert raw.call(*args) == code, what
            assert raw.untouched(), what
        raw = _Raw(n, capacity=-1)
        assert raw.call(a, SRC, P()) == INV and raw.untouched()
        # the accepted forms: a cloud without labels, min_cos = 1 exactly
        kw = dict(c["params"], ignore=())
        _same(nolab.segment_planes(SRC, _params(kw)), plane_ref.segment_planes(c["xyz"], None, None, **kw))
        assert a.segment_planes(SRC, P(axis=(0, 0, 1), min_cos=1.0))["info"]["rounds"] == 1
        # a raw call that succeeds writes everything
        raw = _Raw(n)
        assert raw.call(a, SRC, _params(c["params"])) == sicp.OK
        ref = plane_cases.reference("nan_mix")
        k = ref["n_planes"]
        assert raw.pid.view(np.int32).tobytes() == ref["plane_id"].tobytes() and raw.info.n_planes == k
        assert raw.bufs["coeff"].view(np.float64)[:4 * k].tobytes() == ref["coeff"].tobytes()
        assert raw.bufs["rms"].view(np.float64)[:k].tobytes() == ref["rms"].tobytes()
        assert (raw.bufs["coeff"][32 * k:] == SENTINEL).all()  # (rows past n_planes stay)


def test_capacity_follows_the_cluster_rule():
    c = plane_cases.case("room_corner")
    ref = plane_cases.reference("room_corner")
    n = len(c["xyz"])
    p = _params(c["params"])
    with _engine(E) as e:
        e.set_source(c["xyz"], c["labels"])
        # too small with table arrays: info written, nothing else
        raw = _Raw(n, capacity=2)
        assert raw.call(e, SRC, p) == INV
        assert raw.arrays_untouched() and raw.info.n_planes == 3 and raw.info.rounds == 4 and raw.info.n_assigned == ref["n_assigned"]
        assert "3 planes" in sicp.lib().sicp_last_error(e._h).decode()
        # no table arrays: capacity plays no part
        raw = _Raw(n, capacity=0, tables=False)
        assert raw.call(e, SRC, p) == sicp.OK
        assert raw.pid.view(np.int32).tobytes() == ref["plane_id"].tobytes() and raw.info.n_planes == 3
        # exactly enough
        raw = _Raw(n, capacity=3)
        assert raw.call(e, SRC, p) == sicp.OK
        assert raw.bufs["count"].view(np.int32).tolist() == ref["count"].tolist()
        assert raw.bufs["centroid"].view(np.float64).tobytes() == ref["centroid"].tobytes()


# ---- the recipe ---------------------------------------------------------------------------------------------------------------
def test_removing_the_ground_separates_the_objects_of_a_cloud_without_labels():
    """INTEGRATION.md, "Planes of a cloud": on the street scan without labels everything standing on the road is one component;
    segment_planes(axis = up) -> mask = plane_id != 0 -> filter(mask, dst) -> cluster separates it"""
    xyz = plane_cases.unlabelled_street()
    kw = dict(plane_ref.DEFAULTS, **plane_cases.RECIPE_PLANE)
    ref = plane_ref.segment_planes(xyz, None, None, **kw)
    rest = xyz[ref["plane_id"] != 0]
    whole, parts = cluster_ref.cluster(xyz, None, **plane_cases.RECIPE_CLUSTER), cluster_ref.cluster(rest, None, **plane_cases.RECIPE_CLUSTER)
    print("unfiltered:", whole["n_clusters"], "clusters, the largest of", whole["max_cluster_points"], "of", len(xyz))
    print("ground removed:", parts["n_clusters"], "clusters, the largest of", parts["max_cluster_points"], "of", len(rest))
    assert whole["max_cluster_points"] > 0.9 * len(xyz)            # one giant component
    assert parts["n_clusters"] > 1 and parts["max_cluster_points"] < 0.4 * len(rest)
    cp = sicp.default_cluster_params(**{k: v for k, v in plane_cases.RECIPE_CLUSTER.items() if k != "ignore"})
    with _engine(G) as e, _engine(G) as other:
        e.set_source(xyz)
        got = e.cluster(SRC, cp)
        assert (got["info"]["n_clusters"], got["info"]["max_cluster_points"]) == (whole["n_clusters"], whole["max_cluster_points"])
        planes = e.segment_planes(SRC, _params(kw))
        assert planes["plane_id"].tobytes() == ref["plane_id"].tobytes()
        mask = (planes["plane_id"] != 0).astype(np.uint8)
        kept = e.filter(SRC, sicp.default_filter_params(mean_k=0), mask, dst=other, dst_which=SRC)
        assert kept["info"]["n_kept"] == len(rest)
        got = other.cluster(SRC, cp)
        assert (got["info"]["n_clusters"], got["info"]["max_cluster_points"]) == (parts["n_clusters"], parts["max_cluster_points"])
        assert got["count"].tolist() == parts["count"].tolist()
