"""GPU tests of sicp_cluster: cluster_id and the whole table equal tests/cluster_ref.py exactly -- integers equal, floats
bit-equal -- on every case of tests/cluster_cases.py, whatever the handle's mode and slot; the partition does not depend on the
order of the points; a call leaves the handle as it was; every refusal leaves the outputs as they were."""
import importlib

import numpy as np
import pytest

import cluster_cases
import cluster_ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
TABLE = ("cluster_id", "label", "count", "first_index", "centroid", "bbox_min", "bbox_max")
COUNTS = ("n_points", "n_kept", "n_components", "n_clusters", "max_cluster_points", "n_clustered")
DTYPES = dict(cluster_id=np.int32, label=np.uint32, count=np.int32, first_index=np.int32, centroid=np.float64, bbox_min=np.float32,
              bbox_max=np.float32)


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(c):
    kw = dict(c["params"])
    return sicp.default_cluster_params(ignore=kw.pop("ignore"), **kw)


def _run(c, mode=E, which=SRC):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return e.cluster(which, _params(c))


def _same(out, ref):
    for k in COUNTS:
        print(k, out["info"][k], ref[k])
    for k in COUNTS:
        assert out["info"][k] == ref[k], k
    for k in TABLE:
        assert out[k].dtype == DTYPES[k] and out[k].shape == ref[k].shape, k
        assert out[k].tobytes() == ref[k].tobytes(), k


def _bytes(out):
    return b"".join(out[k].tobytes() for k in TABLE) + repr([out["info"][k] for k in COUNTS]).encode()


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cluster_cases.NAMES)
def test_result_equals_the_restatement(name):
    """the street scan at both tolerances with and without same_label; the lattice on the threshold and one ulp above; chain,
    comb and sheet in both orders; the dense cell with and without the upper bound; pairs across cell faces, edges and corners at
    every magnitude; non-finite points, every label ignored, one point, no labels, the label vote and its tie"""
    out = _run(cluster_cases.case(name))
    _same(out, cluster_cases.reference(name))
    assert out["info"]["t_total_ms"] > 0


def test_street_scan_has_the_same_bytes_on_every_mode_and_slot():
    c = cluster_cases.case("street_05_same")
    want = _bytes(_run(c, E, SRC))
    for mode, which in ((E, TGT), (G, SRC), (G, TGT), (S, SRC), (S, TGT)):
        assert _bytes(_run(c, mode, which)) == want, (mode, which)


def test_a_laid_out_cloud_gives_the_same_bytes():
    """after an align() the clouds lie on the device in the mode's layout (grouped by label on a SEMANTIC handle); the call reads
    the caller-order copy"""
    src, sl, tgt, tl, T = synth.config1_pair()
    p = sicp.default_cluster_params(min_points=5, tolerance=0.2)
    outs = []
    for mode in (E, S):
        with _engine(mode) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            fresh = _bytes(e.cluster(TGT, p))
            e.align(np_ref.mat_to_qt(T))
            assert _bytes(e.cluster(TGT, p)) == fresh
            outs.append(fresh)
    assert outs[0] == outs[1]
    ref = cluster_ref.cluster(tgt, tl, 0.2, 5)
    assert ref["n_clusters"] >= 3 and outs[0] == _bytes({**ref, "info": ref})


@pytest.mark.parametrize("shape", cluster_cases.LONG)
def test_shuffling_the_points_keeps_the_partition(shape):
    a, b = cluster_cases.case(shape), cluster_cases.case(shape + "_shuffled")
    ra, rb = _run(a), _run(b)
    assert ra["info"]["n_clusters"] == rb["info"]["n_clusters"] == 1
    back = np.empty_like(rb["cluster_id"])
    back[b["perm"]] = rb["cluster_id"]  # shuffled point j is point perm[j]
    assert cluster_ref.partition(back) == cluster_ref.partition(ra["cluster_id"])
    for k in ("label", "count", "bbox_min", "bbox_max"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert np.allclose(ra["centroid"], rb["centroid"], rtol=0, atol=1e-9)  # (the order of the adds differs)


def test_street_scan_shuffled_keeps_partition_counts_labels_and_boxes():
    c = cluster_cases.case("street_05_any")
    perm = np.random.default_rng(43).permutation(len(c["xyz"]))
    ra = _run(c)
    rb = _run({"xyz": c["xyz"][perm], "labels": c["labels"][perm], "params": c["params"]})
    back = np.empty_like(rb["cluster_id"])
    back[perm] = rb["cluster_id"]
    assert cluster_ref.partition(back) == cluster_ref.partition(ra["cluster_id"])
    # the clusters are renumbered: compare the rows as sets
    row = lambda r, j: (int(r["label"][j]), int(r["count"][j]), r["bbox_min"][j].tobytes(), r["bbox_max"][j].tobytes())
    assert sorted(row(ra, j) for j in range(len(ra["count"]))) == sorted(row(rb, j) for j in range(len(rb["count"])))


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def test_the_handle_is_untouched():
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    p = sicp.default_cluster_params(min_points=5, tolerance=0.2)
    res = []
    for with_cluster in (False, True):
        with _engine(E) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            if with_cluster:
                assert e.cluster(SRC, p)["info"]["n_clusters"] > 0  # before anything is on the device in a layout
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_cluster:
                e.cluster(SRC, p)
                e.cluster(TGT, p)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
                stats = e.stats()
            second = e.align(qt)
            drop = lambda st: {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), drop(first[1]), drop(second[1])))
    assert res[0] == res[1]


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("street_03_same", "dense", "two_label_blob"):
        c = cluster_cases.case(name)
        with _engine(E) as e:
            e.set_source(c["xyz"], c["labels"])
            a = _bytes(e.cluster(SRC, _params(c)))
            b = _bytes(e.cluster(SRC, _params(c)))
        assert a == b == _bytes(_run(c)), name


# ---- refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A


class _Raw:
    """the C call with outputs the test owns: arrays filled with a sentinel, an info block filled with 0x5A bytes"""

    def __init__(self, n_points, cap):
        self.cap = cap
        self.cid = np.full(max(n_points, 1), SENTINEL, dtype=np.uint32)
        self.arr = [np.full(3 * max(cap, 1), SENTINEL, dtype=np.uint32) for _ in range(3)]
        self.arr += [np.full(6 * max(cap, 1), SENTINEL, dtype=np.uint32)]  # the centroid's doubles
        self.arr += [np.full(3 * max(cap, 1), SENTINEL, dtype=np.uint32) for _ in range(2)]
        self.info = sicp.SicpClusterInfo()
        C.memset(C.byref(self.info), 0x5A, C.sizeof(self.info))

    def call(self, e, which, params, cap=None):
        ip, up, fp, dp = (C.POINTER(t) for t in (C.c_int32, C.c_uint32, C.c_float, C.c_double))
        a = self.arr
        return sicp.lib().sicp_cluster(
            None if e is None else e._h, which, None if params is None else C.byref(params), self.cid.ctypes.data_as(ip),
            self.cap if cap is None else cap, a[0].ctypes.data_as(up), a[1].ctypes.data_as(ip), a[2].ctypes.data_as(ip),
            a[3].ctypes.data_as(dp), a[4].ctypes.data_as(fp), a[5].ctypes.data_as(fp), C.byref(self.info))

    def arrays_untouched(self):
        return (self.cid == SENTINEL).all() and all((a == SENTINEL).all() for a in self.arr)

    def info_untouched(self):
        return bytes(self.info) == b"\x5a" * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = cluster_cases.case("nan_mix")
    n = len(c["xyz"])
    P = sicp.default_cluster_params
    nan, inf = float("nan"), float("inf")
    INV, NR = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY
    many = P()
    many.n_ignore = 65
    neg = P()
    neg.n_ignore = -1
    with _engine(G) as a, _engine(G) as nolab, _engine(S) as sem_nolab, _engine(E) as far:
        a.set_source(c["xyz"], c["labels"])
        nolab.set_source(c["xyz"])
        sem_nolab.set_source(c["xyz"])
        far.set_source(cluster_cases.beyond_the_grid(), np.array([3, 3], np.uint32))
        loose = P(same_label=0)
        refused = [
            ("NULL handle", INV, (None, SRC, P())),
            ("NULL params", INV, (a, SRC, None)),
            ("which 2", INV, (a, 2, P())),
            ("which -1", INV, (a, -1, P())),
            ("tolerance 0", INV, (a, SRC, P(tolerance=0.0))),
            ("tolerance negative", INV, (a, SRC, P(tolerance=-0.5))),
            ("tolerance nan", INV, (a, SRC, P(tolerance=nan))),
            ("tolerance inf", INV, (a, SRC, P(tolerance=inf))),
            ("min_points 0", INV, (a, SRC, P(min_points=0))),
            ("max_points negative", INV, (a, SRC, P(max_points=-1))),
            ("max_points below min_points", INV, (a, SRC, P(min_points=10, max_points=9))),
            ("same_label 2", INV, (a, SRC, P(same_label=2))),
            ("same_label -1", INV, (a, SRC, P(same_label=-1))),
            ("n_ignore 65", INV, (a, SRC, many)),
            ("n_ignore -1", INV, (a, SRC, neg)),
            ("capacity negative", INV, (a, SRC, P(), -1)),
            ("no labels, same_label 1", INV, (nolab, SRC, P())),
            ("no labels, a label ignored", INV, (nolab, SRC, P(ignore=(3,), same_label=0))),
            ("slot without a cloud", NR, (a, TGT, P())),
            ("SEMANTIC handle, cloud never uploaded", NR, (sem_nolab, SRC, loose)),
            ("beyond the grid", INV, (far, SRC, P(tolerance=cluster_cases.T, min_points=1))),
        ]
        for what, code, args in refused:
            raw = _Raw(n, 400)
            assert raw.call(*args) == code, what
            assert raw.arrays_untouched() and raw.info_untouched(), what
        assert "tolerance" in sicp.lib().sicp_last_error(far._h).decode()
        # the same cloud inside the grid of a larger tolerance
        assert far.cluster(SRC, P(tolerance=2.0, min_points=1))["info"]["n_clusters"] == 2
        # the capacity rule: info is written, nothing else
        ref = cluster_ref.cluster(c["xyz"], c["labels"], **c["params"])
        assert ref["n_clusters"] == 3
        raw = _Raw(n, 2)
        assert raw.call(a, SRC, _params(c)) == INV
        assert raw.arrays_untouched() and not raw.info_untouched()
        assert [getattr(raw.info, k) for k in COUNTS] == [ref[k] for k in COUNTS]
        assert "3 clusters" in sicp.lib().sicp_last_error(a._h).decode()
        raw = _Raw(n, 3)
        assert raw.call(a, SRC, _params(c)) == sicp.OK
        assert raw.cid[:n].view(np.int32).tobytes() == ref["cluster_id"].tobytes()
        assert raw.arr[3][:18].view(np.float64).tobytes() == ref["centroid"].tobytes()
        # the accepted form of a cloud without labels
        out = nolab.cluster(SRC, P(same_label=0, min_points=2))
        _same(out, cluster_ref.cluster(c["xyz"], None, 0.5, 2, 0, 0))
        assert (out["label"] == 0).all()
