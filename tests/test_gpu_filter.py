"""GPU tests of sicp_filter: keep, mean_dist, neighbors and info equal tests/filter_ref.py exactly -- integers equal, floats
bit-equal -- on every case of tests/filter_cases.py, whatever the handle's mode, slot and device layout; a filtered dst is the
cloud set_cloud of the kept arrays would make; a call without dst leaves the handle as it was; every refusal leaves the outputs
as they were.

The variance that rounds below zero: filter_cases.search_clamped() finds one on the CPU (three 0.5 x 1.25 rectangles, mean_k = 3:
twelve equal m), the case "clamped"."""
import importlib

import numpy as np
import pytest

import filter_cases
import filter_ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
ARRAYS = ("keep", "mean_dist", "neighbors")
DTYPES = dict(keep=np.uint8, mean_dist=np.float64, neighbors=np.int32)
COUNTS = ("n_points", "n_finite", "n_tested", "n_protected", "n_kept", "n_fail_stat", "n_fail_radius")
FLOATS = ("mean", "stddev", "threshold")
INV, NR, FEW = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_TOO_FEW_POINTS


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _params(c, **over):
    kw = dict(c["params"], **over)
    return sicp.default_filter_params(drop=kw.pop("drop"), protect=kw.pop("protect"), **kw)


def _run(c, mode=E, which=SRC):
    with _engine(mode) as e:
        e.set_cloud(which, c["xyz"], c["labels"])
        return e.filter(which, _params(c), c["mask"])


def _same(out, ref):
    for k in COUNTS + FLOATS:
        print(k, out["info"][k], ref[k])
    for k in COUNTS:
        assert out["info"][k] == ref[k], k
    for k in FLOATS:
        assert np.float64(out["info"][k]).tobytes() == np.float64(ref[k]).tobytes(), k
    for k in ARRAYS:
        assert out[k].dtype == DTYPES[k] and out[k].shape == ref[k].shape, k
        assert out[k].tobytes() == ref[k].tobytes(), k


def _bytes(out):
    return b"".join(out[k].tobytes() for k in ARRAYS) + repr([out["info"][k] for k in COUNTS + FLOATS]).encode()


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", filter_cases.NAMES)
def test_result_equals_the_restatement(name):
    """the street scan with planted points under the statistical test, the radius test and both; every list length at 150 points
    and at exactly mean_k + 1 finite points; duplicated points; non-finite points; the tree sum at one run of the kernel less one,
    exactly, plus one and several runs with holes; the threshold met exactly; the clamped variance; pairs at r and one ulp inside,
    across cell faces, edges and corners; the dense cell; three interleaved labels; the pure selections"""
    out = _run(filter_cases.case(name))
    _same(out, filter_cases.reference(name))
    assert out["info"]["t_total_ms"] > 0


@pytest.mark.parametrize("k", filter_cases.MEAN_KS)
def test_mean_k_finite_points_are_too_few(k):
    c = filter_cases.too_few(k)
    with _engine(E) as e:
        e.set_source(c["xyz"], c["labels"])
        with pytest.raises(sicp.SicpError) as err:
            e.filter(SRC, _params(c))
        assert err.value.status == FEW
        assert e.filter(SRC, _params(c, mean_k=k - 1))["info"]["n_finite"] == k  # (one shorter: exactly enough, or the test off)


def test_the_same_bytes_on_every_mode_slot_and_layout():
    """a SEMANTIC handle groups the cloud by label and searches it label by label: three interleaved labels, one of them on
    five points -- fewer than the lists are long"""
    c = filter_cases.case("interleaved")
    want = _bytes({**filter_cases.reference("interleaved"), "info": filter_cases.reference("interleaved")})
    for mode, which in ((E, SRC), (E, TGT), (G, SRC), (S, SRC), (S, TGT)):
        assert _bytes(_run(c, mode, which)) == want, (mode, which)
    c = filter_cases.case("street_both")
    assert _bytes(_run(c, S, TGT)) == _bytes(_run(c, E, SRC))


def _rare_label_pair():
    """config1's pair with five source points relabelled 7: a label with fewer points than the lists are long"""
    src, sl, tgt, tl, T = synth.config1_pair()
    sl = sl.copy()
    sl[[3, 500, 901, 1400, 2000]] = 7
    return src, sl, tgt, tl, np_ref.mat_to_qt(T)


def test_a_laid_out_cloud_gives_the_same_bytes():
    """before and after an align() has put the clouds on the device in the mode's layout, on an EM and on a SEMANTIC handle"""
    src, sl, tgt, tl, qt = _rare_label_pair()
    p = sicp.default_filter_params(mean_k=10, std_mul=1.0, radius=0.12, min_neighbors=4, protect=(7,))
    ref = filter_ref.filter(src, sl, None, 10, 1.0, 0.12, 4, (), (7,))
    assert ref["n_fail_stat"] > 0 and ref["n_fail_radius"] > 0 and ref["n_protected"] == 5
    want = _bytes({**ref, "info": ref})
    for mode in (E, S):
        with _engine(mode) as e:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            assert _bytes(e.filter(SRC, p)) == want, mode
            e.align(qt)
            assert _bytes(e.filter(SRC, p)) == want, mode
            assert e.filter(TGT, p)["info"]["n_kept"] > 0


# ---- dst ------------------------------------------------------------------------------------------------------------------------
def _drop_times(st):
    return {k: v for k, v in st.items() if not k.startswith("t_") and not k.endswith("_ms")}


@pytest.mark.parametrize("mode", [E, S])
def test_an_align_on_the_filtered_dst_equals_one_on_the_host_filtered_arrays(mode):
    src, sl, tgt, tl, qt = _rare_label_pair()
    p = sicp.default_filter_params(mean_k=10, std_mul=1.0, radius=0.12, min_neighbors=4, drop=(7,))
    mask = (np.arange(len(src)) % 5 != 2).astype(np.uint8)
    ref = filter_ref.filter(src, sl, mask, 10, 1.0, 0.12, 4, (7,), ())
    kept = ref["keep"] == 1
    assert 0 < ref["n_kept"] < mask.sum() - 5
    cm = synth.confusion_matrix(11)
    with _engine(mode) as host, _engine(mode) as other, _engine(mode) as holder, _engine(mode) as place:
        for e in (host, other, place):
            e.set_confusion(cm)
            e.set_target(tgt, tl)
        host.set_source(src[kept], sl[kept])
        want = host.align(qt)
        # into another handle
        holder.set_source(src, sl)
        out = holder.filter(SRC, p, mask, dst=other, dst_which=SRC)
        assert out["keep"].tobytes() == ref["keep"].tobytes() and other.n[SRC] == ref["n_kept"]
        assert other.cloud_size(SRC) == (ref["n_kept"], ref["n_kept"]) and holder.cloud_size(SRC) == (len(src), len(src))
        got = other.align(qt)
        assert got[0].tobytes() == want[0].tobytes() and _drop_times(got[1]) == _drop_times(want[1])
        # in place, after an align() on the unfiltered cloud
        place.set_source(src, sl)
        place.align(qt)
        out = place.filter(SRC, p, mask, dst=place)
        assert out["info"]["n_kept"] == ref["n_kept"] and place.cloud_size(SRC) == (ref["n_kept"], ref["n_kept"])
        got = place.align(qt)
        assert got[0].tobytes() == want[0].tobytes() and _drop_times(got[1]) == _drop_times(want[1])
        # the filtered cloud filters like the arrays it is made of
        again = place.filter(SRC, sicp.default_filter_params(mean_k=5))
        _same(again, filter_ref.filter(src[kept], sl[kept], None, 5))


def test_an_empty_result_leaves_dst_as_it_was():
    c = filter_cases.case("select_mask")
    other_xyz, other_lab = filter_cases._cloud(3, 50)
    with _engine(E) as e, _engine(E) as other:
        e.set_source(c["xyz"], c["labels"])
        other.set_target(other_xyz, other_lab)
        before = _bytes(other.filter(TGT, sicp.default_filter_params(mean_k=3)))
        with pytest.raises(sicp.SicpError) as err:
            e.filter(SRC, _params(c), np.zeros(len(c["xyz"]), np.uint8), dst=other, dst_which=TGT)
        assert err.value.status == FEW and "dst keeps its cloud" in sicp.lib().sicp_last_error(e._h).decode()
        assert other.cloud_size(TGT) == (50, 50)
        assert _bytes(other.filter(TGT, sicp.default_filter_params(mean_k=3))) == before
        # without dst the empty selection is a result like any other
        out = e.filter(SRC, _params(c), np.zeros(len(c["xyz"]), np.uint8))
        assert out["info"]["n_kept"] == 0 and not out["keep"].any()
        with pytest.raises(sicp.SicpError) as err:  # in place too: the cloud stays
            e.filter(SRC, _params(c), np.zeros(len(c["xyz"]), np.uint8), dst=e)
        assert err.value.status == FEW and e.cloud_size(SRC) == (300, 299)


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def test_the_handle_is_untouched():
    src, sl, tgt, tl, qt = _rare_label_pair()
    p = sicp.default_filter_params(mean_k=10, radius=0.12, min_neighbors=4)
    res = []
    for with_filter in (False, True):
        with _engine(E) as e, _engine(E) as other:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            if with_filter:
                assert e.filter(SRC, p)["info"]["n_kept"] > 0  # before anything is on the device in a layout
            first = e.align(qt)
            idx, d2, w = e.correspondences(qt)
            stats = e.stats()
            if with_filter:
                e.filter(SRC, p)
                e.filter(TGT, p, dst=other, dst_which=SRC)
                assert e.stats() == stats
                i2, d22, w2 = e.correspondences(qt)
                assert i2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            second = e.align(qt)
            res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), _drop_times(first[1]),
                        _drop_times(second[1])))
    assert res[0] == res[1]


def test_two_calls_and_a_fresh_handle_give_identical_bytes():
    for name in ("street_both", "duplicates", "tree_1613"):
        c = filter_cases.case(name)
        with _engine(E) as e:
            e.set_source(c["xyz"], c["labels"])
            a = _bytes(e.filter(SRC, _params(c), c["mask"]))
            b = _bytes(e.filter(SRC, _params(c), c["mask"]))
        assert a == b == _bytes(_run(c)), name


# ---- refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_points):
        n = max(n_points, 1)
        self.keep = np.full(n, SENTINEL, np.uint8)
        self.md = np.full(8 * n, SENTINEL, np.uint8)
        self.nb = np.full(4 * n, SENTINEL, np.uint8)
        self.info = sicp.SicpFilterInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, e, which, params, mask=None, dst=None, dst_which=SRC):
        bp, dp, ip = (C.POINTER(t) for t in (C.c_uint8, C.c_double, C.c_int32))
        return sicp.lib().sicp_filter(
            None if e is None else e._h, which, None if params is None else C.byref(params),
            None if mask is None else mask.ctypes.data_as(bp), None if dst is None else dst._h, dst_which, self.keep.ctypes.data_as(bp),
            self.md.ctypes.data_as(dp), self.nb.ctypes.data_as(ip), C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in (self.keep, self.md, self.nb)) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_refusals_write_nothing():
    c = filter_cases.case("nan_mix")
    n = len(c["xyz"])
    P = sicp.default_filter_params
    nan, inf = float("nan"), float("inf")
    many, neg = P(), P()
    many.n_drop, neg.n_protect = 17, -1
    few = filter_cases.too_few(4)
    none = np.zeros(n, np.uint8)
    one = none.copy()
    one[3] = 1
    with _engine(G) as a, _engine(G) as nolab, _engine(S) as sem_nolab, _engine(E) as far, _engine(E) as small, _engine(E) as other:
        a.set_source(c["xyz"], c["labels"])
        nolab.set_source(c["xyz"])
        sem_nolab.set_source(c["xyz"])
        far.set_source(filter_cases.cluster_cases.beyond_the_grid(), np.array([3, 3], np.uint32))
        small.set_source(few["xyz"], few["labels"])
        other.set_source(c["xyz"][:40], c["labels"][:40])
        refused = [
            ("NULL handle", INV, (None, SRC, P())),
            ("NULL params", INV, (a, SRC, None)),
            ("which 2", INV, (a, 2, P())),
            ("which -1", INV, (a, -1, P())),
            ("dst_which 2", INV, (a, SRC, P(), None, other, 2)),
            ("mean_k 32", INV, (a, SRC, P(mean_k=32))),
            ("mean_k -1", INV, (a, SRC, P(mean_k=-1))),
            ("std_mul negative", INV, (a, SRC, P(std_mul=-0.5))),
            ("std_mul nan", INV, (a, SRC, P(std_mul=nan))),
            ("std_mul inf", INV, (a, SRC, P(std_mul=inf))),
            ("radius negative", INV, (a, SRC, P(radius=-1.0))),
            ("radius nan", INV, (a, SRC, P(radius=nan))),
            ("radius inf", INV, (a, SRC, P(radius=inf))),
            ("min_neighbors 0 with the radius test on", INV, (a, SRC, P(radius=0.5, min_neighbors=0))),
            ("n_drop 17", INV, (a, SRC, many)),
            ("n_protect -1", INV, (a, SRC, neg)),
            ("a label in both lists", INV, (a, SRC, P(drop=(3, 4), protect=(9, 4)))),
            ("no labels, a label dropped", INV, (nolab, SRC, P(drop=(3,)))),
            ("no labels, a label protected", INV, (nolab, SRC, P(protect=(3,)))),
            ("slot without a cloud", NR, (a, TGT, P())),
            ("SEMANTIC handle, cloud never uploaded", NR, (sem_nolab, SRC, P())),
            ("beyond the grid", INV, (far, SRC, P(mean_k=0, radius=filter_cases.R, min_neighbors=1))),
            ("mean_k finite points", FEW, (small, SRC, P(mean_k=4))),
            ("no tested point", FEW, (a, SRC, P(mean_k=4), none)),
            ("one tested point", FEW, (a, SRC, P(mean_k=4), one)),
            ("every point protected", FEW, (a, SRC, P(mean_k=4, protect=(3, 4, 9)))),
            ("empty result with dst", FEW, (a, SRC, P(mean_k=0), none, other, SRC)),
        ]
        for what, code, args in refused:
            raw = _Raw(n)
            assert raw.call(*args) == code, what
            assert raw.untouched(), what
        assert "radius" in sicp.lib().sicp_last_error(far._h).decode()
        assert other.cloud_size(SRC) == (40, int(np.isfinite(c["xyz"][:40]).all(axis=1).sum()))
        # the same cloud inside the grid of a larger radius; the accepted forms of a cloud without labels and of min_neighbors
        assert far.filter(SRC, P(mean_k=0, radius=2.0, min_neighbors=1))["info"]["n_kept"] == 0
        _same(nolab.filter(SRC, P(mean_k=8, std_mul=1.0)), filter_ref.filter(c["xyz"], None, None, 8, 1.0))
        _same(a.filter(SRC, P(mean_k=8, std_mul=1.0, min_neighbors=0)), filter_ref.filter(c["xyz"], c["labels"], None, 8, 1.0))
        # a raw call that succeeds writes everything
        raw = _Raw(n)
        assert raw.call(a, SRC, P(mean_k=8, std_mul=1.0, radius=0.15, min_neighbors=6, protect=(9,))) == sicp.OK
        ref = filter_cases.reference("nan_mix")
        assert raw.keep.tobytes() == ref["keep"].tobytes() and raw.md.view(np.float64).tobytes() == ref["mean_dist"].tobytes()
        assert raw.nb.view(np.int32).tobytes() == ref["neighbors"].tobytes() and raw.info.n_kept == ref["n_kept"]
