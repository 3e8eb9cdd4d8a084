"""GPU tests of sicp_merge_clouds: positions, labels, counts and info counts equal tests/merge_ref.py exactly on every case of
tests/merge_cases.py, whatever the parts' handles' modes; a dst slot is what sicp_set_cloud of the returned arrays makes it
(an align() from it has the same bits); every refusal leaves outputs and dst as they were; the parts' handles keep their
correspondences and statistics."""
import importlib

import numpy as np
import pytest

import merge_cases
import merge_ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
INFO_COUNTS = ("n_in", "n_kept", "n_out", "max_voxel_points", "has_label")


def _engine(mode=G, **kw):
    p = sicp.default_params(mode)
    p.num_classes = 11
    for k, v in kw.items():
        setattr(p, k, v)
    return sicp.Engine(0, p)


def _load(parts, modes=None):
    """one handle per part (mode GICP unless given), the cloud in its source or target slot by turns -> [(engine, which)]"""
    out = []
    for i, (xyz, lab) in enumerate(parts):
        e = _engine(G if modes is None else modes[i])
        e.set_cloud(i % 2, xyz, lab)
        out.append((e, i % 2))
    return out


def _close(handles):
    for e in {id(e): e for e, _ in handles}.values():
        e.close()


def _params(c):
    return sicp.default_merge_params(leaf_size=c["leaf"], crop_center=c["center"], crop_range=c["crop_range"])


def _same(out, ref):
    assert out["xyz"].dtype == np.float32 and out["xyz"].shape == ref["xyz"].shape
    assert np.array_equal(out["xyz"].view(np.uint32), ref["xyz"].view(np.uint32))
    assert np.array_equal(out["count"], ref["count"])
    assert (out["labels"] is None) == (ref["labels"] is None)
    if ref["labels"] is not None:
        assert np.array_equal(out["labels"], ref["labels"])
    for k in INFO_COUNTS:
        assert out["info"][k] == ref[k], k


def _same_out(a, b):
    assert a["xyz"].tobytes() == b["xyz"].tobytes() and a["count"].tobytes() == b["count"].tobytes()
    assert (a["labels"] is None) == (b["labels"] is None) and (a["labels"] is None or a["labels"].tobytes() == b["labels"].tobytes())
    assert {k: a["info"][k] for k in INFO_COUNTS} == {k: b["info"][k] for k in INFO_COUNTS}


# ---- the result ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", merge_cases.NAMES)
def test_result_equals_the_restatement(name):
    """1, 2, 3 and 5 parts of 255 / 256 / 257 / 1 / 3000 points with non-finite rows; crop off, on and +inf; a part (one point, or
    a whole workgroup of 256) cropped away; leaf 0; no labels; the 5500-point voxel with a label tie; d^2 = range^2"""
    c = merge_cases.case(name)
    hs = _load(c["parts"])
    try:
        out = sicp.merge_clouds(hs, c["qts"], _params(c))
        _same(out, merge_cases.reference(name))
        again = sicp.merge_clouds(hs, c["qts"], _params(c))  # two calls, the same bits
        _same_out(out, again)
        counts_only = sicp.merge_clouds(hs, c["qts"], _params(c), want_points=False)
        assert counts_only["xyz"] is None and counts_only["count"] is None
        assert {k: counts_only["info"][k] for k in INFO_COUNTS} == {k: out["info"][k] for k in INFO_COUNTS}
        assert out["info"]["t_total_ms"] > 0
    finally:
        _close(hs)


def test_null_poses_are_explicit_identities():
    c = merge_cases.case("five_identity")
    hs = _load(c["parts"])
    try:
        a = sicp.merge_clouds(hs, None, _params(c))
        b = sicp.merge_clouds(hs, np.tile(IDENT, (len(hs), 1)), _params(c))
        _same_out(a, b)
        _same(a, merge_cases.reference("five_identity"))
    finally:
        _close(hs)


def test_the_handles_mode_plays_no_part():
    """one labelled cloud on a GICP, an EM and a SEMANTIC handle (whose device layout is grouped by label): alone each gives the
    restatement's result, and so do the three together -- mixed modes in one call -- at three poses"""
    c = merge_cases.case("one")
    part = c["parts"][0]
    hs = _load([part] * 3, modes=[G, E, S])
    try:
        for h in hs:
            _same(sicp.merge_clouds([h], c["qts"], _params(c)), merge_cases.reference("one"))
        qts = merge_cases.track(3)
        want = merge_ref.merge([part] * 3, qts, c["leaf"], c["center"], 7.0)
        p = sicp.default_merge_params(leaf_size=c["leaf"], crop_center=c["center"], crop_range=7.0)
        _same(sicp.merge_clouds(hs, qts, p), want)
        _same(sicp.merge_clouds(hs[::-1], qts, p), want)  # (the same cloud in every part: the order of the handles is immaterial)
    finally:
        _close(hs)


def test_one_cloud_as_two_parts_and_a_shared_cloud():
    c = merge_cases.case("two")
    (e, w), = _load(c["parts"][:1])
    other = _engine(S)
    try:
        other.share_cloud(TGT, e, w)
        part = c["parts"][0]
        want = merge_ref.merge([part, part, part], merge_cases.track(3), c["leaf"], c["center"], c["crop_range"])
        out = sicp.merge_clouds([(e, w), (e, w), (other, TGT)], merge_cases.track(3), _params(c))
        _same(out, want)
        assert out["info"]["n_in"] == 3 * e.cloud_size(w)[1]
    finally:
        other.close()
        e.close()


@pytest.mark.parametrize("leaf", [0.25, 0.0], ids=["grid", "leaf0"])
def test_a_part_without_finite_points_owns_no_workgroup(leaf):
    """three parts, one of them all NaN -- no device point, no workgroup of the key launch -- as the first, the middle and the
    last part: byte for byte the merge of the two others, and the restatement's"""
    scans = [merge_cases.scan(310, 2000), merge_cases.scan(311, 2100)]
    qts = merge_cases.track(3)
    nothing = (np.full((700, 3), np.nan, np.float32), np.arange(700, dtype=np.uint32) % 5 + 1)
    p = sicp.default_merge_params(leaf_size=leaf, crop_center=(0.5, 0, 0), crop_range=8.0)
    two = _load(scans)
    try:
        for at in range(3):
            keep = [k for k in range(3) if k != at]
            parts = list(scans)
            parts.insert(at, nothing)
            hs = _load(parts)
            try:
                out = sicp.merge_clouds(hs, qts, p)
                _same_out(out, sicp.merge_clouds(two, qts[keep], p))
                _same(out, merge_ref.merge(parts, qts, leaf, (0.5, 0, 0), 8.0))
                assert out["info"]["n_in"] == sum(e.cloud_size(w)[1] for e, w in two) and out["info"]["n_out"] > 0
            finally:
                _close(hs)
    finally:
        _close(two)


# ---- dst ----------------------------------------------------------------------------------------------------------------------
def _align_bits(e, init=IDENT):
    qt, st = e.align(init)
    keys = ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost")
    return qt.tobytes(), tuple(st[k] for k in keys)


@pytest.mark.parametrize("mode", [G, S], ids=["gicp", "semantic"])
def test_dst_is_what_set_cloud_of_the_arrays_makes_it(mode):
    src, sl, tgt, tl, _ = synth.config1_pair()
    half = len(tgt) // 2
    parts = [(tgt[:half], tl[:half]), (tgt[half:], tl[half:])]
    hs = _load(parts)
    a, b, sharer = _engine(mode), _engine(mode), _engine(mode)
    try:
        a.set_source(src, sl)
        a.set_target(tgt[:300], tl[:300])   # the old cloud of the slot ...
        sharer.set_source(src, sl)
        sharer.share_cloud(TGT, a, TGT)     # ... which another handle shares
        before = _align_bits(sharer)
        p = sicp.default_merge_params(leaf_size=0.1)
        out = sicp.merge_clouds(hs, None, p, dst=(a, TGT))
        _same(out, merge_ref.merge(parts, None, 0.1))
        n_out = out["info"]["n_out"]
        assert 0 < n_out < len(tgt) and a.cloud_size(TGT) == (n_out, n_out)
        assert sharer.cloud_size(TGT) == (300, 300) and _align_bits(sharer) == before
        b.set_source(src, sl)
        b.set_target(out["xyz"], out["labels"])
        assert _align_bits(a) == _align_bits(b)
    finally:
        _close(hs)
        for e in (a, b, sharer):
            e.close()


def test_rolling_map_dst_is_a_part():
    scans = [merge_cases.scan(200 + i, 2000) for i in range(3)]
    qts = merge_cases.track(3)
    m = _engine(S)
    feeders = _load(scans[1:])
    try:
        m.set_target(*scans[0])
        p = sicp.default_merge_params(leaf_size=0.25, crop_center=(0.5, 0, 0), crop_range=7.0)
        ref_map = scans[0]
        for r in (1, 2):
            q = np.stack([IDENT, qts[r]])
            want = merge_ref.merge([ref_map, scans[r]], q, 0.25, (0.5, 0, 0), 7.0)
            out = sicp.merge_clouds([(m, TGT), feeders[r - 1]], q, p, dst=(m, TGT))
            _same(out, want)
            assert m.cloud_size(TGT) == (want["n_out"], want["n_out"])
            ref_map = (want["xyz"], want["labels"])
        # the map the handle now holds is the second round's result: merged alone with leaf 0 it comes back point for point
        back = sicp.merge_clouds([(m, TGT)], None, sicp.default_merge_params(leaf_size=0.0))
        assert back["xyz"].tobytes() == ref_map[0].tobytes() and np.array_equal(back["labels"], ref_map[1])
    finally:
        m.close()
        _close(feeders)


# ---- what a call leaves alone -------------------------------------------------------------------------------------------------
def test_part_handles_keep_correspondences_and_statistics():
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    e, d = _engine(E), _engine(G)
    try:
        e.set_confusion(synth.confusion_matrix(11))
        e.set_source(src, sl)
        e.set_target(tgt, tl)
        e.align(qt)
        idx, d2, w = e.correspondences(qt)
        acc, stats = e.accumulate(qt), e.stats()
        sicp.merge_clouds([(e, SRC), (e, TGT)], np.stack([qt, IDENT]), sicp.default_merge_params(leaf_size=0.3), dst=(d, TGT))
        assert d.cloud_size(TGT)[1] > 0
        assert e.stats() == stats
        assert e.accumulate(qt).tobytes() == acc.tobytes()  # (the correspondences on the device are the ones from before)
        idx2, d22, w2 = e.correspondences(qt)
        assert idx2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
    finally:
        e.close()
        d.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A5A5A5A


class _Raw:
    """the C call with outputs the test owns: arrays filled with a sentinel, an info block filled with 0x5A bytes"""

    def __init__(self, cap):
        self.cap = cap
        self.arr = [np.full(max(cap, 1), SENTINEL, dtype=np.uint32) for _ in range(5)]
        self.info = sicp.SicpMergeInfo()
        C.memset(C.byref(self.info), 0x5A, C.sizeof(self.info))

    def call(self, handles, which, n, qts, params, dst=None, dst_which=TGT, arrays=True):
        hs = None if handles is None else (C.c_void_p * len(handles))(*[None if e is None else e._h for e in handles])
        wh = None if which is None else np.asarray(which, dtype=np.int32)
        q = None if qts is None else np.ascontiguousarray(qts, dtype=np.float64)
        ptr = lambda a, t: a.ctypes.data_as(t) if arrays else None
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        return sicp.lib().sicp_merge_clouds(
            hs, None if wh is None else wh.ctypes.data_as(C.POINTER(C.c_int32)), n, None if q is None else q.ctypes.data_as(C.POINTER(C.c_double)),
            None if params is None else C.byref(params), None if dst is None else dst._h, dst_which, self.cap,
            ptr(self.arr[0], fp), ptr(self.arr[1], fp), ptr(self.arr[2], fp), ptr(self.arr[3], up), ptr(self.arr[4], up), C.byref(self.info))

    def arrays_untouched(self):
        return all((a == SENTINEL).all() for a in self.arr)

    def info_untouched(self):
        return bytes(self.info) == b"\x5a" * C.sizeof(self.info)


def _dst_state(d):
    r = d.evaluate(IDENT, 4.0)
    return d.cloud_size(SRC), d.cloud_size(TGT), np.array([r[k] for k in sorted(r)], dtype=np.float64).tobytes()


def test_refusals_leave_outputs_and_dst_untouched():
    xyz, lab = merge_cases.scan(300, 600)
    a, b, nolab, empty, sem_nolab, d = _engine(G), _engine(E), _engine(G), _engine(G), _engine(S), _engine(G)
    try:
        a.set_source(xyz, lab)
        b.set_target(xyz[:257], lab[:257])
        nolab.set_source(xyz[:100])
        sem_nolab.set_source(xyz[:100])
        d.set_source(xyz[:400], lab[:400])
        d.set_target(xyz[200:], lab[200:])
        state = _dst_state(d)
        ok = sicp.default_merge_params()
        P = sicp.default_merge_params
        nan, inf = float("nan"), float("inf")
        bad_pose = np.stack([IDENT, IDENT])
        bad_pose[1, 5] = nan
        inf_pose = np.stack([IDENT, IDENT])
        inf_pose[0, 0] = inf
        INV, NR = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY
        two, w2 = [a, b], [SRC, TGT]
        refused = [
            ("n_parts 0", INV, (two, w2, 0, None, ok)),
            ("n_parts negative", INV, (two, w2, -1, None, ok)),
            ("NULL handle array", INV, (None, w2, 2, None, ok)),
            ("NULL part_which", INV, (two, None, 2, None, ok)),
            ("NULL first handle", INV, ([None, b], w2, 2, None, ok)),
            ("NULL second handle", INV, ([a, None], w2, 2, None, ok)),
            ("NULL params", INV, (two, w2, 2, None, None)),
            ("which 2", INV, (two, [SRC, 2], 2, None, ok)),
            ("which -1", INV, (two, [-1, TGT], 2, None, ok)),
            ("leaf negative", INV, (two, w2, 2, None, P(leaf_size=-0.1))),
            ("leaf nan", INV, (two, w2, 2, None, P(leaf_size=nan))),
            ("leaf inf", INV, (two, w2, 2, None, P(leaf_size=inf))),
            ("range negative", INV, (two, w2, 2, None, P(crop_range=-1.0))),
            ("range nan", INV, (two, w2, 2, None, P(crop_range=nan))),
            ("centre inf", INV, (two, w2, 2, None, P(crop_center=(0, inf, 0), crop_range=3.0))),
            ("centre nan", INV, (two, w2, 2, None, P(crop_center=(nan, 0, 0)))),
            ("pose nan", INV, (two, w2, 2, bad_pose, ok)),
            ("pose inf", INV, (two, w2, 2, inf_pose, ok)),
            ("labelled and unlabelled", INV, ([a, nolab], [SRC, SRC], 2, None, ok)),
            ("slot without a cloud", NR, ([a, empty], [SRC, SRC], 2, None, ok)),
            ("a's empty slot", NR, ([a], [TGT], 1, None, ok)),
            ("voxel out of range", INV, ([a], [SRC], 1, np.array([[0, 0, 0, 1, 100.0, 0, 0]]), P(leaf_size=1e-6))),
        ]
        for what, code, args in refused:
            for dst in (None, d):
                raw = _Raw(2000)
                assert raw.call(*args, dst=dst) == code, what
                assert raw.arrays_untouched() and raw.info_untouched(), what
                assert _dst_state(d) == state, what
        raw = _Raw(2000)
        assert raw.call(two, w2, 2, None, ok, dst=d, dst_which=2) == INV and raw.arrays_untouched() and raw.info_untouched()
        raw = _Raw(2000)
        assert raw.call([a], [SRC], 1, np.array([[0, 0, 0, 1, 100.0, 0, 0]]), P(leaf_size=1e-6)) == INV
        assert "leaf size" in sicp.lib().sicp_last_error(a._h).decode()
        # a SEMANTIC-mode handle never uploaded its unlabelled cloud: its next call would answer the same
        raw = _Raw(2000)
        assert raw.call([sem_nolab], [SRC], 1, None, ok) == NR and raw.arrays_untouched()
        if sicp.device_count() > 1:
            far = sicp.Engine(1, sicp.default_params(G))
            far.set_source(xyz, lab)
            raw = _Raw(2000)
            assert raw.call([a, far], [SRC, SRC], 2, None, ok) == INV and raw.arrays_untouched() and raw.info_untouched()
            raw = _Raw(2000)
            assert raw.call([a], [SRC], 1, None, ok, dst=far) == INV and raw.arrays_untouched() and raw.info_untouched()
            far.close()
        # too small a capacity: refused, info written, nothing else
        want = merge_ref.merge([(xyz, lab), (xyz[:257], lab[:257])], None, 0.2)
        raw = _Raw(want["n_out"] - 1)
        assert raw.call(two, w2, 2, None, ok, dst=d) == INV
        assert raw.arrays_untouched() and not raw.info_untouched() and _dst_state(d) == state
        assert (raw.info.n_in, raw.info.n_kept, raw.info.n_out, raw.info.max_voxel_points, raw.info.has_label) == \
            (want["n_in"], want["n_kept"], want["n_out"], want["max_voxel_points"], 1)
        # ... and with exactly enough it goes through (no dst)
        raw = _Raw(want["n_out"])
        assert raw.call(two, w2, 2, None, ok) == sicp.OK and raw.info.n_out == want["n_out"]
        assert np.array_equal(raw.arr[0].view(np.float32), want["xyz"][:, 0]) and np.array_equal(raw.arr[3], want["labels"])
        # without arrays the capacity is not looked at
        raw = _Raw(0)
        assert raw.call(two, w2, 2, None, ok, arrays=False) == sicp.OK and raw.info.n_out == want["n_out"]
        # an empty result into a dst: refused, dst unchanged; without a dst it is a result
        away = P(crop_center=(500, 0, 0), crop_range=1.0)
        raw = _Raw(2000)
        assert raw.call(two, w2, 2, None, away, dst=d) == sicp.ERR_TOO_FEW_POINTS
        assert raw.arrays_untouched() and _dst_state(d) == state
        raw = _Raw(2000)
        assert raw.call(two, w2, 2, None, away) == sicp.OK and raw.arrays_untouched()
        assert (raw.info.n_in, raw.info.n_kept, raw.info.n_out, raw.info.max_voxel_points) == (want["n_in"], 0, 0, 0)
    finally:
        for e in (a, b, nolab, empty, sem_nolab, d):
            e.close()
