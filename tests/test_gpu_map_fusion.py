"""GPU tests of the voxel map's label fusion (sicp_map_set_confusion, sicp_map_extract_fused, sicp_map_fused_labels) against
tests/map_fusion_ref.py: labels, x, y, z and count exactly, the confidence at rtol 1e-12 -- the scores are the same bits on
both sides, exp is within an ulp on both, and a sum of at most 255 positive terms plus one division stays below 3e-14.  Class
counts on both sides of a wave's 64 lanes, which is also the bound up to which the kernels stage log cm in LDS; 255 / 256 /
257 rows and one; voxels without evidence, ruled-out classes, exact ties; the vote where the vote is right; the relabelled scan
in every mode; refusals; dst; determinism.  tests/test_map_fusion_cpu.py asserts the gap condition that makes the exact label
comparison safe."""
import importlib

import numpy as np
import pytest

import map_cases
import map_fusion_cases as cases
import map_fusion_ref as F
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
LEAF = map_cases.LEAF
RTOL = 1e-12


def _engine(mode=G):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _vmap(num_classes, leaf=LEAF):
    return sicp.VoxelMap(0, sicp.default_map_params(leaf_size=leaf, num_classes=num_classes))


def _fill(vm, scans, qts=None, center=None, crop_range=0.0, mode=G):
    e = _engine(mode)
    try:
        for i, (xyz, lab) in enumerate(scans):
            e.set_source(xyz, lab)
            vm.integrate(e, SRC, None if qts is None else qts[i], center, crop_range)
    finally:
        e.close()


def _same_fused(out, ref, vote):
    """extract_fused of the library against the restatement's, and against the library's own extract under the same params"""
    assert out["xyz"].dtype == np.float32 and out["xyz"].tobytes() == ref["xyz"].tobytes() == vote["xyz"].tobytes()
    assert out["count"].tobytes() == ref["count"].tobytes() == vote["count"].tobytes()
    for k in ("n_voxels", "n_out", "max_voxel_points", "has_label"):
        assert out["info"][k] == vote["info"][k], k
    assert out["info"]["n_out"] == ref["n_out"] == len(out["labels"]) == len(out["confidence"])
    print(f"n_out {ref['n_out']}: labels differing {int((out['labels'] != ref['labels']).sum())}, largest relative confidence error "
          f"{float(np.max(np.abs(out['confidence'] - ref['confidence']) / np.maximum(ref['confidence'], 1e-300), initial=0.0)):.3g}")
    assert out["labels"].dtype == np.uint32 and np.array_equal(out["labels"], ref["labels"])
    assert out["confidence"].dtype == np.float64
    assert np.allclose(out["confidence"], ref["confidence"], rtol=RTOL, atol=0.0)
    assert np.array_equal(out["confidence"] == 0.0, ref["labels"] == 0)


# ---- 1. extract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posed", [False, True], ids=["plain", "posed_crop"])
@pytest.mark.parametrize("classes", cases.CLASS_COUNTS)
def test_extract_fused_against_the_restatement(classes, posed):
    scans, qts, center, rng = cases.scans(posed, classes)
    with _vmap(classes) as vm:
        _fill(vm, scans, qts, center, rng)
        vm.set_confusion(cases.matrix(classes))
        for min_count in cases.MIN_COUNTS:
            kw = dict(min_count=min_count, crop_center=center, crop_range=rng)
            ref = cases.reference(posed, classes, min_count)
            assert 0 < ref["n_out"] and (min_count == 1 or ref["n_out"] < cases.reference(posed, classes, 1)["n_out"])
            _same_fused(vm.extract_fused(**kw), ref, vm.extract(**kw))
        counts_only = vm.extract_fused(want_points=False)
        assert counts_only["labels"] is None and counts_only["confidence"] is None
        assert counts_only["info"]["n_out"] == vm.size()[0]


# ---- 2. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_rows_around_a_workgroup(rows):
    rng = np.random.default_rng(rows)
    xyz, _ = map_cases.lattice([[i, 0, 5] for i in range(rows)], per_cell=3, seed=rows)
    lab = rng.integers(0, 5, len(xyz)).astype(np.uint32)
    ref = map_cases.build([(xyz, lab)], num_classes=4)
    L = F.log_matrix(cases.matrix(4))
    with _vmap(4) as vm:
        _fill(vm, [(xyz, lab)])
        vm.set_confusion(cases.matrix(4))
        assert vm.size()[0] == rows
        _same_fused(vm.extract_fused(), F.extract_fused(ref, L), vm.extract())


# ---- 3. voxel edge cases --------------------------------------------------------------------------------------------------------
def test_voxels_without_evidence_and_exact_ties():
    scans, _, _, _ = cases.scans(False, 4)
    # a voxel of its own that saw label 0 only
    lone = map_cases.lattice([[40, 40, 40]], per_cell=3, label=0, seed=6)
    ref = map_cases.build(list(scans) + [lone], num_classes=4)
    with _vmap(4) as vm:
        _fill(vm, list(scans) + [lone])
        with pytest.raises(sicp.SicpError) as err:
            vm.extract_fused()
        assert err.value.status == sicp.ERR_NOT_READY
        vm.set_confusion(cases.matrix(4))
        plain = vm.extract_fused()
        _same_fused(plain, F.extract_fused(ref, F.log_matrix(cases.matrix(4))), vm.extract())
        assert plain["count"][-1] == 3 and plain["labels"][-1] == 0 and plain["confidence"][-1] == 0.0
        # zero entries: every class ruled out for most voxels -> label 0, confidence 0; the others have a finite posterior
        vm.set_confusion(cases.zero_matrix())
        want = F.extract_fused(ref, F.log_matrix(cases.zero_matrix()))
        out = vm.extract_fused()
        _same_fused(out, want, vm.extract())
        ruled_out = (out["labels"] == 0) & (vm.extract(want_hist=True)["hist"][:, 1:].sum(axis=1) > 0)
        assert ruled_out.sum() > 100 and (out["labels"] > 0).sum() > 100 and (out["confidence"][ruled_out] == 0).all()
        # two identical columns: classes 2 and 3 tie exactly wherever either leads, and 2 takes it (replacing the matrix
        # changes the result accordingly)
        vm.set_confusion(cases.twin_matrix())
        want = F.extract_fused(ref, F.log_matrix(cases.twin_matrix()))
        out = vm.extract_fused()
        _same_fused(out, want, vm.extract())
        assert (out["labels"] == 2).sum() > 100 and (out["labels"] == 3).sum() == 0 and (plain["labels"] == 3).sum() > 100
        tied = out["labels"] == 2
        assert (out["confidence"][tied] <= 0.5).all()


# ---- 4. the vote ----------------------------------------------------------------------------------------------------------------
def test_a_symmetric_matrix_gives_the_vote_where_the_vote_is_unique():
    xyz, lab = cases.vote_scan()
    ref = map_cases.build([(xyz, lab)], num_classes=4)
    with _vmap(4) as vm:
        _fill(vm, [(xyz, lab)])
        vm.set_confusion(cases.vote_matrix())
        vote = vm.extract(want_hist=True)
        out = vm.extract_fused()
        _same_fused(out, F.extract_fused(ref, F.log_matrix(cases.vote_matrix())), vote)
        sure = cases.vote_unique(vote["hist"])
        assert 150 < sure.sum() < 300
        assert np.array_equal(out["labels"][sure], vote["labels"][sure])
        assert (out["confidence"][sure] > 0.25).all()


# ---- 5. relabel -----------------------------------------------------------------------------------------------------------------
def _raw_fused_labels(vm, e, which=SRC, qt=None, include_own=1, min_count=1, n=None, labels=True, conf=True):
    q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    n = 2000 if n is None else n
    out_l, out_c = np.full(n, 0x5A5A5A5A, np.uint32), np.full(n, -7.0)
    st = sicp.lib().sicp_map_fused_labels(vm._m, None if e is None else e._h, which, None if q is None else q.ctypes.data_as(dp),
                                          include_own, min_count, out_l.ctypes.data_as(up) if labels else None,
                                          out_c.ctypes.data_as(dp) if conf else None)
    return st, bool((out_l == 0x5A5A5A5A).all() and (out_c == -7.0).all())


@pytest.mark.parametrize("classes", [4, 65])
@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
def test_fused_labels_of_a_scan(mode, classes):
    scans, qts, center, rng = cases.scans(True, classes)
    m, L = cases.built(True, classes)
    xyz, lab, qt = cases.probe(classes)
    e = _engine(mode)
    with _vmap(classes) as vm:
        try:
            _fill(vm, scans, qts, center, rng)
            vm.set_confusion(cases.matrix(classes))
            e.set_cloud(TGT, xyz, lab)
            before = vm.extract_fused()
            for own in (False, True):
                for min_count in cases.MIN_COUNTS:
                    want_l, want_c = F.fused_labels(m, L, xyz, lab, qt, include_own=own, min_count=min_count)
                    got_l, got_c = vm.fused_labels(e, TGT, qt, include_own=own, min_count=min_count)
                    print(f"own {own} min_count {min_count}: labels differing {int((got_l != want_l).sum())}, relabelled "
                          f"{int((got_l != lab).sum())}, largest relative confidence error "
                          f"{float(np.max(np.abs(got_c - want_c) / np.maximum(want_c, 1e-300))):.3g}")
                    assert got_l.dtype == np.uint32 and got_l.shape == (2000,) and np.array_equal(got_l, want_l)
                    assert np.allclose(got_c, want_c, rtol=RTOL, atol=0.0) and np.array_equal(got_c == 0, want_c == 0)
                    bad = ~np.isfinite(xyz).all(axis=1)
                    assert bad.sum() == 60 and (got_l[bad] == 0).all() and (got_c[bad] == 0).all()
                    if not own:  # outside every voxel, beyond the key's range: no evidence, the own label stays
                        assert np.array_equal(got_l[:14], lab[:14]) and (got_c[:14] == 0).all()
                    assert 0 < (got_l != lab).sum() < 2000 and (got_c > 0).sum() > 300
            labels_only, none = vm.fused_labels(e, TGT, qt, want_confidence=False)
            assert none is None and np.array_equal(labels_only, F.fused_labels(m, L, xyz, lab, qt)[0])
            # the identity pose is the NULL pose
            a = vm.fused_labels(e, TGT, None)
            b = vm.fused_labels(e, TGT, IDENT)
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
            assert np.array_equal(a[0], F.fused_labels(m, L, xyz, lab, None)[0])
            # a label above the classes: refused when it would count, nothing written; passed through when it does not
            high = lab.copy()
            high[1234] = classes + 1
            assert np.isfinite(xyz[1234]).all()
            e.set_cloud(SRC, xyz, high)
            st, untouched = _raw_fused_labels(vm, e, SRC, qt, include_own=1)
            assert st == sicp.ERR_BAD_LABEL and untouched
            got_l, got_c = vm.fused_labels(e, SRC, qt, include_own=False)
            want_l, want_c = F.fused_labels(m, L, xyz, high, qt, include_own=False)
            assert np.array_equal(got_l, want_l) and np.allclose(got_c, want_c, rtol=RTOL, atol=0.0)
            if mode != S:  # (a SEMANTIC handle holds no cloud without labels)
                e.set_cloud(SRC, xyz)
                got_l, got_c = vm.fused_labels(e, SRC, qt)
                want_l, want_c = F.fused_labels(m, L, xyz, None, qt)
                assert np.array_equal(got_l, want_l) and np.allclose(got_c, want_c, rtol=RTOL, atol=0.0)
                assert (got_l[got_c == 0] == 0).all() and (got_l > 0).sum() > 300
            after = vm.extract_fused()
            assert all(before[k].tobytes() == after[k].tobytes() for k in ("xyz", "labels", "count", "confidence"))
        finally:
            e.close()


def test_fused_labels_leaves_the_handle_as_it_was():
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    e = _engine(E)
    with _vmap(11, leaf=0.3) as vm:
        try:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            e.align(qt)
            idx, d2, w = e.correspondences(qt)
            acc, stats = e.accumulate(qt), e.stats()
            vm.integrate(e, TGT)
            vm.set_confusion(synth.confusion_matrix(11))
            size = vm.size()
            labels, conf = vm.fused_labels(e, SRC, qt)
            assert labels.shape == (len(src),) and (conf > 0).all()  # (every point has its own label to count)
            assert (labels == sl).mean() > 0.9
            assert vm.size() == size
            assert e.stats() == stats
            assert e.accumulate(qt).tobytes() == acc.tobytes()
            idx2, d22, w2 = e.correspondences(qt)
            assert idx2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
        finally:
            e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def _snapshot(vm, fused):
    out = vm.extract(want_hist=True)
    snap = tuple(out[k].tobytes() for k in ("xyz", "labels", "count", "hist")) + (vm.size(),)
    if fused:
        f = vm.extract_fused()
        snap += tuple(f[k].tobytes() for k in ("xyz", "labels", "count", "confidence"))
    return snap


def _dst_state(d):
    r = d.evaluate(IDENT, 4.0)
    return d.cloud_size(SRC), d.cloud_size(TGT), np.array([r[k] for k in sorted(r)], dtype=np.float64).tobytes()


def test_refusals_change_nothing():
    scans, _, _, _ = cases.scans(False, 4)
    xyz, lab, qt = cases.probe(4)
    INV, NR = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY
    nan_pose = IDENT.copy()
    nan_pose[2] = np.nan
    dp = C.POINTER(C.c_double)
    good, empty = _engine(), _engine()
    with _vmap(4) as vm, _vmap(0) as plain:
        try:
            _fill(vm, scans)
            _fill(plain, scans)
            good.set_source(xyz, lab)
            good.set_target(*scans[0])
            handle = _dst_state(good)
            lib = sicp.lib()
            # before a matrix is set
            before = _snapshot(vm, False)
            st, untouched = _raw_fused_labels(vm, good)
            assert st == NR and untouched
            with pytest.raises(sicp.SicpError) as err:
                vm.extract_fused()
            assert err.value.status == NR and _snapshot(vm, False) == before
            # matrices that are refused leave no matrix behind ...
            cm = np.array(cases.matrix(4))
            for bad in ((0, 0, -1e-3), (1, 2, np.nan), (3, 3, np.inf)):
                m = cm.copy()
                m[bad[0], bad[1]] = bad[2]
                with pytest.raises(sicp.SicpError) as err:
                    vm.set_confusion(m)
                assert err.value.status == INV and f"[{bad[0]}][{bad[1]}]" in str(err.value)
            assert lib.sicp_map_set_confusion(vm._m, 4, None) == INV
            assert lib.sicp_map_set_confusion(vm._m, 3, cm.ctypes.data_as(dp)) == INV
            assert lib.sicp_map_set_confusion(vm._m, 5, np.eye(5).ctypes.data_as(dp)) == INV
            assert lib.sicp_map_set_confusion(plain._m, 0, cm.ctypes.data_as(dp)) == INV
            assert lib.sicp_map_set_confusion(plain._m, 4, cm.ctypes.data_as(dp)) == INV
            assert _raw_fused_labels(vm, good)[0] == NR
            # ... and, once one is set, leave it as it was
            vm.set_confusion(cm)
            before = _snapshot(vm, True)
            m = cm.copy()
            m[2, 1] = -0.5
            with pytest.raises(sicp.SicpError):
                vm.set_confusion(m)
            assert lib.sicp_map_set_confusion(vm._m, 3, cm.ctypes.data_as(dp)) == INV
            assert _snapshot(vm, True) == before
            refused = [
                ("a NULL handle", INV, dict(e=None)),
                ("NULL out_labels", INV, dict(e=good, labels=False)),
                ("which 2", INV, dict(e=good, which=2)),
                ("which -1", INV, dict(e=good, which=-1)),
                ("include_own 2", INV, dict(e=good, include_own=2)),
                ("include_own -1", INV, dict(e=good, include_own=-1)),
                ("min_count 0", INV, dict(e=good, min_count=0)),
                ("a NaN pose", INV, dict(e=good, qt=nan_pose)),
                ("a slot without a cloud", NR, dict(e=empty)),
            ]
            for what, code, kw in refused:
                st, untouched = _raw_fused_labels(vm, **kw)
                assert st == code and untouched, what
                assert _snapshot(vm, True) == before and _dst_state(good) == handle, what
            st, untouched = _raw_fused_labels(plain, good)
            assert st == INV and untouched  # num_classes = 0
            with pytest.raises(sicp.SicpError) as err:
                plain.extract_fused()
            assert err.value.status == INV
            # extract_fused refuses what extract refuses, with its own name in the text
            for kw in (dict(crop_range=-1.0), dict(crop_range=np.nan), dict(crop_center=(0, np.inf, 0)), dict(dst=good, dst_which=2)):
                with pytest.raises(sicp.SicpError) as err:
                    vm.extract_fused(**kw)
                assert err.value.status == INV and lib.sicp_map_last_error(vm._m).decode().startswith("sicp_map_extract_fused: ")
            with pytest.raises(sicp.SicpError) as err:
                vm.extract_fused(min_count=10 ** 6, dst=good)
            assert err.value.status == sicp.ERR_TOO_FEW_POINTS and _dst_state(good) == handle
            assert vm.extract_fused(min_count=10 ** 6)["info"]["n_out"] == 0
            # the capacity refusal writes info and nothing else
            n1 = vm.size()[0]
            fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
            arr = [np.full(n1, 0x5A5A5A5A, np.uint32) for _ in range(5)]
            conf = np.full(n1, -7.0)
            info = sicp.SicpMapExtractInfo()
            p = sicp.default_map_extract_params()
            args = [arr[0].ctypes.data_as(fp), arr[1].ctypes.data_as(fp), arr[2].ctypes.data_as(fp), arr[3].ctypes.data_as(up),
                    arr[4].ctypes.data_as(up), conf.ctypes.data_as(dp), C.byref(info)]
            assert lib.sicp_map_extract_fused(vm._m, C.byref(p), good._h, TGT, n1 - 1, *args) == INV
            assert all((a == 0x5A5A5A5A).all() for a in arr) and (conf == -7.0).all() and _dst_state(good) == handle
            assert (info.n_out, info.n_voxels, info.has_label) == (n1, n1, 1)
            assert lib.sicp_map_extract_fused(vm._m, C.byref(p), None, TGT, n1, *args) == sicp.OK
            full = vm.extract_fused()
            assert np.array_equal(arr[3], full["labels"]) and conf.tobytes() == full["confidence"].tobytes()
            assert _snapshot(vm, True) == before
            # a good call afterwards
            got = vm.fused_labels(good, SRC, qt)
            want = F.fused_labels(cases.built(False, 4)[0], F.log_matrix(cm), xyz, lab, qt)
            assert np.array_equal(got[0], want[0]) and np.allclose(got[1], want[1], rtol=RTOL, atol=0.0)
        finally:
            good.close()
            empty.close()


# ---- 7. dst ---------------------------------------------------------------------------------------------------------------------
def _align_bits(e, init=IDENT):
    qt, st = e.align(init)
    keys = ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost")
    return qt.tobytes(), tuple(st[k] for k in keys)


@pytest.mark.parametrize("mode", [G, S], ids=["gicp", "semantic"])
def test_dst_is_what_set_target_of_the_arrays_makes_it(mode):
    src, sl, tgt, tl, _ = synth.config1_pair()
    half = len(tgt) // 2
    classes = int(tl.max())
    feeder, a, b = _engine(), _engine(mode), _engine(mode)
    with _vmap(classes, leaf=0.1) as vm:
        try:
            for part in ((tgt[:half], tl[:half]), (tgt[half:], tl[half:])):
                feeder.set_source(*part)
                vm.integrate(feeder)
            vm.set_confusion(synth.confusion_matrix(classes))
            a.set_source(src, sl)
            a.set_target(tgt[:300], tl[:300])
            out = vm.extract_fused(dst=a, dst_which=TGT)
            n_out = out["info"]["n_out"]
            assert 0 < n_out < len(tgt) and a.cloud_size(TGT) == (n_out, n_out)
            assert (out["labels"] > 0).all()
            b.set_source(src, sl)
            b.set_target(out["xyz"], out["labels"])
            assert _align_bits(a) == _align_bits(b)
        finally:
            for e in (feeder, a, b):
                e.close()


# ---- 8. determinism ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", [19, 255])
def test_two_maps_built_alike_give_the_same_bytes(classes):
    scans, qts, center, rng = cases.scans(True, classes)
    snaps = []
    for _ in range(2):
        with _vmap(classes) as vm:
            _fill(vm, scans, qts, center, rng, mode=S if classes == 19 else G)
            vm.set_confusion(cases.matrix(classes))
            f = vm.extract_fused()
            snaps.append(tuple(f[k].tobytes() for k in ("xyz", "labels", "count", "confidence")))
            g = vm.extract_fused()
            assert tuple(g[k].tobytes() for k in ("xyz", "labels", "count", "confidence")) == snaps[-1]
    assert snaps[0] == snaps[1]
