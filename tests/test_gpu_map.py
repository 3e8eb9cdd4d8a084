"""GPU tests of the persistent voxel map (sicp_map_*): integrating scans and extracting equals sicp_merge_clouds of the same
scans and tests/map_ref.py bit for bit, whatever the handles' modes; the rank merge at its edges (empty map, all voxels new
below / above / between the map's, none new, 255 / 256 / 257 rows, one long voxel); every refusal leaves every extract byte as
it was; prune and extract against the restatement; a dst slot is what sicp_set_cloud of the arrays makes it; the scan-to-map
loop has the bits of the loop that merges all scans again; two maps built alike are byte-identical."""
import importlib

import numpy as np
import pytest

import map_cases
import map_ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
LEAF, CLASSES = map_cases.LEAF, map_cases.CLASSES


def _engine(mode=G):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _vmap(leaf=LEAF, num_classes=CLASSES):
    return sicp.VoxelMap(0, sicp.default_map_params(leaf_size=leaf, num_classes=num_classes))


def _same(out, ref):
    """an extract of the library against one of the restatement (or a merge's result): bytes"""
    assert out["xyz"].dtype == np.float32 and out["xyz"].shape == ref["xyz"].shape
    assert np.array_equal(out["xyz"].view(np.uint32), ref["xyz"].view(np.uint32))
    assert np.array_equal(out["count"], ref["count"])
    assert (out["labels"] is None) == (ref["labels"] is None)
    if ref["labels"] is not None:
        assert np.array_equal(out["labels"], ref["labels"])
    if out.get("hist") is not None and ref.get("hist") is not None:
        assert out["hist"].shape == ref["hist"].shape and np.array_equal(out["hist"], ref["hist"])
    assert out["info"]["n_out"] == ref["n_out"] and out["info"]["max_voxel_points"] == ref["max_voxel_points"]


def _bytes(out):
    return tuple(None if out[k] is None else out[k].tobytes() for k in ("xyz", "labels", "count", "hist")) + \
        (out["info"]["n_out"], out["info"]["max_voxel_points"], out["info"]["n_voxels"])


def _snapshot(vm):
    return _bytes(vm.extract(want_hist=vm.num_classes > 0)), vm.size()


INFO_KEYS = ("n_in", "n_kept", "n_scan_voxels", "n_new_voxels", "n_voxels")


def _feed(vm, ref, xyz, lab, qt=None, center=None, crop_range=0.0, mode=G, which=SRC):
    """one scan through a fresh handle into the map and into the restatement; the two infos agree"""
    e = _engine(mode)
    try:
        e.set_cloud(which, xyz, lab)
        info = vm.integrate(e, which, qt, center, crop_range)
    finally:
        e.close()
    want = ref.integrate(xyz, lab if ref.C > 0 else None, qt, (0, 0, 0) if center is None else center, crop_range)
    assert {k: info[k] for k in INFO_KEYS} == want
    assert vm.size() == ref.size()
    return info


def _check(vm, ref, **kw):
    out = vm.extract(want_hist=ref.C > 0, **kw)
    want = ref.extract(kw.get("min_count", 1), kw.get("crop_center", (0, 0, 0)), kw.get("crop_range", 0.0))
    _same(out, want)
    assert out["info"]["n_voxels"] == want["n_voxels"] and out["info"]["has_label"] == want["has_label"]
    return out


# ---- 1. the one-shot merge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [False, True], ids=["nocrop", "crop"])
@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
def test_integrate_then_extract_is_the_one_shot_merge(mode, labelled, crop):
    """the four posed scans with NaN rows, from handles of one mode (SEMANTIC groups the device layout by label): the map's
    extract, the merge of the four handles and the restatement have the same bits.  Without labels the map keeps none
    (num_classes 0) and ignores the clouds' (a SEMANTIC handle needs them to hold a cloud at all)."""
    scans, qts = map_cases.four_posed()
    got_ref, merge_ref_out = map_cases.reference(True, labelled, crop)
    give_labels = labelled or mode == S
    es = []
    try:
        for i, (xyz, lab) in enumerate(scans):
            e = _engine(mode)
            e.set_cloud(i % 2, xyz, lab if give_labels else None)
            es.append((e, i % 2))
        rng = map_cases.RANGE if crop else 0.0
        with _vmap(num_classes=CLASSES if labelled else 0) as vm:
            n_points = 0
            for (e, w), qt in zip(es, qts):
                info = vm.integrate(e, w, qt, map_cases.CENTER, rng)
                n_points += info["n_kept"]
                assert info["n_in"] == e.cloud_size(w)[1] and info["n_voxels"] == vm.size()[0]
            out = vm.extract(want_hist=labelled)
            assert vm.size() == (out["info"]["n_out"], n_points)
        merged = sicp.merge_clouds(es, qts, sicp.default_merge_params(leaf_size=LEAF, crop_center=map_cases.CENTER, crop_range=rng))
        assert out["xyz"].tobytes() == merged["xyz"].tobytes() and out["count"].tobytes() == merged["count"].tobytes()
        if labelled:
            assert out["labels"].tobytes() == merged["labels"].tobytes()
            assert (out["hist"].sum(axis=1) == out["count"]).all()
        else:
            assert out["labels"] is None and out["info"]["has_label"] == 0
        assert (out["info"]["n_out"], out["info"]["max_voxel_points"]) == (merged["info"]["n_out"], merged["info"]["max_voxel_points"])
        assert n_points == merged["info"]["n_kept"]
        _same(out, got_ref)
        _same(out, merge_ref_out)
    finally:
        for e, _ in es:
            e.close()


# ---- 2. the rank merge at its edges -----------------------------------------------------------------------------------------
def _row(n, z=5, x0=0, step=1):
    return [[x0 + step * i, 0, z] for i in range(n)]


def _uniform(seed, n=1500):
    rng = np.random.default_rng(seed)
    return rng.uniform(-3, 3, (n, 3)).astype(np.float32), rng.integers(0, CLASSES + 1, n).astype(np.uint32)


def _edge_steps(name):
    """[(xyz, labels, integrate keywords)]: the scans of an edge case, in order"""
    L = map_cases.lattice
    if name == "below":  # z is the key's highest field: every voxel of the second scan sorts before the map's
        return [L(_row(40), 2), L(_row(30, z=-3), 3, label=2)]
    if name == "above":
        return [L(_row(40), 2), L(_row(30, z=9), 3, label=2)]
    if name == "interleaved":
        return [L(_row(40, step=2), 2), L(_row(40, x0=1, step=2), 1, label=3), L(_row(90, x0=-5), 1, label=4)]
    if name == "same_twice":
        s = _uniform(11)
        return [s, s]
    if name in ("rows255", "rows256", "rows257"):  # a map of exactly that many rows (one workgroup, give or take one), then more
        return [L(_row(int(name[4:])), 1), _uniform(12), L(_row(300, x0=-20), 2, label=0)]
    if name == "long_voxel":  # 700 points of one voxel in one scan (one lane's serial loop), 300 more continue its sums
        return [L([[1, -2, 0]], 700, seed=3), L([[1, -2, 0]], 300, seed=4, label=2), L([[1, -2, 0], [0, 0, 0]], 1, seed=5, label=2)]
    if name == "single_point":
        return [L([[0, 0, 0]], 1), L([[-1, -1, -1]], 1, label=4), L([[0, 0, 0]], 1, label=4)]
    if name == "negative":
        xyz, lab = _uniform(13)
        return [(xyz - np.float32(40.0), lab), (-np.abs(xyz) - np.float32(37.0), lab)]
    if name == "nan_scan":
        return [_uniform(14, 300), (np.full((257, 3), np.nan, np.float32), np.ones(257, np.uint32)), _uniform(15, 300)]
    if name == "cropped_scan":
        far = dict(center=(500.0, 0.0, 0.0), crop_range=1.0)
        return [_uniform(16, 300), _uniform(17, 300) + (far,), _uniform(18, 300) + (dict(center=(0.5, 0.0, 0.0), crop_range=2.5),)]
    raise KeyError(name)


EDGES = ("below", "above", "interleaved", "same_twice", "rows255", "rows256", "rows257", "long_voxel", "single_point", "negative",
         "nan_scan", "cropped_scan")


@pytest.mark.parametrize("name", EDGES)
def test_rank_merge_edges(name):
    ref = map_ref.Map(LEAF, CLASSES)
    with _vmap() as vm:
        empty = vm.extract(want_hist=True)
        assert empty["info"]["n_out"] == 0 and empty["xyz"].shape == (0, 3) and vm.size() == (0, 0)
        infos = []
        for step in _edge_steps(name):
            xyz, lab = step[0], step[1]
            kw = step[2] if len(step) > 2 else {}
            before = _snapshot(vm)
            infos.append(_feed(vm, ref, xyz, lab, **kw))
            if infos[-1]["n_kept"] == 0:
                assert _snapshot(vm) == before  # a scan without a finite or kept point changes nothing
            _check(vm, ref)
        if name in ("below", "above"):
            assert infos[1]["n_new_voxels"] == infos[1]["n_scan_voxels"] == 30
        if name == "same_twice":
            a = infos[0]
            assert infos[1]["n_new_voxels"] == 0 and infos[1]["n_voxels"] == a["n_voxels"] and vm.size() == (a["n_voxels"], 2 * a["n_kept"])
        if name.startswith("rows"):
            assert infos[0]["n_voxels"] == int(name[4:])
        if name == "long_voxel":
            assert _check(vm, ref)["info"]["max_voxel_points"] == 1001
        if name in ("nan_scan", "cropped_scan"):
            assert infos[1]["n_kept"] == 0 and infos[1]["n_voxels"] == infos[0]["n_voxels"]
        vm.clear()
        assert vm.size() == (0, 0) and vm.extract()["info"]["n_out"] == 0


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------
def _raw_integrate(vm, e, which=SRC, qt=None, center=None, crop_range=0.0):
    q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
    c = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    info = sicp.SicpMapIntegrateInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    st = sicp.lib().sicp_map_integrate(vm._m, None if e is None else e._h, which, None if q is None else q.ctypes.data_as(dp),
                                       None if c is None else c.ctypes.data_as(dp), crop_range, C.byref(info))
    return st, bytes(info) == b"\x5a" * C.sizeof(info)


def test_refusals_leave_every_extract_byte_unchanged():
    scans = map_cases.four()
    ref = map_ref.Map(LEAF, CLASSES)
    xyz, lab = scans[2]
    bad_label = lab.copy()
    bad_label[7] = CLASSES + 1
    far = xyz.copy()
    far[3] = (1e6, 0, 0)
    nan_pose = IDENT.copy()
    nan_pose[5] = np.nan
    INV, NR, BL = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_BAD_LABEL
    good, e_bad, e_far, e_nolab, e_empty = (_engine() for _ in range(5))
    with _vmap() as vm:
        try:
            for s in scans[:2]:
                _feed(vm, ref, *s)
            good.set_source(xyz, lab)
            e_bad.set_source(xyz, bad_label)
            e_far.set_source(far, lab)
            e_nolab.set_source(xyz)
            before = _snapshot(vm)
            refused = [
                ("label num_classes + 1", BL, dict(e=e_bad)),
                ("a point at 1e6 with leaf 0.5", INV, dict(e=e_far)),
                ("an unlabelled cloud", INV, dict(e=e_nolab)),
                ("which 2", INV, dict(e=good, which=2)),
                ("which -1", INV, dict(e=good, which=-1)),
                ("a NaN pose", INV, dict(e=good, qt=nan_pose)),
                ("a NaN centre", INV, dict(e=good, center=(0, np.nan, 0), crop_range=3.0)),
                ("an infinite centre", INV, dict(e=good, center=(np.inf, 0, 0))),
                ("a negative range", INV, dict(e=good, crop_range=-1.0)),
                ("a NaN range", INV, dict(e=good, crop_range=np.nan)),
                ("a NULL handle", INV, dict(e=None)),
                ("a slot without a cloud", NR, dict(e=e_empty)),
                ("good's empty slot", NR, dict(e=good, which=TGT)),
            ]
            for what, code, kw in refused:
                st, info_untouched = _raw_integrate(vm, **kw)
                assert st == code, what
                assert info_untouched, what
                assert _snapshot(vm) == before, what
                if what.startswith("a point at 1e6"):
                    assert "leaf size" in sicp.lib().sicp_map_last_error(vm._m).decode()
            # prune and extract refuse their own bad arguments the same way
            for center, rng in (((0, 0, 0), 0.0), ((0, 0, 0), -1.0), ((0, 0, 0), np.nan), ((np.nan, 0, 0), 2.0)):
                with pytest.raises(sicp.SicpError) as err:
                    vm.prune(center, rng)
                assert err.value.status == INV and _snapshot(vm) == before
            for kw in (dict(crop_range=-1.0), dict(crop_range=np.nan), dict(crop_center=(0, np.inf, 0)), dict(dst=good, dst_which=2)):
                with pytest.raises(sicp.SicpError) as err:
                    vm.extract(**kw)
                assert err.value.status == INV
            with _vmap(num_classes=0) as plain, pytest.raises(sicp.SicpError) as err:
                plain.extract(want_hist=True)
            assert err.value.status == INV
            # ... and the map integrates normally afterwards
            assert _raw_integrate(vm, good)[0] == sicp.OK
            ref.integrate(xyz, lab)
            _check(vm, ref)
            # memory: no new slab is allowed and the scan needs ~300K new rows.  Refused -> the map is what it was; granted (the
            # arena happened to have room) -> it holds the scan
            rng = np.random.default_rng(3)
            big = rng.uniform(-60, 60, (300_000, 3)).astype(np.float32), rng.integers(0, CLASSES + 1, 300_000).astype(np.uint32)
            good.set_source(*big)
            before = _snapshot(vm)
            sicp.set_memory_limit(0, max(sicp.memory_reserved(0), 1))
            try:
                st, _ = _raw_integrate(vm, good)
            finally:
                sicp.set_memory_limit(0, 0)
            assert st in (sicp.OK, sicp.ERR_OUT_OF_MEMORY)
            if st == sicp.ERR_OUT_OF_MEMORY:
                assert _snapshot(vm) == before
                assert _raw_integrate(vm, good)[0] == sicp.OK  # with the limit lifted it goes through
            ref.integrate(*big)
            _check(vm, ref)
        finally:
            for e in (good, e_bad, e_far, e_nolab, e_empty):
                e.close()


# ---- 4. prune and extract -----------------------------------------------------------------------------------------------------
def _dst_state(d):
    r = d.evaluate(IDENT, 4.0)
    return d.cloud_size(SRC), d.cloud_size(TGT), np.array([r[k] for k in sorted(r)], dtype=np.float64).tobytes()


def test_prune_and_extract_against_the_restatement():
    scans, qts = map_cases.four_posed()
    ref = map_ref.Map(LEAF, CLASSES)
    d = _engine()
    with _vmap() as vm:
        try:
            for s, qt in zip(scans[:3], qts):
                _feed(vm, ref, *s, qt=qt)
            # a planted tie: a voxel of its own with two points of label 3 and two of label 1 -> 1
            tie_xyz, _ = map_cases.lattice([[30, 30, 30]], 4, seed=9)
            _feed(vm, ref, tie_xyz, np.array([3, 1, 3, 1], np.uint32))
            full = _check(vm, ref)
            k = int(np.flatnonzero((full["hist"][:, 1] == 2) & (full["hist"][:, 3] == 2) & (full["count"] == 4))[-1])
            assert full["labels"][k] == 1 and (full["hist"].sum(axis=1) == full["count"]).all()
            assert np.array_equal(full["labels"], np.argmax(full["hist"], axis=1))
            n1 = full["info"]["n_out"]
            n2 = _check(vm, ref, min_count=2)["info"]["n_out"]
            n3 = _check(vm, ref, min_count=3)["info"]["n_out"]
            assert n1 > n2 > n3 > 0
            cropped = _check(vm, ref, crop_center=map_cases.CENTER, crop_range=2.0, min_count=2)
            assert 0 < cropped["info"]["n_out"] < n2
            assert _check(vm, ref, crop_range=np.inf)["info"]["n_out"] == n1
            counts_only = vm.extract(want_points=False)
            assert counts_only["xyz"] is None and counts_only["info"]["n_out"] == n1
            # the capacity refusal writes info and nothing else
            fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
            arr = [np.full(n1, 0x5A5A5A5A, np.uint32) for _ in range(5)]
            info = sicp.SicpMapExtractInfo()
            p = sicp.default_map_extract_params()
            args = [arr[0].ctypes.data_as(fp), arr[1].ctypes.data_as(fp), arr[2].ctypes.data_as(fp), arr[3].ctypes.data_as(up),
                    arr[4].ctypes.data_as(up), None, C.byref(info)]
            d.set_source(*scans[2])
            d.set_target(*scans[3])
            d_before = _dst_state(d)
            assert sicp.lib().sicp_map_extract(vm._m, C.byref(p), d._h, TGT, n1 - 1, *args) == sicp.ERR_INVALID_ARGUMENT
            assert all((a == 0x5A5A5A5A).all() for a in arr) and _dst_state(d) == d_before
            assert (info.n_out, info.max_voxel_points, info.n_voxels, info.has_label) == (n1, full["info"]["max_voxel_points"], n1, 1)
            assert sicp.lib().sicp_map_extract(vm._m, C.byref(p), None, TGT, n1, *args) == sicp.OK
            assert arr[0].view(np.float32).tobytes() == full["xyz"][:, 0].tobytes() and np.array_equal(arr[3], full["labels"])
            # an empty selection into a dst: refused, dst as it was; without a dst it is a result
            with pytest.raises(sicp.SicpError) as err:
                vm.extract(min_count=10 ** 6, dst=d)
            assert err.value.status == sicp.ERR_TOO_FEW_POINTS and _dst_state(d) == d_before
            assert vm.extract(min_count=10 ** 6)["info"]["n_out"] == 0
            # prune, then integrate again
            before = _bytes(vm.extract(want_hist=True, crop_center=map_cases.CENTER, crop_range=2.5))
            removed = vm.prune(map_cases.CENTER, 2.5)
            assert removed == ref.prune(map_cases.CENTER, 2.5) and 0 < removed < n1
            assert vm.size() == ref.size()
            after = _check(vm, ref)
            assert _bytes(after)[:-1] == before[:-1]  # the survivors' state, bit for bit (n_voxels, the last entry, went down)
            assert vm.prune(map_cases.CENTER, np.inf) == 0
            _feed(vm, ref, *scans[3], qt=qts[3])
            _check(vm, ref)
            assert vm.prune((500.0, 0.0, 0.0), 1.0) == ref.prune((500.0, 0.0, 0.0), 1.0) and vm.size() == (0, 0)
            _feed(vm, ref, *scans[0])
            _check(vm, ref)
        finally:
            d.close()


# ---- 5. dst -------------------------------------------------------------------------------------------------------------------
def _align_bits(e, init=IDENT):
    qt, st = e.align(init)
    keys = ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost")
    return qt.tobytes(), tuple(st[k] for k in keys)


@pytest.mark.parametrize("mode", [G, S], ids=["gicp", "semantic"])
def test_dst_is_what_set_target_of_the_arrays_makes_it(mode):
    src, sl, tgt, tl, _ = synth.config1_pair()
    half = len(tgt) // 2
    feeder, a, b = _engine(), _engine(mode), _engine(mode)
    with _vmap(leaf=0.1, num_classes=int(tl.max())) as vm:
        try:
            for part in ((tgt[:half], tl[:half]), (tgt[half:], tl[half:])):
                feeder.set_source(*part)
                vm.integrate(feeder)
            a.set_source(src, sl)
            a.set_target(tgt[:300], tl[:300])
            out = vm.extract(dst=a, dst_which=TGT)
            n_out = out["info"]["n_out"]
            assert 0 < n_out < len(tgt) and a.cloud_size(TGT) == (n_out, n_out)
            b.set_source(src, sl)
            b.set_target(out["xyz"], out["labels"])
            assert _align_bits(a) == _align_bits(b)
        finally:
            for e in (feeder, a, b):
                e.close()


# ---- 6. the loop it exists for ----------------------------------------------------------------------------------------------
def test_scan_to_map_loop_equals_the_loop_that_merges_every_scan_again():
    """five scans along a track, no crop.  Loop A aligns scan k to the map's extract and integrates it at the result; loop B
    aligns it to merge_clouds of scans 0..k-1 at loop A's poses.  The targets are bit-equal, so the poses are."""
    scans, _, _ = synth.lidar_sequence(seed=5, n_scans=5, n_points=4000)
    n_cls = int(max(l.max() for _, l in scans))
    holders = []
    a, b = _engine(), _engine()
    with _vmap(leaf=0.4, num_classes=n_cls) as vm:
        try:
            for xyz, lab in scans:
                e = _engine()
                e.set_source(xyz, lab)
                holders.append(e)
            poses = [IDENT.copy()]
            vm.integrate(holders[0], SRC, poses[0])
            mp = sicp.default_merge_params(leaf_size=0.4)
            for k in range(1, 5):
                a.set_source(*scans[k])
                target_a = vm.extract(dst=a, dst_which=TGT)
                qt_a, st_a = a.align(poses[-1])
                b.set_source(*scans[k])
                target_b = sicp.merge_clouds([(h, SRC) for h in holders[:k]], np.stack(poses), mp, dst=(b, TGT))
                assert target_a["xyz"].tobytes() == target_b["xyz"].tobytes() and target_a["labels"].tobytes() == target_b["labels"].tobytes()
                assert target_a["count"].tobytes() == target_b["count"].tobytes()
                qt_b, st_b = b.align(poses[-1])
                assert qt_a.tobytes() == qt_b.tobytes() and st_a["outer_iters"] == st_b["outer_iters"]
                poses.append(qt_a)
                vm.integrate(holders[k], SRC, qt_a)
            assert np.isfinite(poses[-1]).all() and np.linalg.norm(poses[-1][4:7]) > 0  # (the registrations moved the pose)
        finally:
            for e in holders + [a, b]:
                e.close()


# ---- 7. other guarantees ------------------------------------------------------------------------------------------------------
def test_two_maps_built_alike_are_byte_identical():
    scans, qts = map_cases.four_posed()
    snaps = []
    for _ in range(2):
        ref = map_ref.Map(LEAF, CLASSES)
        with _vmap() as vm:
            for s, qt in zip(scans, qts):
                _feed(vm, ref, *s, qt=qt, center=map_cases.CENTER, crop_range=map_cases.RANGE, mode=S)
            vm.prune(map_cases.CENTER, 3.0)
            snaps.append(_snapshot(vm))
    assert snaps[0] == snaps[1]


def test_integrate_leaves_the_handle_as_it_was():
    src, sl, tgt, tl, T = synth.config1_pair()
    qt = np_ref.mat_to_qt(T)
    e = _engine(E)
    with _vmap(leaf=0.3, num_classes=11) as vm:
        try:
            e.set_confusion(synth.confusion_matrix(11))
            e.set_source(src, sl)
            e.set_target(tgt, tl)
            e.align(qt)
            idx, d2, w = e.correspondences(qt)
            acc, stats = e.accumulate(qt), e.stats()
            vm.integrate(e, SRC, qt)
            vm.integrate(e, TGT)
            assert vm.size()[1] == len(src) + len(tgt)
            assert e.stats() == stats
            assert e.accumulate(qt).tobytes() == acc.tobytes()  # (the correspondences on the device are the ones from before)
            idx2, d22, w2 = e.correspondences(qt)
            assert idx2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
        finally:
            e.close()
