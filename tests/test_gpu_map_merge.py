"""GPU tests of sicp_map_merge and of sicp_map_get_state / sicp_map_set_state.  Everything is compared in the BYTES of
get_state() -- keys, float64 sums, counts, histograms -- and in info and size(), against tests/map_merge_ref.py: the identity
merge reproduces src; the exact scene equals direct integration at the composed pose (an oracle that does not go through the
restatement of the merge); general poses between maps of different leaf sizes; the rank merge at its edges and at the wave and
workgroup edges; one run of ~300 rows, whose fold order shows in the bytes; every histogram stride; crop and min_count; one test
per refusal, each leaving dst's bytes as they were and dst usable; merges interleaved with integrate, prune and carve; and a map
reloaded from its state gives the bytes of the original from every later call.  src's state is checked after every merge."""
import ctypes
import importlib

import numpy as np
import pytest

import map_carve_ref
import map_cases
import map_merge_cases as cases
import map_merge_ref as ref
import map_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
SRC, TGT = sicp.SOURCE, sicp.TARGET
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
LEAF, CLASSES = map_cases.LEAF, map_cases.CLASSES


def _engine():
    p = sicp.default_params(sicp.MODE_GICP)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _vmap(leaf=LEAF, num_classes=CLASSES):
    return sicp.VoxelMap(0, sicp.default_map_params(leaf_size=leaf, num_classes=num_classes))


def _gpu(m):
    """the library's map with exactly the rows of the restatement's"""
    return sicp.VoxelMap.from_state(ref.state(m))


def _integrate(vm, xyz, lab, qt=None):
    e = _engine()
    try:
        e.set_cloud(SRC, xyz, lab)
        return vm.integrate(e, SRC, qt)
    finally:
        e.close()


def _bytes(vm):
    return ref.state_bytes(vm.get_state())


def _same_state(vm, want):
    """get_state() of the library against a state of the restatement (or of another map): dtypes, shapes, bytes"""
    got = vm.get_state()
    assert got["key"].dtype == np.uint64 and got["sums"].dtype == np.float64 and got["sums"].shape == (len(got["key"]), 3)
    assert got["count"].dtype == np.uint32 and (got["hist"] is None) == (want["hist"] is None)
    for k in ("key", "count", "sums", "hist"):
        if want[k] is not None:
            assert got[k].shape == np.asarray(want[k]).shape, k
            assert got[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    assert vm.size() == (len(want["key"]), int(np.asarray(want["count"], np.int64).sum()))


def _merge(dst, src, kw):
    """the library's merge with the restatement's keywords; src's bytes are what they were"""
    before = _bytes(src)
    info = dst.merge(src, kw.get("qt"), kw.get("min_count", 1), kw.get("center"), kw.get("crop_range", 0.0))
    assert _bytes(src) == before
    return {k: info[k] for k in ref.INFO_KEYS}


# ---- 1. identity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_classes", [0, 3, 255])
@pytest.mark.parametrize("qt", [None, IDENT], ids=["null", "ident"])
def test_identity_merge_into_an_empty_map_reproduces_src(qt, num_classes):
    scans, qts = map_cases.four_posed()
    with _vmap(num_classes=num_classes) as src, _vmap(num_classes=num_classes) as dst:
        for (xyz, lab), pose in zip(scans, qts):
            _integrate(src, xyz, (lab % (num_classes + 1)).astype(np.uint32) if num_classes else None, pose)
        n = src.size()[0]
        assert n > 1000
        info = _merge(dst, src, dict(qt=qt))
        assert _bytes(dst) == _bytes(src) and dst.size() == src.size()
        assert info == dict(n_src_rows=n, n_kept_rows=n, n_kept_points=src.size()[1], n_touched=n, n_new_voxels=n, max_run=1, n_voxels=n)
        if num_classes:
            st = dst.get_state()
            assert (st["hist"].sum(axis=1) == st["count"]).all()


# ---- 2. the exact scene -------------------------------------------------------------------------------------------------------------
def test_exact_scene_equals_direct_integration_at_the_composed_pose():
    """points at (k + 0.5) 2^-10, leaf 0.25, a half turn about z and a translation by whole voxels: every sum is exact, so the
    submap merged at the pose and the scans integrated at the composed poses hold the same bytes"""
    scans, inner = cases.exact_scans()
    composed = cases.exact_composed()
    kw = dict(leaf=cases.EXACT_LEAF, num_classes=cases.EXACT_CLASSES)
    with _vmap(**kw) as sub, _vmap(**kw) as dst, _vmap(**kw) as direct:
        for (xyz, lab), a, b in zip(scans, inner, composed):
            _integrate(sub, xyz, lab, a)
            _integrate(direct, xyz, lab, b)
        info = _merge(dst, sub, dict(qt=cases.HALF_TURN))
        assert info["n_kept_points"] == 4500 and info["max_run"] == 1 and info["n_touched"] == info["n_new_voxels"] == sub.size()[0] > 400
        assert _bytes(dst) == _bytes(direct)
        assert dst.get_state()["key"].tobytes() != sub.get_state()["key"].tobytes()
        want = map_cases.build(scans, composed, **kw)
        _same_state(dst, ref.state(want))


# ---- 3. general poses, rank-merge edges, class counts, crop and min_count against the restatement -------------------------------------
@pytest.mark.parametrize("name", cases.ALL)
def test_merge_against_the_restatement(name):
    src_ref, dst_ref, kw = cases.case(name)
    want, want_info = cases.reference(name)
    with _gpu(src_ref) as src, _gpu(dst_ref) as dst:
        before = _bytes(dst)
        info = _merge(dst, src, kw)
        assert info == want_info
        _same_state(dst, want)
        if want_info["n_kept_rows"] == 0:
            assert _bytes(dst) == before
        if name == "long_run":  # the run's rows added in descending order give other sums: a split or reordered fold shows
            ref.merge(dst_ref, src_ref, descending=True, **kw)
            other = ref.state(dst_ref)
            assert other["key"].tobytes() == want["key"].tobytes() and other["sums"].tobytes() != want["sums"].tobytes()
            assert dst.get_state()["sums"].tobytes() != other["sums"].tobytes()


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(dst, src, text, status=None, **kw):
    """the merge is refused with `text` in the message; dst and src hold their bytes; a following merge works"""
    d0, s0, size0 = _bytes(dst), _bytes(src), dst.size()
    with pytest.raises(sicp.SicpError) as e:
        dst.merge(src, **kw)
    assert e.value.status == (sicp.ERR_INVALID_ARGUMENT if status is None else status)
    assert text in str(e.value), str(e.value)
    assert _bytes(dst) == d0 and _bytes(src) == s0 and dst.size() == size0


def _pair(name="g_0.2_0.2_full"):
    src_ref, dst_ref, kw = cases.case(name)
    return _gpu(src_ref), _gpu(dst_ref), kw, cases.reference(name)


def _still_works(dst, src, kw, want):
    assert _merge(dst, src, kw) == want[1]
    _same_state(dst, want[0])


def test_refused_null_maps():
    src, dst, kw, want = _pair()
    with src, dst:
        lib = sicp.lib()
        before = _bytes(dst)
        assert lib.sicp_map_merge(None, src._m, None, None, None) == sicp.ERR_INVALID_ARGUMENT
        assert lib.sicp_map_merge(dst._m, None, None, None, None) == sicp.ERR_INVALID_ARGUMENT
        assert b"src is NULL" in lib.sicp_map_last_error(dst._m) and _bytes(dst) == before
        _still_works(dst, src, kw, want)


def test_refused_src_is_dst():
    src, dst, kw, want = _pair()
    with src, dst:
        _refused(dst, dst, "the same map")
        _still_works(dst, src, kw, want)


def test_refused_maps_on_different_devices():
    """needs a second device to make the second map on; with one device the creation of that map is what is refused"""
    src, dst, kw, want = _pair()
    with src, dst:
        if sicp.device_count() > 1:
            with sicp.VoxelMap(1, sicp.default_map_params(leaf_size=0.2, num_classes=CLASSES)) as other:
                _refused(dst, other, "device")
        else:
            with pytest.raises(sicp.SicpError):
                sicp.VoxelMap(1, sicp.default_map_params(leaf_size=0.2, num_classes=CLASSES))
        _still_works(dst, src, kw, want)


@pytest.mark.parametrize("what, text, bad", [
    ("pose_nan", "pose is not finite", dict(qt=[0, 0, 0, 1, np.nan, 0, 0])),
    ("pose_inf", "pose is not finite", dict(qt=[0, 0, np.inf, 1, 0, 0, 0])),
    ("centre_nan", "crop_center must be finite", dict(crop_center=(0.0, np.nan, 0.0), crop_range=5.0)),
    ("centre_inf", "crop_center must be finite", dict(crop_center=(np.inf, 0.0, 0.0))),
    ("range_negative", "crop_range must be >= 0", dict(crop_range=-1.0)),
    ("range_nan", "crop_range must be >= 0", dict(crop_range=np.nan)),
    ("min_count_0", "min_count must be >= 1", dict(min_count=0)),
    ("min_count_negative", "min_count must be >= 1", dict(min_count=-3)),
], ids=lambda v: v if isinstance(v, str) and " " not in v else "")
def test_refused_arguments(what, text, bad):
    src, dst, kw, want = _pair()
    with src, dst:
        _refused(dst, src, text, **bad)
        _still_works(dst, src, kw, want)


@pytest.mark.parametrize("src_classes", [0, 3, 5])
def test_refused_class_mismatch(src_classes):
    src, dst, kw, want = _pair()
    with src, dst, _vmap(0.2, src_classes) as odd:
        xyz, lab = map_cases.four()[0]
        _integrate(odd, xyz, (lab % (src_classes + 1)).astype(np.uint32) if src_classes else None)
        _refused(dst, odd, f"src keeps {src_classes} classes, dst {CLASSES}")
        _still_works(dst, src, kw, want)


def test_refused_range_overflow_names_dsts_leaf():
    """a far translation onto a fine grid: the moved rows' voxel coordinates pass 2^20"""
    src_ref, dst_ref, kw = cases.case("g_0.2_0.2_empty")
    with _gpu(src_ref) as src, _vmap(0.001) as dst:
        xyz, lab = map_cases.four()[0]
        _integrate(dst, xyz, lab)
        far = np.array([0, 0, 0, 1, 2000.0, 0, 0])
        _refused(dst, src, "leaf size 0.001", qt=far)
        with pytest.raises(ref.Refused):
            ref.merge(map_ref.Map(0.001, CLASSES), src_ref, far)
        ok = dst.merge(src, IDENT)
        assert ok["n_kept_rows"] == src.size()[0] and dst.size()[1] == len(xyz) + src.size()[1]


@pytest.mark.parametrize("num_classes", [0, 2])
def test_refused_more_than_2_32_minus_1_points(num_classes):
    """two set_state rows of 2^31 points each, one in either map: no large cloud is needed"""
    big = 1 << 31
    key = ref.state(map_cases.build([map_cases.lattice([[1, 2, 3]], 1, label=1)], num_classes=num_classes))["key"]
    one = dict(key=key, sums=np.array([[0.6 * big, 1.2 * big, 1.7 * big]]), count=np.array([big], np.uint32),
               hist=np.array([[0, big - 1, 1]], np.uint32) if num_classes else None, leaf_size=LEAF, num_classes=num_classes)
    with sicp.VoxelMap.from_state(one) as src, sicp.VoxelMap.from_state(one) as dst, _vmap(num_classes=num_classes) as empty:
        assert dst.size() == (1, big)
        _refused(dst, src, "2^32 - 1 points")
        info = empty.merge(src)  # the same rows into a map with room
        assert info["n_kept_points"] == big and empty.size() == (1, big) and _bytes(empty) == _bytes(src)
        less = dict(one, count=np.array([big - 1], np.uint32), hist=np.array([[0, big - 2, 1]], np.uint32) if num_classes else None)
        with sicp.VoxelMap.from_state(less) as under:
            assert dst.merge(under)["n_kept_points"] == big - 1 and dst.size() == (1, 2 * big - 1)  # exactly 2^32 - 1 fits
            assert dst.get_state()["count"].tolist() == [2 * big - 1]


def test_refused_by_the_arena_leaves_dst_as_it_was():
    """no new slab is allowed and the merge needs scratch and rows for ~290K voxels: refused -> dst holds its bytes and the merge
    goes through once the limit is lifted; granted (the arena happened to have room) -> dst holds the rows.  Either way it ends
    equal to the restatement."""
    rng = np.random.default_rng(3)
    big = rng.uniform(-60, 60, (300_000, 3)).astype(np.float32), rng.integers(0, CLASSES + 1, 300_000).astype(np.uint32)
    src_ref = map_cases.build([big])
    _, dst_ref, _ = cases.case("g_0.2_0.2_full")
    dst_ref = ref.from_state(dict(ref.state(dst_ref), leaf_size=LEAF))  # (the same rows on src's grid: the keys are what they are)
    with _gpu(src_ref) as src, _gpu(dst_ref) as dst:
        before = _bytes(dst)
        sicp.set_memory_limit(0, max(sicp.memory_reserved(0), 1))
        status = sicp.OK
        try:
            dst.merge(src, cases.GENERAL_POSE)
        except sicp.SicpError as err:
            status = err.status
        finally:
            sicp.set_memory_limit(0, 0)
        assert status in (sicp.OK, sicp.ERR_OUT_OF_MEMORY)
        if status == sicp.ERR_OUT_OF_MEMORY:
            assert _bytes(dst) == before
            dst.merge(src, cases.GENERAL_POSE)
        ref.merge(dst_ref, src_ref, cases.GENERAL_POSE)
        _same_state(dst, ref.state(dst_ref))


# ---- 5. interleaved with the other calls ----------------------------------------------------------------------------------------------
def test_interleaved_with_integrate_prune_and_carve():
    """integrate, merge, prune, integrate, carve, merge on two library maps and on the restatement, driven alike"""
    scans, qts = map_cases.four_posed()
    sub_a = map_cases.build(scans[:2], qts[:2], leaf=0.25)
    sub_b = map_cases.build(scans[2:], qts[2:], leaf=1.0)
    pose_a, pose_b = cases.GENERAL_POSE, cases.pose(-40.0, (0.0, 0.3, 1.0), (-0.5, 0.8, 0.1))
    extra = [map_cases.four()[i] for i in (0, 1)]
    rm = map_ref.Map(LEAF, CLASSES)
    carve_lib, carve_ref = sicp.default_map_carve_params(min_rays=1), map_carve_ref.defaults(min_rays=1)
    with _gpu(sub_a) as a, _gpu(sub_b) as b, _vmap() as m1, _vmap() as m2:
        hist_a, hist_b = (s.get_state()["hist"].sum(axis=0, dtype=np.int64) for s in (a, b))

        def both(step):
            out = [step(m) for m in (m1, m2)]
            assert _bytes(m1) == _bytes(m2)
            return out[0]

        def merge_step(sub, sub_ref, pose, hist_sub):
            points, cols = m1.size()[1], m1.get_state()["hist"].sum(axis=0, dtype=np.int64) if m1.size()[0] else 0
            info = both(lambda m: _merge(m, sub, dict(qt=pose)))
            assert info == ref.merge(rm, sub_ref, pose)
            assert m1.size()[1] == points + info["n_kept_points"]
            assert np.array_equal(m1.get_state()["hist"].sum(axis=0, dtype=np.int64), cols + hist_sub)

        both(lambda m: _integrate(m, *extra[0]))
        rm.integrate(*extra[0])
        merge_step(a, sub_a, pose_a, hist_a)
        _same_state(m1, ref.state(rm))
        assert both(lambda m: m.prune((0.2, 0.1, 0.0), 3.0)) == rm.prune((0.2, 0.1, 0.0), 3.0) > 0
        both(lambda m: _integrate(m, *extra[1], qts[1]))
        rm.integrate(*extra[1], qts[1])
        _same_state(m1, ref.state(rm))

        def carve(m):
            e = _engine()
            try:
                e.set_cloud(SRC, extra[0][0], extra[0][1])
                return m.carve(e, SRC, qts[2], (0.0, 0.0, 0.5), carve_lib)["info"]["n_removed"]
            finally:
                e.close()

        assert both(carve) == map_carve_ref.carve(rm, extra[0][0], qts[2], (0.0, 0.0, 0.5), carve_ref)["info"]["n_removed"] > 0
        _same_state(m1, ref.state(rm))
        merge_step(b, sub_b, pose_b, hist_b)
        _same_state(m1, ref.state(rm))
        _same_state(m2, ref.state(rm))


# ---- 6. the state -------------------------------------------------------------------------------------------------------------------
def _out_bytes(d):
    return tuple((k, None if v is None else (v.tobytes() if isinstance(v, np.ndarray) else {a: b for a, b in v.items() if a != "t_total_ms"}))
                 for k, v in sorted(d.items()))


def test_a_reloaded_map_answers_as_the_original():
    scans, qts = map_cases.four_posed()
    sub = map_cases.build(scans[2:], qts[2:], leaf=0.25)
    ends = sicp.lidar_ray_ends(8, 90, -20.0, 20.0, 6.0)
    with _vmap() as orig, _gpu(sub) as src:
        for (xyz, lab), pose in zip(scans[:2], qts[:2]):
            _integrate(orig, xyz, lab, pose)
        state = orig.get_state()
        assert state["leaf_size"] == LEAF and state["num_classes"] == CLASSES and len(state["key"]) == orig.size()[0] > 1000
        with sicp.VoxelMap.from_state(state) as copy:
            assert _bytes(copy) == _bytes(orig) and copy.size() == orig.size()
            for m in (orig, copy):
                m.set_confusion(synth.confusion_matrix(CLASSES))
            for step in range(2):  # as loaded, then after an integrate and a merge on both
                assert _out_bytes(orig.extract(want_hist=True)) == _out_bytes(copy.extract(want_hist=True))
                assert _out_bytes(orig.extract(min_count=2, crop_center=(0.3, 0.0, 0.1), crop_range=2.0)) == \
                    _out_bytes(copy.extract(min_count=2, crop_center=(0.3, 0.0, 0.1), crop_range=2.0))
                assert _out_bytes(orig.extract_fused()) == _out_bytes(copy.extract_fused())
                assert _out_bytes(orig.raycast(ends, qts[1], (0.0, 0.0, 0.2))) == _out_bytes(copy.raycast(ends, qts[1], (0.0, 0.0, 0.2)))
                if step == 0:
                    infos = [(_integrate(m, *scans[3], qts[3]), _merge(m, src, dict(qt=cases.GENERAL_POSE))) for m in (orig, copy)]
                    assert {k: v for k, v in infos[0][0].items() if k != "t_total_ms"} == {k: v for k, v in infos[1][0].items() if k != "t_total_ms"}
                    assert infos[0][1] == infos[1][1]
                    assert _bytes(copy) == _bytes(orig)


def test_set_state_refusals_name_the_row_and_change_nothing():
    st, _ = cases.reference("g_0.2_0.2_full")
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
    n = len(st["key"])

    def broken(**change):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
        for k, (row, value) in change.items():
            bad[k][row] = value
        return bad

    unsorted = broken(key=(5, st["key"][6]))
    unsorted["key"][6] = st["key"][5]
    off_by_one = broken(hist=((2, 1), st["hist"][2, 1] + 1))
    bad_states = [("unsorted", unsorted), ("duplicate", broken(key=(9, st["key"][8]))),
                  ("zero_field", broken(key=(n - 1, (st["key"][n - 1] & ~np.uint64(0x1fffff << 21))))),
                  ("top_bit", broken(key=(n - 1, st["key"][n - 1] | np.uint64(1 << 63)))), ("zero_count", broken(count=(7, 0))),
                  ("nan_sum", broken(sums=((3, 1), np.nan))), ("inf_sum", broken(sums=((n - 1, 2), np.inf))), ("hist_off_by_one", off_by_one)]
    with _vmap(0.2) as vm:
        xyz, lab = map_cases.four()[0]
        _integrate(vm, xyz, lab)
        before = _bytes(vm)
        for what, bad in bad_states:
            with pytest.raises(ref.BadState) as want:
                ref.check_state(bad)
            with pytest.raises(sicp.SicpError) as e:
                vm.set_state(bad)
            assert e.value.status == sicp.ERR_INVALID_ARGUMENT, what
            assert f"row {want.value.row}:" in str(e.value), (what, str(e.value))
            assert _bytes(vm) == before, what
        vm.set_state(st)  # and it is still usable
        _same_state(vm, st)
        with pytest.raises(ValueError):
            vm.set_state(dict(st, num_classes=3))
        # hist for a map without classes, no hist for a map with
        lib, kp, dp, up = sicp.lib(), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
        args = (st["key"].ctypes.data_as(kp), st["sums"].ctypes.data_as(dp), st["count"].ctypes.data_as(up))
        assert lib.sicp_map_set_state(vm._m, n, *args, None) == sicp.ERR_INVALID_ARGUMENT
        assert lib.sicp_map_set_state(vm._m, n, None, args[1], args[2], st["hist"].ctypes.data_as(up)) == sicp.ERR_INVALID_ARGUMENT
        assert lib.sicp_map_set_state(vm._m, -1, *args, st["hist"].ctypes.data_as(up)) == sicp.ERR_INVALID_ARGUMENT
        with _vmap(0.2, 0) as plain:
            assert lib.sicp_map_set_state(plain._m, n, *args, st["hist"].ctypes.data_as(up)) == sicp.ERR_INVALID_ARGUMENT
            assert plain.size() == (0, 0)
            assert lib.sicp_map_set_state(plain._m, n, *args, None) == sicp.OK and plain.size() == vm.size()
        _same_state(vm, st)
        vm.set_state(dict(st, key=st["key"][:0], sums=st["sums"][:0], count=st["count"][:0], hist=st["hist"][:0]))  # n = 0 clears
        assert vm.size() == (0, 0) and len(vm.get_state()["key"]) == 0
        assert vm.extract()["info"]["n_out"] == 0


def test_get_state_capacity_rules():
    st, _ = cases.reference("n257")
    n = len(st["key"])
    lib, kp, dp, up = sicp.lib(), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    with sicp.VoxelMap.from_state(st) as vm, _vmap(LEAF, 0) as plain:
        rows = ctypes.c_int64(-1)
        assert lib.sicp_map_get_state(vm._m, 0, None, None, None, None, ctypes.byref(rows)) == sicp.OK and rows.value == n
        assert lib.sicp_map_get_state(vm._m, 0, None, None, None, None, None) == sicp.OK
        key, count = np.full(n + 3, 7, np.uint64), np.full(n + 3, 7, np.uint32)
        sums, hist = np.full((n + 3, 3), 7.0), np.full((n + 3, CLASSES + 1), 7, np.uint32)
        rows.value = -1
        assert lib.sicp_map_get_state(vm._m, n - 1, key.ctypes.data_as(kp), None, None, None, ctypes.byref(rows)) == sicp.ERR_INVALID_ARGUMENT
        assert rows.value == n and (key == 7).all() and b"rows" in lib.sicp_map_last_error(vm._m)
        assert lib.sicp_map_get_state(vm._m, n - 1, None, None, None, hist.ctypes.data_as(up), None) == sicp.ERR_INVALID_ARGUMENT and (hist == 7).all()
        # each array alone, and a capacity above the row count: the rows are written, the tail is not touched
        assert lib.sicp_map_get_state(vm._m, n + 3, key.ctypes.data_as(kp), None, None, None, None) == sicp.OK
        assert key[:n].tobytes() == st["key"].tobytes() and (key[n:] == 7).all() and (count == 7).all() and (sums == 7.0).all()
        assert lib.sicp_map_get_state(vm._m, n, None, sums.ctypes.data_as(dp), count.ctypes.data_as(up), hist.ctypes.data_as(up), None) == sicp.OK
        assert sums[:n].tobytes() == st["sums"].tobytes() and count[:n].tobytes() == st["count"].tobytes()
        assert hist[:n].tobytes() == st["hist"].tobytes() and (sums[n:] == 7.0).all() and (hist[n:] == 7).all()
        # histograms of a map that keeps none
        _integrate(plain, *map_cases.four()[0])
        before = _bytes(plain)
        assert lib.sicp_map_get_state(plain._m, 1 << 20, None, None, None, hist.ctypes.data_as(up), ctypes.byref(rows)) == sicp.ERR_INVALID_ARGUMENT
        assert rows.value == plain.size()[0] and b"no labels" in lib.sicp_map_last_error(plain._m) and _bytes(plain) == before
        assert plain.get_state()["hist"] is None
