"""GPU tests of the distance field (sicp_map_distance), everything compared for equal bytes against tests/distance_ref.py: every
array and the info of every case of tests/distance_cases.py on VoxelMap.from_state of its rows; the same on a map built by
integrate of synthetic scans, in 3-D and planar; the map's state is the same before and after; two calls give the same bytes;
every output alone; every refusal leaves the outputs and the map as they were; the point outputs on every handle mode, slot and
layout and on a cloud with dropped points, with the handle left as it was; and a cell's bytes do not depend on the window."""
import gc
import importlib
import math

import numpy as np
import pytest

import distance_cases as cases
import distance_ref as ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
INV, NR, OOM = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY, sicp.ERR_OUT_OF_MEMORY
ALL = ref.CELL_ARRAYS + ref.POINT_ARRAYS


def _engine(mode=G, num_classes=11):
    p = sicp.default_params(mode)
    p.num_classes = num_classes
    return sicp.Engine(0, p)


def _params(p):
    kw = {k: v for k, v in p.items() if k not in ("ignore", "only", "nx", "ny", "nz")}
    return sicp.default_map_distance_params(ignore=p["ignore"], only=p["only"], **kw)


def _same(got, want, what=""):
    arrays = [(k, dt) for k, dt in ALL if k in want]
    assert set(got) == set(want), what
    for k, dt in arrays:
        assert got[k].dtype == dt and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero(got[k].reshape(-1) != want[k].reshape(-1))[:5])
    assert {k: got["info"][k] for k in ref.INFO} == want["info"], what


def _state_bytes(st):
    return tuple(None if st[k] is None else st[k].tobytes() for k in ("key", "sums", "count", "hist"))


def _run_case(c, vm, engine=None, which=SRC):
    return vm.distance(c["center"], c["shape"], _params(c["params"]), engine, which, c["qt"])


# ---- 1. the cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_equals_the_restatement(name):
    c = cases.case(name)
    want = cases.reference(name)
    with sicp.VoxelMap.from_state(c["state"]) as vm:
        before = _state_bytes(vm.get_state())
        if c["points"] is None:
            got = _run_case(c, vm)
        else:
            with _engine() as e:
                e.set_source(c["points"], c["point_labels"])
                got = _run_case(c, vm, e)
        _same(got, want, name)
        c["expect"](got)
        assert _state_bytes(vm.get_state()) == before == _state_bytes(c["state"])
        if c["points"] is None:
            _same(_run_case(c, vm), want, name + " again")


# ---- 2. a map built by integrate -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def street_map():
    """three scans of the synthetic street at their poses in a map of leaf 0.25 with 11 classes; its state"""
    scans, poses, _ = synth.lidar_sequence(seed=5, n_scans=3, n_points=6000)
    vm = sicp.VoxelMap(0, sicp.default_map_params(leaf_size=0.25, num_classes=11))
    with _engine(E) as e:
        for (xyz, lab), T in zip(scans, poses):
            e.set_source(xyz, lab)
            vm.integrate(e, SRC, np_ref.mat_to_qt(T))
    yield vm, vm.get_state(), scans, poses
    vm.close()


@pytest.mark.parametrize("planar", [0, 1])
def test_an_integrated_map_equals_the_restatement(street_map, planar):
    vm, state, scans, poses = street_map
    assert len(state["key"]) > 5000
    shape = (121, 96, 1) if planar else (121, 96, 24)
    kw = dict(nx=shape[0], ny=shape[1], nz=shape[2], max_dist_voxels=10, ignore=(3, 4), min_count=2, planar=planar)
    if planar:
        kw.update(z_min=0.3, z_max=1.8)
    centre = (1.3, -0.4, 1.9)
    xyz, lab = scans[2]
    qt = np_ref.mat_to_qt(poses[2])
    want = ref.distance(state, ref.defaults(**kw), centre, xyz, qt)
    assert want["info"]["n_obstacles"] > 100 and 0 < want["info"]["n_reached"] < want["dist_sq"].size
    assert (want["point_cell"] >= 0).sum() > len(xyz) // 4 and (want["point_dist_sq"] > 0).sum() > 20
    with _engine(E) as e:
        e.set_source(xyz, lab)
        got = vm.distance(centre, shape, _params(ref.defaults(**kw)), e, SRC, qt)
    _same(got, want, planar)
    assert _state_bytes(vm.get_state()) == _state_bytes(state)


# ---- 3. the contracts -------------------------------------------------------------------------------------------------------------
def p_with_window(p, c):
    q = sicp.SicpMapDistanceParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    q.nx, q.ny, q.nz = c["shape"]
    return q


def test_each_output_alone():
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    with sicp.VoxelMap.from_state(c["state"]) as vm, _engine() as e:
        e.set_source(c["points"], c["point_labels"])
        p = _params(c["params"])
        for k, _ in ALL:
            got = vm.distance(c["center"], c["shape"], p, e, SRC, c["qt"], want=(k,))
            assert set(got) == {k, "info"} and got[k].tobytes() == want[k].tobytes(), k
            assert {q: got["info"][q] for q in ref.INFO} == want["info"], k
        info = sicp.SicpMapDistanceInfo()  # no out struct at all: the counts are there
        ctr = np.array(c["center"])
        assert sicp.lib().sicp_map_distance(vm._m, sicp._ptr(ctr, sicp._dp), C.byref(p_with_window(p, c)), None, None, 0, None, C.byref(info)) == sicp.OK
        for k in ("n_obstacles", "n_reached", "max_dist_sq", "x0", "y0", "z0"):
            assert getattr(info, k) == want["info"][k], k
        assert info.n_points == 0 and info.n_points_inside == 0


SENTINEL = 0x5A


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_cells, n_points):
        self.bufs = {k: np.full(np.dtype(dt).itemsize * max(n_points if (k, dt) in ref.POINT_ARRAYS else n_cells, 1), SENTINEL, np.uint8)
                     for k, dt in ALL}
        self.out = sicp.SicpMapDistanceOut()
        types = dict(sicp.SicpMapDistanceOut._fields_)
        for k, a in self.bufs.items():
            setattr(self.out, k, a.ctypes.data_as(types[k]))
        self.info = sicp.SicpMapDistanceInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, vm, center, p, h=None, which=SRC, qt=None, points=True, range_sq=True):
        out = sicp.SicpMapDistanceOut()
        C.memmove(C.byref(out), C.byref(self.out), C.sizeof(out))
        if not points:
            out.point_cell, out.point_dist_sq, out.point_nearest, out.point_range_sq = None, None, None, None
        if not range_sq:
            out.point_range_sq = None
        ctr = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
        return sicp.lib().sicp_map_distance(None if vm is None else vm._m, sicp._ptr(ctr, sicp._dp), None if p is None else C.byref(p),
                                            C.byref(out), None if h is None else h._h, which, sicp._ptr(q, sicp._dp), C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.bufs.values()) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_every_refusal_writes_nothing_and_leaves_the_map_usable():
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    nx, ny, nz = c["shape"]

    def params(**kw):
        lists = {k: kw.pop(k, ()) for k in ("ignore", "only")}
        return sicp.default_map_distance_params(**lists, **{**dict(nx=nx, ny=ny, nz=nz, max_dist_voxels=1), **kw})

    with sicp.VoxelMap.from_state(c["state"]) as vm, _engine() as e, _engine() as e_empty, \
            sicp.VoxelMap.from_state(cases.patch_state(0)) as vm0:
        e.set_source(c["points"], c["point_labels"])
        before = _state_bytes(vm.get_state())
        raw = _Raw(nx * ny * nz, len(c["points"]))
        ok = params()
        refused = [(what, INV, dict(p=params(**kw))) for what, kw in cases.REFUSED.items()]
        n65 = params()
        n65.n_only = 65
        neg = params()
        neg.n_ignore = -1
        far = 0.5 * (1 << 20)
        refused += [
            ("n_only 65", INV, dict(p=n65)), ("n_ignore -1", INV, dict(p=neg)),
            ("NULL params", INV, dict(p=None)), ("NULL centre", INV, dict(center=None)),
            ("a centre that is NaN", INV, dict(center=(math.nan, 0.0, 0.0))), ("a centre that is infinite", INV, dict(center=(0.0, 0.0, math.inf))),
            ("a centre beyond the key's range", INV, dict(center=(0.0, 0.0, far))),
            ("a planar centre whose z is not finite", INV, dict(center=(0.0, 0.0, math.nan), p=params(nz=1, planar=1), range_sq=False)),
            ("a pose that is not finite", INV, dict(qt=[0, 0, 0, 1, 0, math.nan, 0])),
            ("a pose that is not finite, without a handle", INV, dict(qt=[0, 0, math.inf, 1, 0, 0, 0], h=None, points=False)),
            ("which = 2", INV, dict(which=2)), ("which = -1", INV, dict(which=-1)),
            ("point outputs without a handle", INV, dict(h=None)),
            ("point_range_sq in planar mode", INV, dict(p=params(nz=1, planar=1))),
            ("a slot without a cloud", NR, dict(h=e_empty)), ("the handle's empty slot", NR, dict(which=TGT)),
            ("an ignore list on a map without classes", INV, dict(vm=vm0, p=params(ignore=(0,)))),
            ("an only list on a map without classes", INV, dict(vm=vm0, p=params(only=(0,)))),
        ]
        for what, code, kw in refused:
            args = dict(vm=vm, center=c["center"], p=ok, h=e, which=SRC, qt=c["qt"])
            args.update(kw)
            assert raw.call(**args) == code, what
            assert raw.untouched(), what
            assert sicp.lib().sicp_map_last_error(args["vm"]._m).decode().startswith("sicp_map_distance: "), what
        assert raw.call(None, c["center"], ok, e) == INV and raw.untouched()  # a NULL map
        assert raw.call(vm, (0.0, 0.0, far), params(nz=1, planar=1), e, qt=c["qt"], range_sq=False) == sicp.OK  # (planar: z is not keyed)
        assert _state_bytes(vm.get_state()) == before
        _same(_run_case(c, vm, e), want, "after the refusals")
        # a memory limit: the arena is trimmed to the slabs that hold live blocks and may take no new one, and a 2^24-cell call
        # needs two 8-byte key buffers of 16 Mi cells, 268 MB, before anything else.  While the arena holds less than that the
        # refusal is certain and is asserted; nothing is written and the map answers afterwards.  (An arena that other live
        # objects of the process keep larger may have the room: then the call may also be granted.)
        gc.collect()
        assert sicp.lib().sicp_release_pool(0) == sicp.OK
        reserved = sicp.memory_reserved(0)
        sicp.set_memory_limit(0, max(reserved, 1))
        try:
            big = params(nx=1024, ny=1024, nz=16)
            raw2 = _Raw(1 << 24, 1)
            st = raw2.call(vm, c["center"], big, None, points=False)
        finally:
            sicp.set_memory_limit(0, 0)
        print("memory limit: reserved", reserved, "status", st)
        assert st == OOM if reserved < 2 * 8 * (1 << 24) else st in (sicp.OK, OOM)
        if st == OOM:
            assert raw2.untouched() and "sicp_map_distance" in sicp.lib().sicp_map_last_error(vm._m).decode()
        assert _state_bytes(vm.get_state()) == before
        _same(_run_case(c, vm, e), want, "after the memory limit")


def test_the_points_on_every_mode_slot_and_layout_and_the_handle_untouched():
    """the point outputs are the restatement's on a GICP, an EM and a SEMANTIC handle (which groups its device layout by label),
    from either slot, before and after an align() has laid the clouds out; and a handle that made the calls aligns to the bytes
    of a twin that never did"""
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    assert not np.isfinite(c["points"]).all()  # a cloud with dropped points: the finite ones go through their caller indices
    with sicp.VoxelMap.from_state(c["state"]) as vm:
        for mode in (G, E, S):
            for which in (SRC, TGT):
                with _engine(mode) as e:
                    e.set_cloud(which, c["points"], c["point_labels"])
                    _same(_run_case(c, vm, e, which), want, (mode, which))
        src, sl, tgt, tl, T = synth.config1_pair()
        qt = np_ref.mat_to_qt(T)
        st = cases.patch_state()
        shape = (40, 40, 12)
        kw = dict(nx=40, ny=40, nz=12, max_dist_voxels=3)
        centre = (float(src[:, 0].mean()), float(src[:, 1].mean()), float(src[:, 2].mean()))
        want_pair = {w: ref.distance(st, ref.defaults(**kw), centre, pts, qt) for w, pts in ((SRC, src), (TGT, tgt))}
        assert (want_pair[SRC]["point_cell"] >= 0).sum() > 100
        p = _params(ref.defaults(**kw))
        with sicp.VoxelMap.from_state(st) as vp:
            for mode in (E, S):
                res = []
                for with_calls in (False, True):
                    with _engine(mode) as e:
                        e.set_confusion(synth.confusion_matrix(11))
                        e.set_source(src, sl)
                        e.set_target(tgt, tl)
                        if with_calls:  # before anything is on the device in a layout
                            _same(vp.distance(centre, shape, p, e, SRC, qt), want_pair[SRC], (mode, "before align"))
                        first = e.align(qt)
                        idx, d2, w = e.correspondences(qt)
                        stats = e.stats()
                        if with_calls:
                            _same(vp.distance(centre, shape, p, e, SRC, qt), want_pair[SRC], (mode, "laid out"))
                            _same(vp.distance(centre, shape, p, e, TGT, qt), want_pair[TGT], (mode, "laid out, target"))
                            assert e.stats() == stats
                        second = e.align(qt)
                        drop = lambda s: {k: v for k, v in s.items() if not k.startswith("t_") and not k.endswith("_ms")}
                        res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), drop(first[1]),
                                    drop(second[1])))
                assert res[0] == res[1], mode


def test_a_cells_bytes_do_not_depend_on_the_window(street_map):
    vm, state, _, _ = street_map
    R = 7
    p = sicp.default_map_distance_params(max_dist_voxels=R, ignore=(3,))
    a = vm.distance((0.3, 0.3, 1.0), (90, 70, 24), p)
    b = vm.distance((4.9, -2.8, 1.6), (61, 100, 20), p)
    ia, ib = a["info"], b["info"]
    span = []
    for o, n in (("x0", "nx"), ("y0", "ny"), ("z0", "nz")):
        lo, hi = max(ia[o], ib[o]) + R, min(ia[o] + ia[n], ib[o] + ib[n]) - R
        assert hi - lo >= 5, (o, lo, hi)
        span.append((lo, hi))
    cut = lambda i: tuple(slice(lo - i[o], hi - i[o]) for (lo, hi), o in zip(span[::-1], ("z0", "y0", "x0")))
    for k, _ in ref.CELL_ARRAYS:
        assert a[k][cut(ia)].tobytes() == b[k][cut(ib)].tobytes(), k
    assert (a["dist_sq"][cut(ia)] > 0).sum() > 100
