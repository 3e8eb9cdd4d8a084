"""GPU tests of the elevation grid (sicp_map_elevation), everything compared for equal bytes against tests/elevation_ref.py: every
array and the info of every case of tests/elevation_cases.py on VoxelMap.from_state of its rows; the same on a map built by
integrate of synthetic scans, at one and at 4 x 4 columns a cell; a single-level cell's elevation is extract's z; the map's
state is the same before and after; two calls give the same bytes; every output alone; every refusal leaves the outputs and the
map as they were; the point outputs on every handle mode, slot and layout, with the handle left as it was; a cell's bytes do not
depend on the window; and one street scene with a kerb, a wall, a bridge and a parked car."""
import gc
import importlib
import math

import numpy as np
import pytest

import elevation_cases as cases
import elevation_ref as ref
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
    kw = {k: v for k, v in p.items() if k not in ("ignore", "blocked", "drivable", "width", "height")}
    return sicp.default_map_elevation_params(ignore=p["ignore"], blocked=p["blocked"], drivable=p["drivable"], **kw)


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
    return vm.elevation(c["center"], c["width"], c["height"], _params(c["params"]), engine, which, c["qt"])


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


@pytest.mark.parametrize("B", [1, 4])
def test_an_integrated_map_equals_the_restatement(street_map, B):
    vm, state, scans, poses = street_map
    assert len(state["key"]) > 5000
    kw = dict(width=120 // B + 1, height=96 // B, cell_voxels=B, clearance_voxels=6, ignore=(3, 4), blocked=(2,), max_step=0.3, min_neighbors=3,
              min_clearance=2.0)
    centre = (1.3, -0.4)
    xyz, lab = scans[2]
    qt = np_ref.mat_to_qt(poses[2])
    want = ref.elevation(state, ref.defaults(**kw), centre, xyz, qt)
    assert want["state"].sum() > want["state"].size // 5 and len(set(want["cell_class"].reshape(-1).tolist())) >= 4
    assert (want["point_cell"] >= 0).sum() > len(xyz) // 4 and np.isfinite(want["point_height"]).sum() > len(xyz) // 4
    with _engine(E) as e:
        e.set_source(xyz, lab)
        got = vm.elevation(centre, kw["width"], kw["height"], _params(ref.defaults(**kw)), e, SRC, qt)
    _same(got, want, B)
    assert _state_bytes(vm.get_state()) == _state_bytes(state)


def test_a_single_level_cell_has_extracts_z(street_map):
    vm, state, _, _ = street_map
    got = vm.elevation((0.0, 0.0), 200, 160, sicp.default_map_elevation_params(), want=("state", "elevation", "n_levels", "level_top", "count"))
    ex = vm.extract()
    key = state["key"].astype(np.int64)
    v = np.stack([(key & 0x1FFFFF) - ref.BIAS, ((key >> 21) & 0x1FFFFF) - ref.BIAS, (key >> 42) - ref.BIAS], axis=1)
    i, j = v[:, 0] - got["info"]["x0"], v[:, 1] - got["info"]["y0"]
    inside = (i >= 0) & (i < 200) & (j >= 0) & (j < 160)
    rows = np.flatnonzero(inside)
    top = rows[(got["level_top"][j[rows], i[rows]] == v[rows, 2]) & (got["state"][j[rows], i[rows]] == 1)]
    assert len(top) > 2000  # the top voxel of every surface cell: B = 1, so one row a level
    assert got["elevation"][j[top], i[top]].tobytes() == ex["xyz"][top, 2].tobytes()
    assert np.array_equal(got["count"][j[top], i[top]], ex["count"][top])
    assert (got["n_levels"][j[top], i[top]] == 1).sum() > 500


# ---- 3. the contracts -------------------------------------------------------------------------------------------------------------
def test_each_output_alone():
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    with sicp.VoxelMap.from_state(c["state"]) as vm, _engine() as e:
        e.set_source(c["points"], c["point_labels"])
        p = _params(c["params"])
        for k, _ in ALL:
            got = vm.elevation(c["center"], c["width"], c["height"], p, e, SRC, c["qt"], want=(k,))
            assert set(got) == {k, "info"} and got[k].tobytes() == want[k].tobytes(), k
            assert {q: got["info"][q] for q in ref.INFO} == want["info"], k
        info = sicp.SicpMapElevationInfo()  # no out struct at all: the counts are there
        ctr = np.array(c["center"])
        assert sicp.lib().sicp_map_elevation(vm._m, sicp._ptr(ctr, sicp._dp), C.byref(p_with_window(p, c)), None, None, 0, None, C.byref(info)) == sicp.OK
        assert list(info.n_class) == want["info"]["n_class"] and info.n_points == 0


def p_with_window(p, c):
    q = sicp.SicpMapElevationParams()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
    q.width, q.height = c["width"], c["height"]
    return q


SENTINEL = 0x5A


class _Raw:
    """the C call with outputs the test owns: arrays and an info block filled with 0x5A bytes"""

    def __init__(self, n_cells, n_points):
        self.bufs = {k: np.full(np.dtype(dt).itemsize * max(n_points if (k, dt) in ref.POINT_ARRAYS else n_cells, 1), SENTINEL, np.uint8)
                     for k, dt in ALL}
        self.out = sicp.SicpMapElevationOut()
        types = dict(sicp.SicpMapElevationOut._fields_)
        for k, a in self.bufs.items():
            setattr(self.out, k, a.ctypes.data_as(types[k]))
        self.info = sicp.SicpMapElevationInfo()
        C.memset(C.byref(self.info), SENTINEL, C.sizeof(self.info))

    def call(self, vm, center, p, h=None, which=SRC, qt=None, points=True):
        out = self.out
        if not points:
            out = sicp.SicpMapElevationOut()
            C.memmove(C.byref(out), C.byref(self.out), C.sizeof(out))
            out.point_cell, out.point_height = None, None
        ctr = None if center is None else np.ascontiguousarray(center, dtype=np.float64)
        q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
        return sicp.lib().sicp_map_elevation(None if vm is None else vm._m, sicp._ptr(ctr, sicp._dp), None if p is None else C.byref(p),
                                             C.byref(out), None if h is None else h._h, which, sicp._ptr(q, sicp._dp), C.byref(self.info))

    def untouched(self):
        return all((a == SENTINEL).all() for a in self.bufs.values()) and bytes(self.info) == bytes([SENTINEL]) * C.sizeof(self.info)


def test_every_refusal_writes_nothing_and_leaves_the_map_usable():
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    W, H = c["width"], c["height"]

    def params(**kw):
        lists = {k: kw.pop(k, ()) for k in ("ignore", "blocked", "drivable")}
        return sicp.default_map_elevation_params(**lists, **{**dict(width=W, height=H), **kw})

    with sicp.VoxelMap.from_state(c["state"]) as vm, _engine() as e, _engine() as e_empty, \
            sicp.VoxelMap.from_state(cases.patch_state(0)) as vm0:
        e.set_source(c["points"], c["point_labels"])
        before = _state_bytes(vm.get_state())
        raw = _Raw(W * H, len(c["points"]))
        ok = params()
        refused = [(what, INV, dict(p=params(**kw))) for what, kw in cases.REFUSED.items()]
        n65 = params()
        n65.n_blocked = 65
        neg = params()
        neg.n_ignore = -1
        refused += [
            ("n_blocked 65", INV, dict(p=n65)), ("n_ignore -1", INV, dict(p=neg)),
            ("NULL params", INV, dict(p=None)), ("NULL centre", INV, dict(center=None)),
            ("a centre that is NaN", INV, dict(center=(math.nan, 0.0))), ("a centre that is infinite", INV, dict(center=(0.0, math.inf))),
            ("a centre beyond the key's range", INV, dict(center=(0.5 * (1 << 20), 0.0))),
            ("a pose that is not finite", INV, dict(qt=[0, 0, 0, 1, 0, math.nan, 0])),
            ("a pose that is not finite, without a handle", INV, dict(qt=[0, 0, math.inf, 1, 0, 0, 0], h=None, points=False)),
            ("which = 2", INV, dict(which=2)), ("which = -1", INV, dict(which=-1)),
            ("point outputs without a handle", INV, dict(h=None)),
            ("a slot without a cloud", NR, dict(h=e_empty)), ("the handle's empty slot", NR, dict(which=TGT)),
            ("an ignore list on a map without classes", INV, dict(vm=vm0, p=params(ignore=(0,)))),
            ("a blocked list on a map without classes", INV, dict(vm=vm0, p=params(blocked=(0,)))),
            ("a drivable list on a map without classes", INV, dict(vm=vm0, p=params(drivable=(0,)))),
        ]
        for what, code, kw in refused:
            args = dict(vm=vm, center=c["center"], p=ok, h=e, which=SRC, qt=c["qt"])
            args.update(kw)
            assert raw.call(**args) == code, what
            assert raw.untouched(), what
            assert sicp.lib().sicp_map_last_error(args["vm"]._m).decode().startswith("sicp_map_elevation: "), what
        assert raw.call(None, c["center"], ok, e) == INV and raw.untouched()  # a NULL map
        assert _state_bytes(vm.get_state()) == before
        _same(_run_case(c, vm, e), want, "after the refusals")
        # a memory limit: the arena is trimmed to the slabs that hold live blocks and may take no new one, and a 2048 x 2048 call
        # needs nine 4-byte arrays of 4 Mi cells, 151 MB, before anything else.  While the arena holds less than that the refusal
        # is certain and is asserted; nothing is written and the map answers afterwards.  (An arena that other live objects of
        # the process keep larger may have the room: then the call may also be granted.)
        gc.collect()
        assert sicp.lib().sicp_release_pool(0) == sicp.OK
        reserved = sicp.memory_reserved(0)
        sicp.set_memory_limit(0, max(reserved, 1))
        try:
            big = params(width=2048, height=2048)
            raw2 = _Raw(2048 * 2048, 1)
            st = raw2.call(vm, c["center"], big, None, points=False)
        finally:
            sicp.set_memory_limit(0, 0)
        print("memory limit: reserved", reserved, "status", st)
        assert st == OOM if reserved < 9 * 4 * 2048 * 2048 else st in (sicp.OK, OOM)
        if st == OOM:
            assert raw2.untouched() and "sicp_map_elevation" in sicp.lib().sicp_map_last_error(vm._m).decode()
        assert _state_bytes(vm.get_state()) == before
        _same(_run_case(c, vm, e), want, "after the memory limit")


def test_the_points_on_every_mode_slot_and_layout_and_the_handle_untouched():
    """the point outputs are the restatement's on a GICP, an EM and a SEMANTIC handle (which groups its device layout by label),
    from either slot, before and after an align() has laid the clouds out; and a handle that made the calls aligns to the bytes
    of a twin that never did"""
    c = cases.case("points_posed")
    want = cases.reference("points_posed")
    with sicp.VoxelMap.from_state(c["state"]) as vm:
        for mode in (G, E, S):
            for which in (SRC, TGT):
                with _engine(mode) as e:
                    e.set_cloud(which, c["points"], c["point_labels"])
                    _same(_run_case(c, vm, e, which), want, (mode, which))
        src, sl, tgt, tl, T = synth.config1_pair()
        qt = np_ref.mat_to_qt(T)
        st = cases.patch_state()
        kw = dict(width=40, height=40, clearance_voxels=2)
        centre = (float(src[:, 0].mean()), float(src[:, 1].mean()))
        want_pair = {w: ref.elevation(st, ref.defaults(**kw), centre, pts, qt) for w, pts in ((SRC, src), (TGT, tgt))}
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
                            _same(vp.elevation(centre, 40, 40, p, e, SRC, qt), want_pair[SRC], (mode, "before align"))
                        first = e.align(qt)
                        idx, d2, w = e.correspondences(qt)
                        stats = e.stats()
                        if with_calls:
                            _same(vp.elevation(centre, 40, 40, p, e, SRC, qt), want_pair[SRC], (mode, "laid out"))
                            _same(vp.elevation(centre, 40, 40, p, e, TGT, qt), want_pair[TGT], (mode, "laid out, target"))
                            assert e.stats() == stats
                        second = e.align(qt)
                        drop = lambda s: {k: v for k, v in s.items() if not k.startswith("t_") and not k.endswith("_ms")}
                        res.append((first[0].tobytes(), second[0].tobytes(), idx.tobytes(), d2.tobytes(), w.tobytes(), drop(first[1]),
                                    drop(second[1])))
                assert res[0] == res[1], mode


def test_a_cells_bytes_do_not_depend_on_the_window(street_map):
    vm, state, _, _ = street_map
    p = sicp.default_map_elevation_params(cell_voxels=2, clearance_voxels=6, ignore=(3,))
    a = vm.elevation((0.3, 0.3), 90, 70, p)
    b = vm.elevation((7.9, -5.8), 61, 120, p)
    ia, ib = a["info"], b["info"]
    xs = range(max(ia["x0"], ib["x0"]), min(ia["x0"] + 90, ib["x0"] + 61))
    ys = range(max(ia["y0"], ib["y0"]), min(ia["y0"] + 70, ib["y0"] + 120))
    assert len(xs) > 30 and len(ys) > 30
    for k in ref.WINDOW_FREE:
        va = a[k][ys[0] - ia["y0"]:ys[-1] + 1 - ia["y0"], xs[0] - ia["x0"]:xs[-1] + 1 - ia["x0"]]
        vb = b[k][ys[0] - ib["y0"]:ys[-1] + 1 - ib["y0"], xs[0] - ib["x0"]:xs[-1] + 1 - ib["x0"]]
        assert va.tobytes() == vb.tobytes(), k
    assert a["state"].sum() > 1000


# ---- 4. a scene with meaning ---------------------------------------------------------------------------------------------------
ROAD, SIDEWALK, WALL, CAR, BRIDGE = 1, 2, 3, 4, 5


def _scene():
    """points on a grid of 0.1 m at leaf 0.25: a road (x in 0..10, y in 0..6, z = 0), a sidewalk 0.3 m higher beyond the kerb
    at y = 4, a wall at y in 5.5..6 from the sidewalk up to 3 m, a bridge deck at z = 5 over x in 6..8, and a parked car
    (a box 1.5 m high over x in 2..4, y in 1..2.5) of its own class"""
    g = np.arange(0.05, 10.0, 0.1)
    pts, lab = [], []

    def add(x, y, z, label):
        x, y, z = np.broadcast_arrays(x, y, z)
        pts.append(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1))
        lab.append(np.full(x.size, label))

    X, Y = np.meshgrid(g, g[g < 4.0], indexing="ij")
    add(X, Y, 0.02, ROAD)
    X, Y = np.meshgrid(g, g[(g > 4.0) & (g < 6.0)], indexing="ij")
    add(X, Y, 0.32, SIDEWALK)
    X, Z = np.meshgrid(g, np.arange(0.35, 3.0, 0.1), indexing="ij")
    for y in (5.55, 5.65, 5.8, 5.95):
        add(X, y, Z, WALL)
    X, Y = np.meshgrid(g[(g > 6.0) & (g < 8.0)], g[g < 6.0], indexing="ij")
    add(X, Y, 5.02, BRIDGE)
    X, Y, Z = np.meshgrid(g[(g > 2.0) & (g < 4.0)], g[(g > 1.0) & (g < 2.5)], np.arange(0.3, 1.5, 0.1), indexing="ij")
    add(X, Y, Z, CAR)
    return np.concatenate(pts).astype(np.float32), np.concatenate(lab).astype(np.uint32)


SCENE_LEAF = 0.25
SCENE_CENTRE = (5.1, 3.1)  # vc = (20, 12): x0 = 0, y0 = 0, a cell is a column of 0.25 m
SCENE = dict(width=40, height=24, clearance_voxels=6, ignore=(CAR,), max_extent_voxels=2, max_step=0.2)


def check_scene(run, xyz, lab):
    """what the scene means, asserted on run(keywords, with_points) -> an elevation result"""
    got = run(SCENE, False)
    assert (got["info"]["x0"], got["info"]["y0"]) == (0, 0)
    cell = lambda x, y: (int(y / SCENE_LEAF), int(x / SCENE_LEAF))
    road, under_car, under_bridge, kerb_low, kerb_high, sidewalk, wall = \
        cell(1.1, 1.1), cell(3.1, 1.6), cell(7.1, 1.1), cell(1.1, 3.9), cell(1.1, 4.1), cell(1.1, 4.9), cell(1.1, 5.8)
    z_road, z_walk, z_deck = np.float32(0.02), np.float32(0.32), np.float32(5.02)  # (a few equal float32 add up exactly in float64)
    # the car's cells carry the road's elevation and label: its voxels do not exist for this call
    assert got["elevation"][road] == z_road and got["elevation"][under_car] == z_road and got["label"][under_car] == ROAD
    assert got["cell_class"][under_car] == ref.FREE and got["cell_class"][road] == ref.FREE and np.isinf(got["ceiling"][road])
    assert got["n_levels"][under_car] == 1 and np.isinf(got["ceiling"][under_car])
    # the bridge is the ceiling over the road, not its elevation
    assert got["elevation"][under_bridge] == z_road and got["ceiling"][under_bridge] == z_deck
    assert got["label"][under_bridge] == ROAD and got["cell_class"][under_bridge] == ref.FREE
    # the kerb steps, on both sides; the sidewalk beyond it is free; the wall is an obstacle
    assert got["cell_class"][kerb_low] == ref.STEP and got["cell_class"][kerb_high] == ref.STEP
    assert got["step"][kerb_low] == got["step"][kerb_high] == z_walk - z_road
    assert got["cell_class"][sidewalk] == ref.FREE and got["label"][sidewalk] == SIDEWALK and got["elevation"][sidewalk] == z_walk
    assert got["cell_class"][wall] == ref.OBSTACLE and got["label"][wall] == WALL and got["level_bottom"][wall] == 1
    # a car that is seen is an obstacle; one whose class is blocked is that first
    seen = run(dict(SCENE, ignore=()), False)
    assert seen["cell_class"][under_car] == ref.OBSTACLE and seen["label"][under_car] == CAR and seen["level_bottom"][under_car] == 0
    assert run(dict(SCENE, ignore=(), blocked=(CAR,)), False)["cell_class"][under_car] == ref.BLOCKED_LABEL
    # with ref_z on the deck, the deck is the surface where there is one; elsewhere nothing changes
    deck = run(dict(SCENE, use_ref_z=1, ref_z=5.1), False)
    assert deck["elevation"][under_bridge] == z_deck and deck["label"][under_bridge] == BRIDGE and np.isinf(deck["ceiling"][under_bridge])
    assert deck["bottom"][under_bridge] == z_deck and deck["level_top"][under_bridge] == 20
    off = np.ones(got["state"].shape, bool)
    off[:, 24:32] = False  # the deck spans x in 6..8
    for k in ref.WINDOW_FREE:
        assert deck[k][off].tobytes() == got[k][off].tobytes(), k
    # the heights of the scan's own points above the MAPPED ground: the car's roof over the road under it
    pts = run(SCENE, True)
    roof = np.flatnonzero((lab == CAR) & (xyz[:, 2] > 1.35))
    assert len(roof) > 100 and (got["state"].reshape(-1)[pts["point_cell"][roof]] == 1).all()
    assert pts["point_height"][roof].tobytes() == (xyz[roof, 2] - z_road).astype(np.float32).tobytes()


def test_a_street_with_a_kerb_a_wall_a_bridge_and_a_parked_car():
    xyz, lab = _scene()
    with sicp.VoxelMap(0, sicp.default_map_params(leaf_size=SCENE_LEAF, num_classes=5)) as vm, _engine(G, 5) as e:
        e.set_source(xyz, lab)
        vm.integrate(e)
        state = vm.get_state()

        def run(kw, with_points):
            p = ref.defaults(**kw)
            got = vm.elevation(SCENE_CENTRE, kw["width"], kw["height"], _params(p), e if with_points else None)
            _same(got, ref.elevation(state, p, SCENE_CENTRE, xyz if with_points else None), kw)
            return got

        check_scene(run, xyz, lab)
