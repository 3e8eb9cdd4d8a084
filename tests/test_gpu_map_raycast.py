"""GPU tests of ray casting (sicp_map_raycast), everything compared exactly against tests/map_raycast_ref.py: every per-ray array
and every count of the info over the parameters, poses, origins, NaN ends and the modes of the handles that fed the map; the
walk at its edges (the hand cases at every start_margin, ray counts around a wave and a wave's share, rays of zero steps, of
one step and of more than 600 in one call, permuted ends and sub-ranges, voxels below / above / between the map's keys, a map
of one voxel, an empty map); dst (only what can be seen, the bits of set_target of the same arrays, the empty refusal); the
scene (through the car with ignore, the scan points the map contradicts); the contracts (refusals write nothing, the map's
bytes never change, two calls give the same bytes, a ray cast after a carve)."""
import importlib

import numpy as np
import pytest

import map_carve_cases
import map_carve_ref
import map_cases
import map_raycast_cases as cases
import map_raycast_ref as ref
import map_ref

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
LEAF, CLASSES = cases.LEAF, cases.CLASSES
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
DTYPES = dict(row=np.int32, step=np.int32, length=np.int32, xyz=np.float32, labels=np.uint32, count=np.uint32, range_sq=np.float64)


def _engine(mode=G):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _vmap(leaf=LEAF, num_classes=CLASSES):
    return sicp.VoxelMap(0, sicp.default_map_params(leaf_size=leaf, num_classes=num_classes))


def _snapshot(vm):
    out = vm.extract(want_hist=vm.num_classes > 0)
    return tuple(None if out[k] is None else out[k].tobytes() for k in ("xyz", "labels", "count", "hist")) + \
        (out["info"]["n_out"], out["info"]["max_voxel_points"], out["info"]["n_voxels"]), vm.size()


def _integrate(vm, m, scans, mode=G):
    """the scans into the library's map and (when given) into the restatement's"""
    e = _engine(mode)
    try:
        for xyz, lab in scans:
            e.set_source(xyz, lab)
            vm.integrate(e)
            if m is not None:
                m.integrate(xyz, lab if m.C > 0 else None)
    finally:
        e.close()


def _same(got, want, what=""):
    for k in ref.ARRAYS:
        assert got[k].dtype == DTYPES[k] and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.flatnonzero((got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))[:5])
    assert {k: got["info"][k] for k in ref.COUNTS} == want["info"], what


def _cast_both(vm, m, ends, qt=None, origin=None, want=None, **kw):
    """one ray cast through the library and through the restatement: every array and every count agree, and the hit's point,
    label and count are extract's at `row`"""
    got = vm.raycast(ends, qt, origin, sicp.default_map_raycast_params(**kw))
    if want is None:
        want = ref.raycast(m, ends, qt, origin, ref.defaults(**kw))
    _same(got, want, kw)
    ex = vm.extract()
    h = got["row"] >= 0
    assert got["xyz"][h].tobytes() == ex["xyz"][got["row"][h]].tobytes() and np.array_equal(got["count"][h], ex["count"][got["row"][h]])
    if vm.num_classes > 0:
        assert np.array_equal(got["labels"][h], ex["labels"][got["row"][h]])
    else:
        assert not got["labels"].any()
    return got


# ---- 1. restatement parity ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sparse_feeders():
    """one handle per sparse scan, uploaded once"""
    es = []
    for xyz, lab in cases.sparse_scans():
        e = _engine()
        e.set_source(xyz, lab)
        es.append(e)
    yield es
    for e in es:
        e.close()


@pytest.mark.parametrize("name", sorted(cases.PARITY))
def test_parity_over_the_parameters(sparse_feeders, name):
    n_scans, kw = cases.PARITY[name]
    want = cases.parity_reference(name)
    with _vmap() as vm:
        for e in sparse_feeders[:n_scans]:
            vm.integrate(e)
        assert vm.size()[0] == want["info"]["n_voxels"]
        before = _snapshot(vm)
        got = _cast_both(vm, None, cases.sparse_ends(), None, cases.ORIGIN, want=want, **kw)
        assert got["info"]["n_hits"] == int((got["row"] >= 0).sum()) and got["info"]["n_visible"] == len(np.unique(got["row"][got["row"] >= 0]))
        assert _snapshot(vm) == before


@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
def test_parity_posed_with_nan_ends_in_every_mode(mode):
    """a posed sensor, ends with NaN rows, the sensor origin off the frame's origin, the map fed from a handle of each mode
    (SEMANTIC groups the device layout by label): the result does not depend on the layout"""
    ends = cases.sparse_ends(0.03)
    qt = map_carve_cases.pose()
    m = map_ref.Map(LEAF, CLASSES)
    with _vmap() as vm:
        _integrate(vm, m, cases.sparse_scans()[:1], mode)
        got = _cast_both(vm, m, ends, qt, cases.ORIGIN, ignore=(2,))
        bad = ~np.isfinite(ends).all(axis=1)
        assert bad.sum() == 45 and (got["length"][bad] == -1).all() and (got["length"][~bad] >= 0).all()
        assert got["info"]["n_in"] == 1500 and got["info"]["n_rays"] == 1455 and 20 <= got["info"]["n_hits"] <= 1435
        _cast_both(vm, m, ends, qt, None, max_range=5.0)  # the origin at the pose's own translation
        _cast_both(vm, m, ends, None, None, start_margin=0, min_count=2)


# ---- 2. walk edges --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    e = _engine()
    e.set_source(*map_carve_cases.box_map())
    m = map_ref.Map(LEAF, CLASSES)
    m.integrate(*map_carve_cases.box_map())
    for a in (m.key, m.s, m.cnt, m.hist):
        a.setflags(write=False)
    vm = _vmap()
    vm.integrate(e)
    yield vm, m
    vm.close()
    e.close()


def _coords(key):
    B = map_ref.BIAS
    return int(key & 0x1fffff) - B, int((key >> 21) & 0x1fffff) - B, int((key >> 42) & 0x1fffff) - B


@pytest.mark.parametrize("name", sorted(map_carve_cases.HAND))
def test_hand_cases_on_the_device(box, name):
    """every voxel of the box map is occupied: with start_margin = k the hit is the walk's k-th voxel, written out by hand"""
    vm, m = box
    o, p, _, want = map_carve_cases.HAND[name]
    end = np.asarray(p, np.float32)[None]
    n = len(want) - 1
    for k in range(n + 2):
        got = _cast_both(vm, m, end, None, o, start_margin=k)
        assert got["length"][0] == n and got["info"]["n_rays"] == 1
        if k <= n:
            assert got["step"][0] == k and _coords(m.key[got["row"][0]]) == want[k], (name, k)
            assert (got["info"]["n_steps"], got["info"]["n_hits"], got["info"]["n_visible"]) == (1, 1, 1)
        else:
            assert (got["row"][0], got["step"][0], got["range_sq"][0]) == (-1, -1, -1.0) and got["info"]["n_steps"] == 0


def test_many_rays_on_the_box_map(box):
    """every ray hits at step start_margin, whatever its length"""
    vm, m = box
    ends = map_carve_cases.seeded_rays(500)
    for k in (0, 1, 2):
        got = _cast_both(vm, m, ends, None, map_carve_cases.ORIGIN, start_margin=k)
        long_enough = got["length"] >= k
        assert (got["step"][long_enough] == k).all() and (got["row"][~long_enough] == -1).all() and long_enough.sum() > 400


@pytest.fixture(scope="module")
def sparse(sparse_feeders):
    vm = _vmap()
    vm.integrate(sparse_feeders[0])
    m = cases.sparse_map()
    for a in (m.key, m.s, m.cnt, m.hist):
        a.setflags(write=False)
    yield vm, m
    vm.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 257, 1000])
def test_ray_counts_around_a_wave_and_a_waves_share(sparse, n):
    vm, m = sparse
    ends = map_carve_cases.seeded_rays(n, half=5.9)
    got = _cast_both(vm, m, ends, None, cases.ORIGIN)
    assert got["info"]["n_rays"] == n and got["info"]["n_steps"] > 0
    if n >= 63:
        assert 0 < got["info"]["n_hits"] < n


def test_zero_one_and_600_step_rays_in_one_call():
    """leaf 0.05: ends in the sensor's own voxel (0 steps), ends two voxels along x whose ray hits the voxel beside the sensor at
    step 1, and one ray of more than 600 steps that hits nothing -- the lanes that finish at once are dealt the next rays
    while one lane walks on"""
    rng = np.random.default_rng(47)
    o = np.array([0.01, 0.02, 0.03])
    here = o + rng.uniform(0.0, 0.015, (30, 3))
    beside = np.array([0.11, 0.02, 0.03]) + rng.uniform(0.0, 0.015, (30, 3))
    far = np.array([[-12.5, -9.5, -10.5]])
    ends = np.concatenate([here, beside, far])[rng.permutation(61)].astype(np.float32)
    pts = np.concatenate([[[0.07, 0.02, 0.03], [0.07, 0.03, 0.04]], rng.uniform(0.3, 2.0, (200, 3))]).astype(np.float32)
    lab = np.ones(len(pts), np.uint32)
    m = map_ref.Map(0.05, CLASSES)
    with _vmap(leaf=0.05) as vm:
        _integrate(vm, m, [(pts, lab)])
        got = _cast_both(vm, m, ends, None, o)
        assert (got["length"] == 0).sum() == 30 and ((got["step"] == 1) & (got["length"] == 2)).sum() == 30
        long_one = got["length"] > 600
        assert long_one.sum() == 1 and got["row"][long_one][0] == -1
        assert got["info"]["n_hits"] == 30 and got["info"]["n_visible"] == 1
        assert got["info"]["n_steps"] == 30 + int(got["length"][long_one][0])
        _cast_both(vm, m, ends, None, o, start_margin=0)  # (the sensor's own voxel is not in the map: the same hits)


def test_permuted_ends_and_sub_ranges_give_the_same_bytes_per_ray(sparse):
    vm, _ = sparse
    ends = cases.sparse_ends(0.03)
    full = vm.raycast(ends, None, cases.ORIGIN)
    perm = np.random.default_rng(5).permutation(len(ends))
    shuffled = vm.raycast(ends[perm], None, cases.ORIGIN)
    for k in ref.ARRAYS:
        assert shuffled[k].tobytes() == full[k][perm].tobytes(), k
    assert {k: shuffled["info"][k] for k in ref.COUNTS} == {k: full["info"][k] for k in ref.COUNTS}
    for a, b in ((100, 300), (0, 1), (129, 1500), (700, 764)):
        part = vm.raycast(ends[a:b], None, cases.ORIGIN)
        for k in ref.ARRAYS:
            assert part[k].tobytes() == full[k][a:b].tobytes(), (k, a, b)
        assert part["info"]["n_hits"] == int((full["row"][a:b] >= 0).sum())


def test_voxels_below_above_and_between_the_keys():
    """a map of every other voxel column of the slab z = 0: rays from z = -3 up to z = +3 look up keys below the smallest,
    between neighbours and above the largest; with the slab transparent they look up all the way"""
    cells = [[x, y, 0] for x in range(-4, 5, 2) for y in range(-4, 5)]
    slab = map_cases.lattice(cells, seed=3)
    rng = np.random.default_rng(43)
    ends = np.column_stack([rng.uniform(-2.4, 2.4, (300, 2)), rng.uniform(1.0, 1.6, 300)]).astype(np.float32)
    m = map_ref.Map(LEAF, CLASSES)
    with _vmap() as vm:
        _integrate(vm, m, [slab])
        o = (0.1, 0.2, -1.4)
        got = _cast_both(vm, m, ends, None, o)
        assert 50 < got["info"]["n_hits"] < 250 and (got["step"][got["row"] >= 0] < got["length"][got["row"] >= 0]).all()
        through = _cast_both(vm, m, ends, None, o, ignore=(1,))  # every voxel of the slab is label 1
        assert through["info"]["n_hits"] == 0 and through["info"]["n_steps"] == int(through["length"].sum())
        _cast_both(vm, m, -ends, None, (0.1, 0.2, 1.4))  # downwards: the z steps search below


def test_a_map_of_one_voxel_and_an_empty_map():
    one = map_cases.lattice([[2, 0, 0]], 3, seed=4)
    # voxel (2, 0, 0) is x in [1, 1.5): an end in it, an end behind it, an end before it, an end away from it, no end at all
    ends = np.array([[1.2, 0.2, 0.3], [3.3, 0.25, 0.2], [0.7, 0.3, 0.25], [-1.0, 0.2, 0.2], [np.nan, 0.0, 0.0]], np.float32)
    o = (0.2, 0.2, 0.2)
    m = map_ref.Map(LEAF, CLASSES)
    with _vmap() as vm:
        # an empty map: all -1, and n_steps is still counted
        got = _cast_both(vm, m, ends, None, o)
        assert (got["row"] == -1).all() and got["length"].tolist() == [2, 6, 1, 2, -1] and got["info"]["n_steps"] == 2 + 6 + 1 + 2
        assert got["info"]["n_voxels"] == 0 and got["info"]["n_rays"] == 4
        assert _cast_both(vm, m, ends, None, o, start_margin=3)["info"]["n_steps"] == 0 + 4 + 0 + 0
        _integrate(vm, m, [one])
        assert vm.size() == (1, 3)
        got = _cast_both(vm, m, ends, None, o)
        assert got["row"].tolist() == [0, 0, -1, -1, -1] and got["step"].tolist() == [2, 2, -1, -1, -1] and got["count"][:2].tolist() == [3, 3]
        assert got["info"]["n_visible"] == 1
        assert _cast_both(vm, m, ends, None, o, min_count=4)["info"]["n_hits"] == 0
        none = vm.raycast(np.zeros((0, 3), np.float32), None, o)
        assert none["row"].shape == (0,) and none["xyz"].shape == (0, 3) and none["info"]["n_in"] == 0 and none["info"]["n_voxels"] == 1


# ---- 3. dst ---------------------------------------------------------------------------------------------------------------------
def _align_bits(e, init=IDENT):
    qt, st = e.align(init)
    keys = ("outer_iters", "total_lm_iters", "total_evals", "total_corr", "total_active", "final_cost")
    return qt.tobytes(), tuple(st[k] for k in keys)


def test_only_the_inner_layer_of_a_shell_is_visible():
    """a shell two voxels thick around the sensor: every ray hits, every row hit lies in the inner layer, and of its 98 voxels
    the 54 that are seen are the 3 x 3 in the middle of each face -- a voxel on an edge or a corner of the layer can only be
    entered through a face voxel, which stops the ray"""
    xyz, lab, cells = cases.shell_map()
    ends = sicp.lidar_ray_ends(48, 96, -89.0, 89.0, 4.0, origin=(0.25, 0.25, 0.25))
    m = map_ref.Map(LEAF, CLASSES)
    e = _engine()
    with _vmap() as vm:
        try:
            _integrate(vm, m, [(xyz, lab)])
            assert vm.size()[0] == 7 ** 3 - 3 ** 3
            got = vm.raycast(ends, None, (0.25, 0.25, 0.25), dst=e, dst_which=SRC)
            _same(got, ref.raycast(m, ends, None, (0.25, 0.25, 0.25)))
            u = np.unique(got["row"][got["row"] >= 0])
            ring = np.array([max(abs(c) for c in _coords(k)) for k in m.key[u]])
            assert got["info"]["n_hits"] == len(ends) and (ring == 2).all() and got["info"]["n_visible"] == len(u) == 6 * 9
            assert all(sorted(abs(c) for c in _coords(k))[1] <= 1 for k in m.key[u])
            assert e.cloud_size(SRC) == (len(u), len(u))
        finally:
            e.close()


@pytest.mark.parametrize("mode,which", [(G, TGT), (S, TGT), (G, SRC)], ids=["gicp_target", "semantic_target", "gicp_source"])
def test_dst_is_what_set_cloud_of_the_visible_rows_makes_it(mode, which):
    scans = map_carve_cases.scene()["scans"]
    other = SRC if which == TGT else TGT
    a, b = _engine(mode), _engine(mode)
    with _vmap(num_classes=3) as vm:
        try:
            _integrate(vm, None, scans[:2])
            a.set_cloud(other, *scans[2])
            a.set_cloud(which, scans[0][0][:300], scans[0][1][:300])
            before = _snapshot(vm)
            got = vm.raycast(cases.scene_rays(), None, map_carve_cases.SENSOR, dst=a, dst_which=which)
            _same(got, cases.scene_reference())
            u = np.unique(got["row"][got["row"] >= 0])
            assert got["info"]["n_visible"] == len(u) == 316 and a.cloud_size(which) == (316, 316) and _snapshot(vm) == before
            ex = vm.extract()
            b.set_cloud(other, *scans[2])
            b.set_cloud(which, ex["xyz"][u], ex["labels"][u])
            assert _align_bits(a) == _align_bits(b)
        finally:
            a.close()
            b.close()


def _raw(vm, ends, qt=None, origin=None, params="default", dst=None, dst_which=TGT, n=None, null_end=False, fill=0x5A):
    """sicp_map_raycast with sentinel-filled outputs: (status, outputs untouched, info untouched, info)"""
    ends = np.ascontiguousarray(ends, np.float32).reshape(-1, 3)
    cols = [np.ascontiguousarray(ends[:, a]) if len(ends) else np.zeros(1, np.float32) for a in range(3)]
    n = len(ends) if n is None else n
    q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
    o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    dp, fp, ip, up = (C.POINTER(t) for t in (C.c_double, C.c_float, C.c_int32, C.c_uint32))
    p = sicp.default_map_raycast_params() if isinstance(params, str) else params
    outs = [np.full(max(len(ends), 1), fill, np.uint8).repeat(8).view(t) for t in
            (np.int32, np.int32, np.int32, np.float32, np.float32, np.float32, np.uint32, np.uint32, np.float64)]
    outs = [a[:max(len(ends), 1)].copy() for a in outs]
    ptrs = [a.ctypes.data_as(t) for a, t in zip(outs, (ip, ip, ip, fp, fp, fp, up, up, dp))]
    info = sicp.SicpMapRaycastInfo()
    C.memset(C.byref(info), fill, C.sizeof(info))
    st = sicp.lib().sicp_map_raycast(vm._m, None if q is None else q.ctypes.data_as(dp), None if o is None else o.ctypes.data_as(dp), n,
                                     cols[0].ctypes.data_as(fp), None if null_end else cols[1].ctypes.data_as(fp), cols[2].ctypes.data_as(fp),
                                     None if p is None else C.byref(p), None if dst is None else dst._h, dst_which, *ptrs, C.byref(info))
    untouched = all(a.tobytes() == bytes([fill]) * a.nbytes for a in outs)
    return st, untouched, bytes(info) == bytes([fill]) * C.sizeof(info), info


def test_no_visible_row_refuses_dst_and_writes_info_only(sparse):
    vm, m = sparse
    ends = cases.sparse_ends()[:200]
    want = ref.raycast(m, ends, None, cases.ORIGIN, ref.defaults(min_count=50))["info"]
    assert want["n_hits"] == 0 and want["n_rays"] == 200 and want["n_steps"] > 0
    a, b = _engine(), _engine()
    try:
        for e in (a, b):
            e.set_source(*cases.sparse_scans()[0])
            e.set_target(*cases.sparse_scans()[1])
        before = _snapshot(vm)
        st, untouched, info_untouched, info = _raw(vm, ends, None, cases.ORIGIN, sicp.default_map_raycast_params(min_count=50), dst=a)
        assert st == sicp.ERR_TOO_FEW_POINTS and untouched and not info_untouched
        assert {k: getattr(info, k) for k in ref.COUNTS} == want
        assert "sicp_map_raycast: " in sicp.lib().sicp_map_last_error(vm._m).decode()
        with pytest.raises(sicp.SicpError) as err:
            vm.raycast(ends, None, cases.ORIGIN, sicp.default_map_raycast_params(min_count=50), dst=a)
        assert err.value.status == sicp.ERR_TOO_FEW_POINTS
        assert a.cloud_size(TGT) == b.cloud_size(TGT) == (800, 800) and _snapshot(vm) == before
        assert _align_bits(a) == _align_bits(b)
        # without dst the same call is fine
        st, untouched, info_untouched, info = _raw(vm, ends, None, cases.ORIGIN, sicp.default_map_raycast_params(min_count=50))
        assert st == sicp.OK and not untouched and info.n_hits == 0 and info.n_visible == 0
    finally:
        a.close()
        b.close()


# ---- 4. the scene ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_vm():
    vm = _vmap(num_classes=3)
    _integrate(vm, None, map_carve_cases.scene()["scans"][:2])
    yield vm
    vm.close()


def test_the_scene_sees_the_car_or_through_it(scene_vm):
    CAR = map_carve_cases.CAR
    seen = scene_vm.raycast(cases.scene_rays(), None, map_carve_cases.SENSOR)
    _same(seen, cases.scene_reference())
    on_car = (seen["row"] >= 0) & (seen["labels"] == CAR)
    assert seen["info"]["n_hits"] == 1840 and on_car.sum() == 150
    through = scene_vm.raycast(cases.scene_rays(), None, map_carve_cases.SENSOR, sicp.default_map_raycast_params(ignore=(CAR,)))
    _same(through, cases.scene_reference((CAR,)))
    assert through["info"]["n_hits"] == 1840 and not (through["labels"][through["row"] >= 0] == CAR).any()
    assert (through["range_sq"][on_car] > seen["range_sq"][on_car]).all()


def test_scan_points_that_the_map_contradicts(scene_vm):
    """scan 3's own points as ends against the map of scans 1 - 2: the points whose ray meets a CAR voxel before its end"""
    CAR = map_carve_cases.CAR
    scan3 = map_carve_cases.scene()["scans"][2][0]
    got = scene_vm.raycast(scan3, None, map_carve_cases.SENSOR)
    want = ref.raycast(map_carve_cases.scene_map(), scan3, None, map_carve_cases.SENSOR)
    _same(got, want)
    blocked = np.flatnonzero((got["row"] >= 0) & (got["labels"] == CAR) & (got["step"] < got["length"]))
    assert len(blocked) > 0
    assert np.array_equal(blocked, np.flatnonzero((want["row"] >= 0) & (want["labels"] == CAR) & (want["step"] < want["length"])))


# ---- 5. contracts ---------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(sparse):
    vm, _ = sparse
    ends = cases.sparse_ends()[:100]
    nan_pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
    nan_pose[5] = np.nan
    P = sicp.default_map_raycast_params
    too_many = P()
    too_many.n_ignore = sicp.MAP_RAYCAST_MAX_IGNORE + 1
    a, b = _engine(), _engine()
    with _vmap(num_classes=0) as plain:
        try:
            for e in (a, b):
                e.set_source(*cases.sparse_scans()[0])
                e.set_target(*cases.sparse_scans()[1])
            plain.integrate(a)
            before, plain_before = _snapshot(vm), _snapshot(plain)
            refused = [
                ("NULL params", dict(params=None)),
                ("a NULL end array", dict(null_end=True)),
                ("n -1", dict(n=-1)),
                ("a NaN pose", dict(qt=nan_pose)),
                ("a NaN origin", dict(origin=(0, np.nan, 0))),
                ("an infinite origin", dict(origin=(np.inf, 0, 0))),
                ("an origin at 1e6 with leaf 0.5", dict(origin=(1e6, 0, 0))),
                ("a negative max_range", dict(params=P(max_range=-1.0))),
                ("a NaN max_range", dict(params=P(max_range=np.nan))),
                ("min_count 0", dict(params=P(min_count=0))),
                ("start_margin -1", dict(params=P(start_margin=-1))),
                ("n_ignore -1", dict(params=P(n_ignore=-1))),
                ("n_ignore 65", dict(params=too_many)),
                ("an ignored label above num_classes", dict(params=P(ignore=(1, CLASSES + 1)))),
                ("dst_which 2", dict(dst=a, dst_which=2)),
                ("dst_which -1", dict(dst=a, dst_which=-1)),
            ]
            for what, kw in refused:
                kw = dict(dict(origin=cases.ORIGIN), **kw)
                st, untouched, info_untouched, _ = _raw(vm, ends, **kw)
                assert st == sicp.ERR_INVALID_ARGUMENT, what
                assert untouched and info_untouched, what
                assert _snapshot(vm) == before, what
                assert sicp.lib().sicp_map_last_error(vm._m).decode().startswith("sicp_map_raycast: "), what
                if what.startswith("an origin at 1e6"):
                    assert "leaf size" in sicp.lib().sicp_map_last_error(vm._m).decode()
            st, untouched, info_untouched, _ = _raw(plain, ends, params=P(ignore=(1,)))
            assert st == sicp.ERR_INVALID_ARGUMENT and untouched and info_untouched and _snapshot(plain) == plain_before
            assert sicp.lib().sicp_map_raycast(None, *([None] * 2), 0, *([None] * 5), 0, *([None] * 10)) == sicp.ERR_INVALID_ARGUMENT
            # dst is as it was: its size, and the bits of its next align
            assert a.cloud_size(TGT) == b.cloud_size(TGT) == (800, 800) and a.cloud_size(SRC) == b.cloud_size(SRC)
            assert _align_bits(a) == _align_bits(b)
            # ... and the map casts normally afterwards, +inf taking every ray
            st, untouched, info_untouched, info = _raw(vm, ends, origin=cases.ORIGIN, params=P(max_range=np.inf))
            assert st == sicp.OK and not untouched and not info_untouched and info.n_rays == 100 and _snapshot(vm) == before
        finally:
            a.close()
            b.close()


def test_every_output_is_nullable_and_two_calls_give_the_same_bytes(sparse):
    vm, m = sparse
    ends = cases.sparse_ends()
    before = _snapshot(vm)
    one = vm.raycast(ends, None, cases.ORIGIN)
    two = vm.raycast(ends, None, cases.ORIGIN)
    for k in ref.ARRAYS:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert _snapshot(vm) == before
    # no arrays at all: the counts alone; then one array alone
    fp = C.POINTER(C.c_float)
    cols = [np.ascontiguousarray(ends[:, a]) for a in range(3)]
    info = sicp.SicpMapRaycastInfo()
    p = sicp.default_map_raycast_params()
    o = np.ascontiguousarray(cases.ORIGIN, np.float64)
    args = (vm._m, None, o.ctypes.data_as(C.POINTER(C.c_double)), len(ends), *(c.ctypes.data_as(fp) for c in cols), C.byref(p), None, TGT)
    assert sicp.lib().sicp_map_raycast(*args, *([None] * 9), C.byref(info)) == sicp.OK
    assert {k: getattr(info, k) for k in ref.COUNTS} == {k: one["info"][k] for k in ref.COUNTS}
    step = np.full(len(ends), -7, np.int32)
    assert sicp.lib().sicp_map_raycast(*args, None, step.ctypes.data_as(C.POINTER(C.c_int32)), *([None] * 7), None) == sicp.OK
    assert np.array_equal(step, one["step"])


def test_a_ray_cast_after_a_carve(sparse_feeders):
    """the shared lookup on a map the carve has changed: carve the second sparse scan's rays out of the first scan's map, then
    cast; both follow the restatement"""
    xyz, lab = cases.sparse_scans()[1]
    m = cases.sparse_map()
    with _vmap() as vm:
        vm.integrate(sparse_feeders[0])
        got = vm.carve(sparse_feeders[1], SRC, None, cases.ORIGIN, sicp.default_map_carve_params(min_rays=1), want_miss=True)
        want = map_carve_ref.carve(m, xyz, None, cases.ORIGIN, map_carve_ref.defaults(min_rays=1))
        assert np.array_equal(got["miss"], want["miss"]) and got["info"]["n_removed"] == want["info"]["n_removed"] > 50
        assert vm.size()[0] == len(m.key) < 780
        _cast_both(vm, m, cases.sparse_ends(), None, cases.ORIGIN)
        _cast_both(vm, m, cases.sparse_ends(), map_carve_cases.pose(), None, ignore=(1, 3), start_margin=0)
