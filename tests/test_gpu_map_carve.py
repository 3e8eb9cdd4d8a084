"""GPU tests of free-space carving (sicp_map_carve), everything compared exactly against tests/map_carve_ref.py: the miss
counts of a dry run, every count of the info and every extract byte after a real carve, over the parameters, poses, origins,
NaN rows and handle modes; the walk at its edges (the hand cases, ray counts around a wave and a wave's share, rays of zero
and of more than 600 steps in one scan, candidates below / above / between the map's keys, a map of one voxel, a carve that
empties the map); the contracts (refusals change no byte, dry runs change nothing, the capacity refusal writes info only, the
handle is untouched, two maps driven alike are byte-identical, integrating after a carve continues the survivors' sums)."""
import importlib

import numpy as np
import pytest

import map_carve_cases as cases
import map_carve_ref as ref
import map_cases
import map_ref
import np_ref
import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
LEAF, CLASSES = cases.LEAF, cases.CLASSES
COUNTS = ("n_in", "n_rays", "n_steps", "n_voxels", "n_touched", "n_hit", "n_removed", "n_spared_hit", "n_spared_label")


def _engine(mode=G):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _vmap(leaf=LEAF, num_classes=CLASSES):
    return sicp.VoxelMap(0, sicp.default_map_params(leaf_size=leaf, num_classes=num_classes))


def _bytes(out):
    return tuple(None if out[k] is None else out[k].tobytes() for k in ("xyz", "labels", "count", "hist")) + \
        (out["info"]["n_out"], out["info"]["max_voxel_points"], out["info"]["n_voxels"])


def _snapshot(vm):
    return _bytes(vm.extract(want_hist=vm.num_classes > 0)), vm.size()


def _ref_bytes(m):
    ex = m.extract()
    hist = ex["hist"] if m.C > 0 else None
    return (ex["xyz"].tobytes(), None if ex["labels"] is None else ex["labels"].tobytes(), ex["count"].tobytes(),
            None if hist is None else hist.tobytes(), ex["n_out"], ex["max_voxel_points"], ex["n_voxels"]), m.size()


def _integrate(vm, m, scans, mode=G):
    """the scans into the library's map and into the restatement's"""
    e = _engine(mode)
    try:
        for xyz, lab in scans:
            e.set_source(xyz, lab)
            vm.integrate(e)
            m.integrate(xyz, lab if m.C > 0 else None)
    finally:
        e.close()


def _params(kw):
    """(the library's params, the restatement's) of one set of keywords"""
    return sicp.default_map_carve_params(**kw), ref.defaults(**kw)


def _carve_both(vm, m, e, xyz, qt=None, origin=None, which=SRC, **kw):
    """one carve through the library and through the restatement: miss, every count and -- after a real carve -- every extract
    byte agree"""
    lp, rp = _params(kw)
    got = vm.carve(e, which, qt, origin, lp, want_miss=True)
    want = ref.carve(m, xyz, qt, origin, rp)
    assert got["miss"].dtype == np.uint32 and np.array_equal(got["miss"], want["miss"])
    assert {k: got["info"][k] for k in COUNTS} == want["info"]
    assert _snapshot(vm) == _ref_bytes(m)
    return got


# ---- 1. restatement parity ------------------------------------------------------------------------------------------------------
PARITY = {
    "defaults": dict(),
    "min_rays1": dict(min_rays=1),
    "min_rays2": dict(min_rays=2),
    "margin0": dict(end_margin=0),
    "margin3": dict(end_margin=3),
    "range2.5": dict(max_range=2.5),
    "protect": dict(protect=(1, 3)),
    "protect_bin0_range": dict(protect=(0, 4), max_range=2.5, min_rays=2, end_margin=0),
}


@pytest.fixture(scope="module")
def four_maps():
    """the library's map of map_cases.four() is rebuilt per test from one handle per scan, uploaded once"""
    es = []
    for xyz, lab in map_cases.four():
        e = _engine()
        e.set_source(xyz, lab)
        es.append(e)
    yield es
    for e in es:
        e.close()


def _four(vm, es):
    for e in es:
        vm.integrate(e)
    return cases.four_map()


@pytest.mark.parametrize("name", sorted(PARITY))
def test_parity_over_the_parameters(four_maps, name):
    xyz, lab = cases.fifth()
    e = _engine()
    with _vmap() as vm:
        try:
            m = _four(vm, four_maps)
            assert vm.size()[0] == 1676
            e.set_source(xyz, lab)
            before = _snapshot(vm)
            dry = _carve_both(vm, m, e, xyz, None, cases.ORIGIN, dry_run=1, **PARITY[name])
            assert _snapshot(vm) == before and dry["info"]["n_voxels"] == 1676 and dry["info"]["n_removed"] > 0
            real = _carve_both(vm, m, e, xyz, None, cases.ORIGIN, **PARITY[name])
            assert np.array_equal(real["miss"], dry["miss"])
            assert {k: real["info"][k] for k in COUNTS if k != "n_voxels"} == {k: dry["info"][k] for k in COUNTS if k != "n_voxels"}
            assert real["info"]["n_voxels"] == 1676 - dry["info"]["n_removed"] == vm.size()[0]
        finally:
            e.close()


@pytest.mark.parametrize("mode", [G, E, S], ids=["gicp", "em", "semantic"])
def test_parity_posed_with_nan_rows_in_every_mode(four_maps, mode):
    """a posed scan with NaN rows and a sensor origin off the scan's own origin, from a handle of each mode (SEMANTIC groups
    the device layout by label): the result does not depend on the layout"""
    xyz, lab = cases.fifth(0.03)
    qt = cases.pose()
    e = _engine(mode)
    with _vmap() as vm:
        try:
            m = _four(vm, four_maps)
            e.set_cloud(TGT, xyz, lab)
            n_fin = e.cloud_size(TGT)[1]
            assert n_fin < 1500
            dry = _carve_both(vm, m, e, xyz, qt, cases.ORIGIN, which=TGT, dry_run=1, min_rays=2, protect=(2,))
            assert dry["info"]["n_in"] == n_fin and dry["info"]["n_removed"] > 0 and dry["info"]["n_spared_label"] > 0
            _carve_both(vm, m, e, xyz, qt, cases.ORIGIN, which=TGT, min_rays=2, protect=(2,))
            _carve_both(vm, m, e, xyz, qt, None, which=TGT, min_rays=1)  # the origin at the pose's own translation
        finally:
            e.close()


# ---- 2. walk edges --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def box():
    e = _engine()
    e.set_source(*cases.box_map())
    m = map_ref.Map(LEAF, CLASSES)
    m.integrate(*cases.box_map())
    for a in (m.key, m.s, m.cnt, m.hist):
        a.setflags(write=False)
    yield e, m
    e.close()


@pytest.mark.parametrize("name", sorted(cases.HAND))
def test_hand_cases_on_the_device(box, name):
    o, p, end_margin, want = cases.HAND[name]
    feeder, m = box
    e = _engine()
    with _vmap() as vm:
        try:
            vm.integrate(feeder)
            xyz = np.array([p], np.float32)
            e.set_source(xyz)
            got = _carve_both(vm, m, e, xyz, None, o, min_rays=1, end_margin=end_margin, dry_run=1)
            cand = want[:max(len(want) - 1 - end_margin, 0)]
            assert cases.visited_on_box(m, got["miss"]) == set(cand) and int(got["miss"].sum()) == len(cand)
            assert got["info"]["n_rays"] == 1 and got["info"]["n_steps"] == len(cand) and got["info"]["n_hit"] == 1
        finally:
            e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 257])
def test_ray_counts_around_a_wave(box, n):
    feeder, m = box
    xyz = cases.seeded_rays(n)
    e = _engine()
    with _vmap() as vm:
        try:
            vm.integrate(feeder)
            e.set_source(xyz)
            got = _carve_both(vm, m, e, xyz, None, cases.ORIGIN, min_rays=1, end_margin=0, dry_run=1)
            assert got["info"]["n_rays"] == n and got["info"]["n_steps"] == int(got["miss"].sum()) > 0  # (every candidate is in the box)
        finally:
            e.close()


def test_zero_length_and_600_step_rays_in_one_scan():
    """leaf 0.05: 30 returns in the sensor's own voxel among 40 rays of more than 600 steps, the map a sprinkling of points
    along those rays"""
    rng = np.random.default_rng(41)
    o = np.array([0.01, 0.02, 0.03])
    far = (np.array([12.5, 9.5, 10.5]) * rng.choice([-1.0, 1.0], (40, 3)) + rng.uniform(-0.5, 0.5, (40, 3)))
    here = o + rng.uniform(0.0, 0.015, (30, 3))
    xyz = np.concatenate([far, here])[rng.permutation(70)].astype(np.float32)
    along = (o + rng.uniform(0.02, 0.98, (400, 1)) * (far[rng.integers(0, 40, 400)] - o)).astype(np.float32)
    lab = np.ones(len(along), np.uint32)
    m = map_ref.Map(0.05, CLASSES)
    e = _engine()
    with _vmap(leaf=0.05) as vm:
        try:
            _integrate(vm, m, [(along, lab)])
            e.set_source(xyz)
            got = _carve_both(vm, m, e, xyz, None, o, min_rays=1, end_margin=0, dry_run=1)
            p, o32, vo, v, valid, casts = ref.rays_of(xyz, None, o, 0.05)
            steps = np.abs(v - vo).sum(axis=1)
            assert (steps == 0).sum() == 30 and (steps > 600).sum() == 40
            assert got["info"]["n_rays"] == 70 and got["info"]["n_steps"] == int(steps.sum()) and got["info"]["n_touched"] > 100
            _carve_both(vm, m, e, xyz, None, o, min_rays=1)
        finally:
            e.close()


def test_candidates_below_above_and_between_the_keys():
    """a map of every other voxel of the slab z = 0: rays from z = -3 up to z = +3 look up keys below the smallest, between
    neighbours and above the largest"""
    cells = [[x, y, 0] for x in range(-4, 5, 2) for y in range(-4, 5)]
    slab = map_cases.lattice(cells, seed=3)
    rng = np.random.default_rng(43)
    xyz = np.column_stack([rng.uniform(-2.4, 2.4, (300, 2)), rng.uniform(1.0, 1.6, 300)]).astype(np.float32)
    m = map_ref.Map(LEAF, CLASSES)
    e = _engine()
    with _vmap() as vm:
        try:
            _integrate(vm, m, [slab])
            e.set_source(xyz)
            got = _carve_both(vm, m, e, xyz, None, (0.1, 0.2, -1.4), min_rays=1, end_margin=0, dry_run=1)
            assert got["info"]["n_hit"] == 0 and 0 < got["info"]["n_touched"] < len(cells)
            assert int(got["miss"].sum()) < got["info"]["n_steps"]  # (most candidates are not in the map)
            _carve_both(vm, m, e, xyz, None, (0.1, 0.2, -1.4), min_rays=2)
        finally:
            e.close()


def test_a_map_of_one_voxel_and_a_carve_that_empties_it():
    one = map_cases.lattice([[2, 0, 0]], 3, seed=4)
    through = np.array([[2.2, 0.2, 0.3], [2.3, 0.25, 0.2], [2.1, 0.3, 0.25], [-1.0, 0.2, 0.2]], np.float32)  # three pass, one does not
    inside = np.array([[1.2, 0.2, 0.2]], np.float32)
    m = map_ref.Map(LEAF, CLASSES)
    e = _engine()
    with _vmap() as vm:
        try:
            _integrate(vm, m, [one])
            assert vm.size() == (1, 3)
            e.set_source(inside)
            got = _carve_both(vm, m, e, inside, None, (0.2, 0.2, 0.2), min_rays=1)  # a return in it: hit, never a candidate
            assert (got["info"]["n_hit"], got["info"]["n_touched"], got["info"]["n_removed"]) == (1, 0, 0) and vm.size() == (1, 3)
            e.set_source(through)
            got = _carve_both(vm, m, e, through, None, (0.2, 0.2, 0.2), min_rays=4)
            assert got["miss"].tolist() == [3] and got["info"]["n_removed"] == 0 and vm.size() == (1, 3)
            got = _carve_both(vm, m, e, through, None, (0.2, 0.2, 0.2))
            assert got["info"]["n_removed"] == 1 and got["info"]["n_voxels"] == 0 and vm.size() == (0, 0)
            ex = vm.extract(want_hist=True)
            assert ex["info"]["n_out"] == 0 and ex["xyz"].shape == (0, 3)
            # an empty map: nothing to do, nothing wrong
            got = _carve_both(vm, m, e, through, None, (0.2, 0.2, 0.2))
            assert got["miss"].shape == (0,) and got["info"]["n_rays"] == 4 and got["info"]["n_removed"] == 0
            _integrate(vm, m, [one])
            assert _snapshot(vm) == _ref_bytes(m)
        finally:
            e.close()


def test_a_scan_without_a_finite_point(four_maps):
    """an all-NaN scan casts no ray: SICP_OK, zero counts, a miss array of zeros, nothing changed -- and its origin is still
    checked"""
    xyz = np.full((130, 3), np.nan, np.float32)
    lab = np.ones(130, np.uint32)
    e = _engine()
    with _vmap() as vm:
        try:
            m = _four(vm, four_maps)
            e.set_source(xyz, lab)
            before = _snapshot(vm)
            got = _carve_both(vm, m, e, xyz, cases.pose(), cases.ORIGIN, min_rays=1)
            assert {k: got["info"][k] for k in COUNTS} == dict({k: 0 for k in COUNTS}, n_voxels=1676)
            assert got["miss"].shape == (1676,) and not got["miss"].any() and _snapshot(vm) == before
            with pytest.raises(ref.merge_ref.GridOverflow):
                ref.carve(m, xyz, None, (1e6, 0.0, 0.0))
            with pytest.raises(sicp.SicpError) as err:
                vm.carve(e, SRC, None, (1e6, 0.0, 0.0))
            assert err.value.status == sicp.ERR_INVALID_ARGUMENT and "leaf size" in str(err.value) and _snapshot(vm) == before
        finally:
            e.close()


def test_a_real_carve_without_a_miss_array(four_maps):
    xyz, lab = cases.fifth()
    e = _engine()
    with _vmap() as vm:
        try:
            m = _four(vm, four_maps)
            e.set_source(xyz, lab)
            got = vm.carve(e, SRC, None, cases.ORIGIN)
            want = ref.carve(m, xyz, None, cases.ORIGIN)
            assert got["miss"] is None and {k: got["info"][k] for k in COUNTS} == want["info"] and want["info"]["n_removed"] > 0
            assert _snapshot(vm) == _ref_bytes(m)
        finally:
            e.close()


# ---- 3. contracts ---------------------------------------------------------------------------------------------------------------
def _raw_carve(vm, e, which=SRC, qt=None, origin=None, params="default", capacity=0, miss=None):
    q = None if qt is None else np.ascontiguousarray(qt, dtype=np.float64)
    o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    p = sicp.default_map_carve_params() if isinstance(params, str) else params
    info = sicp.SicpMapCarveInfo()
    C.memset(C.byref(info), 0x5A, C.sizeof(info))
    st = sicp.lib().sicp_map_carve(vm._m, None if e is None else e._h, which, None if q is None else q.ctypes.data_as(dp),
                                   None if o is None else o.ctypes.data_as(dp), None if p is None else C.byref(p), capacity,
                                   None if miss is None else miss.ctypes.data_as(up), C.byref(info))
    return st, bytes(info) == b"\x5a" * C.sizeof(info), info


def test_refusals_leave_every_extract_byte_unchanged(four_maps):
    xyz, lab = cases.fifth()
    nan_pose = np.array([0, 0, 0, 1, 0, 0, 0.0])
    nan_pose[5] = np.nan
    INV, NR = sicp.ERR_INVALID_ARGUMENT, sicp.ERR_NOT_READY
    P = sicp.default_map_carve_params
    too_many = P()
    too_many.n_protect = sicp.MAP_MAX_PROTECT + 1
    good, empty = _engine(), _engine()
    with _vmap() as vm, _vmap(num_classes=0) as plain:
        try:
            _four(vm, four_maps)
            good.set_source(xyz, lab)
            plain.integrate(good)
            before, plain_before = _snapshot(vm), _snapshot(plain)
            refused = [
                ("a NULL handle", INV, dict(e=None)),
                ("NULL params", INV, dict(e=good, params=None)),
                ("which 2", INV, dict(e=good, which=2)),
                ("which -1", INV, dict(e=good, which=-1)),
                ("a NaN pose", INV, dict(e=good, qt=nan_pose)),
                ("a NaN origin", INV, dict(e=good, origin=(0, np.nan, 0))),
                ("an infinite origin", INV, dict(e=good, origin=(np.inf, 0, 0))),
                ("an origin at 1e6 with leaf 0.5", INV, dict(e=good, origin=(1e6, 0, 0))),
                ("a negative max_range", INV, dict(e=good, params=P(max_range=-1.0))),
                ("a NaN max_range", INV, dict(e=good, params=P(max_range=np.nan))),
                ("min_rays 0", INV, dict(e=good, params=P(min_rays=0))),
                ("end_margin -1", INV, dict(e=good, params=P(end_margin=-1))),
                ("dry_run 2", INV, dict(e=good, params=P(dry_run=2))),
                ("n_protect -1", INV, dict(e=good, params=P(n_protect=-1))),
                ("n_protect 65", INV, dict(e=good, params=too_many)),
                ("a protected label above num_classes", INV, dict(e=good, params=P(protect=(1, CLASSES + 1)))),
                ("a slot without a cloud", NR, dict(e=empty)),
                ("good's empty slot", NR, dict(e=good, which=TGT)),
            ]
            for what, code, kw in refused:
                st, info_untouched, _ = _raw_carve(vm, **kw)
                assert st == code, what
                assert info_untouched, what
                assert _snapshot(vm) == before, what
                assert sicp.lib().sicp_map_last_error(vm._m).decode().startswith("sicp_map_carve: "), what
                if what.startswith("an origin at 1e6"):
                    assert "leaf size" in sicp.lib().sicp_map_last_error(vm._m).decode()
            st, info_untouched, _ = _raw_carve(plain, good, params=P(protect=(1,)))
            assert st == INV and info_untouched and _snapshot(plain) == plain_before
            assert "sicp_map_carve: " in sicp.lib().sicp_map_last_error(plain._m).decode()
            # the capacity refusal writes info and nothing else
            m = cases.four_map()
            want = ref.carve(m, xyz, None, cases.ORIGIN, ref.defaults(dry_run=1))
            miss = np.full(1676, 0x5A5A5A5A, np.uint32)
            st, info_untouched, info = _raw_carve(vm, good, origin=cases.ORIGIN, capacity=1675, miss=miss)
            assert st == INV and not info_untouched and (miss == 0x5A5A5A5A).all() and _snapshot(vm) == before
            assert {k: getattr(info, k) for k in COUNTS} == want["info"]
            assert sicp.lib().sicp_map_last_error(vm._m).decode().startswith("sicp_map_carve: ")
            # ... and the map carves normally afterwards, +inf taking every ray
            st, _, info = _raw_carve(vm, good, origin=cases.ORIGIN, params=P(max_range=np.inf), capacity=1676, miss=miss)
            assert st == sicp.OK and np.array_equal(miss, want["miss"]) and info.n_voxels == 1676 - want["info"]["n_removed"]
            ref.carve(m, xyz, None, cases.ORIGIN)
            assert _snapshot(vm) == _ref_bytes(m)
        finally:
            good.close()
            empty.close()


def test_two_maps_driven_alike_and_integrating_after_a_carve(four_maps):
    """carve, then integrate the same scan (the loop's order), twice over: the two maps are byte-identical and equal the
    restatement, whose survivors' sums the integrate continues"""
    scans = [cases.fifth(), cases.fifth(0.03)]
    qts = [None, cases.pose()]
    snaps = []
    for _ in range(2):
        e = _engine(S)
        with _vmap() as vm:
            try:
                m = _four(vm, four_maps)
                for (xyz, lab), qt in zip(scans, qts):
                    e.set_source(xyz, lab)
                    got = _carve_both(vm, m, e, xyz, qt, cases.ORIGIN, min_rays=2)
                    assert got["info"]["n_removed"] > 0
                    info = vm.integrate(e, SRC, qt)
                    assert info["n_voxels"] == m.integrate(xyz, lab, qt)["n_voxels"]
                    assert _snapshot(vm) == _ref_bytes(m)
                snaps.append(_snapshot(vm))
            finally:
                e.close()
    assert snaps[0] == snaps[1]


def test_carve_leaves_the_handle_as_it_was():
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
            vm.integrate(e, TGT)
            n0 = vm.size()[0]
            out = vm.carve(e, SRC, qt, (0.0, 0.0, 0.5), sicp.default_map_carve_params(min_rays=1), want_miss=True)
            assert out["info"]["n_rays"] == len(src) and out["info"]["n_touched"] > 0 and len(out["miss"]) == n0
            assert e.stats() == stats
            assert e.accumulate(qt).tobytes() == acc.tobytes()  # (the correspondences on the device are the ones from before)
            idx2, d22, w2 = e.correspondences(qt)
            assert idx2.tobytes() == idx.tobytes() and d22.tobytes() == d2.tobytes() and w2.tobytes() == w.tobytes()
            qt2, st2 = e.align(qt)
            e2 = _engine(E)
            try:
                e2.set_confusion(synth.confusion_matrix(11))
                e2.set_source(src, sl)
                e2.set_target(tgt, tl)
                e2.align(qt)
                qt3, st3 = e2.align(qt)
            finally:
                e2.close()
            assert qt2.tobytes() == qt3.tobytes() and st2["final_cost"] == st3["final_cost"]  # the handle's align bits
        finally:
            e.close()
