"""GPU tests of the scan-descriptor database (sicp_place_*), everything compared exactly against tests/place_ref.py: descriptor
bytes and info counts over channels, shapes, boundary points, NaN rows, origins and handle modes; every candidate's id, shift,
match and either over entry counts around the capacity doubling and the search's chunk edges, sector counts below, at and
above a wave, sub-ranges, top_k and min_score cuts, duplicated, periodic and empty entries; batches against lone calls;
storage across growth; the refusals, each leaving the database as it was; and the loop from a query to a registration."""
import importlib
import math

import numpy as np
import pytest

import place_cases as PC
import place_ref as PR

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
C = sicp.C
G, E, S = sicp.MODE_GICP, sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
BAD = sicp.ERR_INVALID_ARGUMENT


def _engine(mode=G, classes=11):
    p = sicp.default_params(mode)
    p.num_classes = classes
    return sicp.Engine(0, p)


def _both(R=20, S=60, max_range=40.0, min_range=0.0, channel=PR.LABEL, num_classes=7, z_min=-2.0, z_step=0.5, min_cell_points=1,
          ignore=()):
    """(the library's params, the restatement's, the restatement's tables) of one set of values"""
    if channel == PR.HEIGHT:
        num_classes, ignore = 0, ()
    lib = sicp.default_place_params(n_rings=R, n_sectors=S, max_range=max_range, min_range=min_range, channel=channel,
                                    num_classes=num_classes, z_min=z_min, z_step=z_step, min_cell_points=min_cell_points, ignore=ignore)
    ref = PR.params(R=R, S=S, max_range=max_range, min_range=min_range, channel=channel, num_classes=num_classes, z_min=z_min,
                    z_step=z_step, min_cell_points=min_cell_points, ignore=ignore)
    return lib, ref, PR.make_tables(R, S, max_range)


def _snapshot(db):
    return db.size(), db.get().tobytes()


def _counts(info):
    return {k: info[k] for k in ("n_in", "n_kept", "n_cells")}


# ---- describe ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel", [PR.LABEL, PR.HEIGHT], ids=["label", "height"])
@pytest.mark.parametrize("shape", [(1, 4), (20, 60), (7, 64), (64, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_describe_against_the_restatement(channel, shape):
    R, S_ = shape
    lp, rp, T = _both(R=R, S=S_, min_range=1.0, channel=channel, min_cell_points=2 if shape == (20, 60) else 1,
                      ignore=(3,) if shape != (1, 4) else ())
    xyz, lab = PC.cloud(17 + R, 3000, 40.0, 7)
    origin = (1.5, -2.25, 0.75)
    with sicp.PlaceDB(0, lp) as db, _engine() as e:
        got = db.tables()
        for k in ("edge2", "cos_half", "sin_half"):
            assert np.array_equal(got[k], T[k]), k
        e.set_source(xyz, lab)
        for o in (None, origin):
            desc, info = db.describe(e, SRC, o)
            want, winfo = PR.describe(xyz, lab, rp, T, o)
            assert desc.dtype == np.uint8 and desc.shape == (R, S_)
            assert np.array_equal(desc, want), np.argwhere(desc != want)[:5]
            assert _counts(info) == winfo
            assert winfo["n_in"] == len(xyz) - 4 and 0 < winfo["n_kept"] < winfo["n_in"] and winfo["n_cells"] > 0
        # no kept point: every cell is empty
        e.set_target(xyz + np.float32(1000.0), lab)
        desc, info = db.describe(e, TGT)
        assert not desc.any() and _counts(info) == {"n_in": len(xyz) - 4, "n_kept": 0, "n_cells": 0}
        # one point
        one = np.array([[3.0, 4.0, 0.4]], np.float32)
        e.set_target(one, np.array([2], np.uint32))
        desc, info = db.describe(e, TGT)
        want, winfo = PR.describe(one, [2], rp, T)
        assert np.array_equal(desc, want) and _counts(info) == winfo
        assert winfo["n_kept"] == 1 and winfo["n_cells"] == (0 if rp["min_cell_points"] == 2 else 1)
        assert db.size() == 0


def test_boundary_points_on_the_device():
    B = PC.BOUNDARY_PARAMS
    lp, rp, T = _both(R=B["R"], S=B["S"], max_range=B["max_range"], min_range=B["min_range"], channel=PR.HEIGHT, z_min=0.0, z_step=1.0)
    with sicp.PlaceDB(0, lp) as db, _engine() as e:
        for (p, kept, ring, sector) in PC.BOUNDARY_POINTS:
            e.set_source(np.array([p], np.float32))
            desc, info = db.describe(e)
            want = np.zeros((B["R"], B["S"]), np.uint8)
            if kept:
                want[ring, sector] = 1
            assert np.array_equal(desc, want) and info["n_kept"] == int(kept), p


def test_the_handle_mode_and_layout_play_no_part():
    lp, rp, T = _both(num_classes=11)
    xyz, lab = PC.cloud(5, 3000, 40.0, 11)
    want, winfo = PR.describe(xyz, lab, rp, T)
    with sicp.PlaceDB(0, lp) as db:
        for mode in (G, E, S):
            for which in (SRC, TGT):
                with _engine(mode) as e:
                    e.set_cloud(which, xyz, lab)
                    desc, info = db.describe(e, which)
                    assert np.array_equal(desc, want) and _counts(info) == winfo, (mode, which)
                    before = e.cloud_size(which)
                    assert db.add(e, which) == db.size() - 1 and e.cloud_size(which) == before
        assert np.array_equal(db.get(), np.stack([want] * 6))


# ---- search --------------------------------------------------------------------------------------------------------------
def _ranked(q, entries):
    return PR.query(q, entries, top_k=len(entries))


def _cut(ranked, first, count, top_k, min_score):
    rows = [r for r in ranked if first <= r["id"] < first + count][:top_k]
    out = []
    for r in rows:
        if not r["score"] >= min_score:
            break
        out.append(r)
    return out


SEARCH = [(1, 4, 1), (1, 4, 63), (1, 4, 64), (1, 4, 65), (1, 4, 300), (20, 60, 1), (20, 60, 63), (20, 60, 64), (20, 60, 65), (20, 60, 300),
          (20, 64, 65), (20, 256, 65), (1, 256, 300), (1, 60, 300), (64, 256, 9)]


@pytest.mark.parametrize("R,S_,n", SEARCH, ids=[f"{r}x{s}-{n}" for r, s, n in SEARCH])
def test_search_against_the_restatement(R, S_, n):
    lp, _, _ = _both(R=R, S=S_, num_classes=6)
    entries, queries = PC.search_database(40 + n + S_, n, R, S_)
    with sicp.PlaceDB(0, lp) as db:
        half = n // 2
        if half:
            assert db.add_descriptors(entries[:half]) == 0
            assert np.array_equal(db.get(), entries[:half])
        assert db.add_descriptors(entries[half:]) == half
        assert db.size() == n and np.array_equal(db.get(), entries)
        if n > 3:
            assert np.array_equal(db.get(2, n - 3), entries[2:n - 1])
        for qi, q in enumerate(queries):
            ranked = _ranked(q, entries)
            assert len(ranked) == n
            for top_k in (1, 5, n + 3):
                got = db.query(q, top_k=top_k)
                assert got == ranked[:top_k], (qi, top_k)
            # sub-ranges, an empty one among them
            for first, count in ((0, n), (n // 3, n - n // 3), (n // 3, max(n // 2 - n // 3, 0)), (n, 0), (0, 0), (n - 1, 1)):
                got = db.query(q, first=first, count=count, top_k=4)
                assert got == _cut(ranked, first, count, 4, 0.0), (qi, first, count)
            assert db.query(q, first=n // 3, count=-1, top_k=3) == _cut(ranked, n // 3, n, 3, 0.0)
            # a min_score that cuts the list behind its second row (or before its first)
            if n >= 3:
                floor_ = ranked[1]["score"]
                want = _cut(ranked, 0, n, n, floor_)
                assert db.query(q, top_k=n, min_score=floor_) == want and (len(want) < n or ranked[-1]["score"] == floor_)
            assert db.query(q, top_k=2, min_score=1.5) == []
        for row in db.query(queries[0], top_k=3):
            assert row["score"] == (row["match"] / row["either"] if row["either"] else 0.0)
            assert row["yaw"] == PR.yaw_of(row["shift"], S_) and -math.pi < row["yaw"] <= math.pi + 1e-12
        if n >= 8 and S_ >= 60:  # the rolled query meets entry 0 at its shift and its rolled copy one further
            top = db.query(queries[0], top_k=2)
            assert [(r["id"], r["shift"], r["match"] == r["either"]) for r in top] == [(0, S_ // 3, True), (7, (S_ // 3 + 1) % S_, True)]
            assert [r["id"] for r in db.query(queries[2], top_k=1)] == [3] and db.query(queries[2], top_k=1)[0]["shift"] == 0


def test_batches_equal_lone_calls_and_query_is_describe_then_search():
    lp, rp, T = _both(R=20, S=60, num_classes=7)
    entries, _ = PC.search_database(77, 150, 20, 60, codes=7)
    qs = PC.descriptors(78, 16, 20, 60, 7)
    qs[5] = entries[9]
    qs[11] = 0
    xyz, lab = PC.cloud(6, 3000, 40.0, 7)
    with sicp.PlaceDB(0, lp) as db, _engine() as e:
        db.add_descriptors(entries)
        batch = db.query(qs, top_k=6, first=10, count=120, min_score=0.05)
        assert len(batch) == 16
        for q in range(16):
            assert batch[q] == db.query(qs[q], top_k=6, first=10, count=120, min_score=0.05), q
            assert batch[q] == _cut(_ranked(qs[q], entries), 10, 120, 6, 0.05), q
        assert db.query(qs[:1], top_k=2) == [db.query(qs[0], top_k=2)]
        e.set_source(xyz, lab)
        desc, _ = db.describe(e)
        assert db.query(e, top_k=7) == db.query(desc, top_k=7) and len(db.query(e, top_k=7)) == 7
        origin = (0.5, 0.25, -1.0)
        assert db.query(e, SRC, origin, top_k=3) == db.query(db.describe(e, SRC, origin)[0], top_k=3)


def test_storage_clear_and_two_databases_alike():
    lp, rp, T = _both(R=7, S=64, num_classes=7)
    entries, queries = PC.search_database(91, 200, 7, 64, codes=7)
    clouds = [PC.cloud(200 + i, 1500, 40.0, 7) for i in range(3)]
    snaps = []
    for _ in range(2):
        with sicp.PlaceDB(0, lp) as db, _engine() as e:
            want = []
            for i, (xyz, lab) in enumerate(clouds):
                e.set_source(xyz, lab)
                assert db.add(e) == i
                want.append(PR.describe(xyz, lab, rp, T)[0])
            assert np.array_equal(db.get(), np.stack(want))
            assert db.add_descriptors(entries[:60]) == 3       # 63 entries: below the first capacity
            assert db.add_descriptors(entries[60:62]) == 63     # across it
            assert np.array_equal(db.get(), np.concatenate([np.stack(want), entries[:62]]))
            assert db.add_descriptors(entries[62:]) == 65       # and across the next doublings
            everything = np.concatenate([np.stack(want), entries])
            assert db.size() == 203 and np.array_equal(db.get(), everything)
            e.set_source(*clouds[1])
            assert db.add(e) == 203 and np.array_equal(db.get(203, 1)[0], want[1])
            first = db.query(queries[0], top_k=4)
            snaps.append((_snapshot(db), first))
            db.clear()
            assert db.size() == 0 and db.get().shape == (0, 7, 64) and db.query(queries[0]) == []
            assert db.add_descriptors(entries[:5]) == 0 and db.add(e) == 5
            assert db.query(entries[2], top_k=1)[0]["id"] == 2
    assert snaps[0] == snaps[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_create_refuses_bad_parameters():
    L = sicp.lib()
    ok = dict(num_classes=5)
    bad = [dict(n_rings=0), dict(n_rings=65), dict(n_sectors=0), dict(n_sectors=6), dict(n_sectors=260), dict(max_range=0.0),
           dict(max_range=float("inf")), dict(max_range=float("nan")), dict(min_range=-1.0), dict(min_range=40.0),
           dict(min_range=float("nan")), dict(channel=2), dict(num_classes=0), dict(num_classes=256), dict(ignore=(0,)),
           dict(ignore=(6,)), dict(n_ignore=65), dict(n_ignore=-1), dict(min_cell_points=0),
           dict(channel=sicp.PLACE_HEIGHT, z_step=0.0), dict(channel=sicp.PLACE_HEIGHT, z_step=float("nan")),
           dict(channel=sicp.PLACE_HEIGHT, z_step=5e-324),  # (its reciprocal is not finite)
           dict(channel=sicp.PLACE_HEIGHT, z_min=float("inf"))]
    for kw in bad:
        h = C.c_void_p()
        p = sicp.default_place_params(**{**ok, **kw})
        assert L.sicp_place_create(0, C.byref(p), C.byref(h)) == BAD and not h.value, kw
    h = C.c_void_p()
    p = sicp.default_place_params(**ok)
    assert L.sicp_place_create(0, None, C.byref(h)) == BAD
    assert L.sicp_place_create(0, C.byref(p), None) == BAD
    assert L.sicp_place_create(-1, C.byref(p), C.byref(h)) == BAD and L.sicp_place_create(99, C.byref(p), C.byref(h)) == BAD
    # the height channel ignores the label fields
    with sicp.PlaceDB(0, sicp.default_place_params(channel=sicp.PLACE_HEIGHT, num_classes=999)) as db:
        assert db.size() == 0
    assert L.sicp_place_destroy(None) == sicp.OK and L.sicp_place_size(None, None) == BAD and L.sicp_place_clear(None) == BAD
    assert L.sicp_place_last_error(None) == b""


def test_refusals_leave_the_database_as_it_was():
    L = sicp.lib()
    lp, rp, T = _both(R=4, S=8, num_classes=5)
    entries = PC.descriptors(3, 70, 4, 8, 5)
    xyz, lab = PC.cloud(8, 500, 40.0, 5)
    origin = np.zeros(3)
    with sicp.PlaceDB(0, lp) as db, _engine() as e, _engine() as bare, _engine() as empty, _engine() as wrong:
        db.add_descriptors(entries)
        e.set_source(xyz, lab)
        bare.set_source(xyz)                       # a cloud without labels
        far = lab.copy()
        far[np.isfinite(xyz).all(axis=1) & (np.hypot(xyz[:, 0], xyz[:, 1]) > 45.0)] = 99
        e.set_target(xyz, far)                     # labels above C on points the range drops: no error
        assert np.array_equal(db.describe(e, TGT)[0], db.describe(e, SRC)[0])
        near = lab.copy()
        near[int(np.argmax(np.isfinite(xyz).all(axis=1) & (np.hypot(xyz[:, 0], xyz[:, 1]) < 30.0)))] = 6
        wrong.set_source(xyz, near)                # one kept point with label C + 1
        before = _snapshot(db)
        desc = np.full((4, 8), 77, np.uint8)
        info = sicp.SicpPlaceDescribeInfo()
        info.n_in = -5
        new_id = C.c_int32(-7)
        out = (sicp.SicpPlaceCandidate * 4)()
        out[0].id = -9
        found = C.c_int32(-3)
        dp, bp, ip = sicp._dp, sicp._bp, sicp._ip
        d_ptr = desc.ctypes.data_as(bp)
        o_ptr = origin.ctypes.data_as(dp)
        nan_o = np.array([0.0, float("nan"), 0.0]).ctypes.data_as(dp)
        inf_o = np.array([float("inf"), 0.0, 0.0]).ctypes.data_as(dp)
        q_ptr = entries[0].ctypes.data_as(bp)
        high = entries[:2].copy()
        high[1, 2, 3] = 6
        calls = [
            ("describe NULL handle", lambda: L.sicp_place_describe(db._db, None, SRC, o_ptr, d_ptr, C.byref(info)), BAD),
            ("describe which", lambda: L.sicp_place_describe(db._db, e._h, 2, o_ptr, d_ptr, C.byref(info)), BAD),
            ("describe origin", lambda: L.sicp_place_describe(db._db, e._h, SRC, nan_o, d_ptr, C.byref(info)), BAD),
            ("describe no labels", lambda: L.sicp_place_describe(db._db, bare._h, SRC, o_ptr, d_ptr, C.byref(info)), BAD),
            ("describe no cloud", lambda: L.sicp_place_describe(db._db, empty._h, SRC, o_ptr, d_ptr, C.byref(info)), sicp.ERR_NOT_READY),
            ("describe bad label", lambda: L.sicp_place_describe(db._db, wrong._h, SRC, o_ptr, d_ptr, C.byref(info)), sicp.ERR_BAD_LABEL),
            ("add NULL handle", lambda: L.sicp_place_add(db._db, None, SRC, None, C.byref(new_id), d_ptr, C.byref(info)), BAD),
            ("add NULL id", lambda: L.sicp_place_add(db._db, e._h, SRC, None, None, d_ptr, C.byref(info)), BAD),
            ("add which", lambda: L.sicp_place_add(db._db, e._h, -1, None, C.byref(new_id), d_ptr, C.byref(info)), BAD),
            ("add origin", lambda: L.sicp_place_add(db._db, e._h, SRC, inf_o, C.byref(new_id), d_ptr, C.byref(info)), BAD),
            ("add no labels", lambda: L.sicp_place_add(db._db, bare._h, SRC, None, C.byref(new_id), d_ptr, C.byref(info)), BAD),
            ("add no cloud", lambda: L.sicp_place_add(db._db, empty._h, TGT, None, C.byref(new_id), d_ptr, C.byref(info)), sicp.ERR_NOT_READY),
            ("add bad label", lambda: L.sicp_place_add(db._db, wrong._h, SRC, None, C.byref(new_id), d_ptr, C.byref(info)), sicp.ERR_BAD_LABEL),
            ("add_descriptors n", lambda: L.sicp_place_add_descriptors(db._db, 0, q_ptr, C.byref(new_id)), BAD),
            ("add_descriptors NULL", lambda: L.sicp_place_add_descriptors(db._db, 1, None, C.byref(new_id)), BAD),
            ("add_descriptors byte", lambda: L.sicp_place_add_descriptors(db._db, 2, high.ctypes.data_as(bp), C.byref(new_id)), BAD),
            ("get first", lambda: L.sicp_place_get(db._db, -1, 1, d_ptr), BAD),
            ("get beyond", lambda: L.sicp_place_get(db._db, 69, 2, d_ptr), BAD),
            ("get count", lambda: L.sicp_place_get(db._db, 0, -2, d_ptr), BAD),
            ("get NULL", lambda: L.sicp_place_get(db._db, 0, 1, None), BAD),
            ("query NULL handle", lambda: L.sicp_place_query(db._db, None, SRC, None, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query which", lambda: L.sicp_place_query(db._db, e._h, 5, None, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query origin", lambda: L.sicp_place_query(db._db, e._h, SRC, nan_o, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query top_k", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 0, -1, 0, 0.0, out, C.byref(found)), BAD),
            ("query min_score", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 0, -1, 4, float("nan"), out, C.byref(found)), BAD),
            ("query first", lambda: L.sicp_place_query(db._db, e._h, SRC, None, -1, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query beyond", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 10, 61, 4, 0.0, out, C.byref(found)), BAD),
            ("query first beyond", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 71, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query NULL out", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 0, -1, 4, 0.0, None, C.byref(found)), BAD),
            ("query NULL n_found", lambda: L.sicp_place_query(db._db, e._h, SRC, None, 0, -1, 4, 0.0, out, None), BAD),
            ("query no labels", lambda: L.sicp_place_query(db._db, bare._h, SRC, None, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query no cloud", lambda: L.sicp_place_query(db._db, empty._h, SRC, None, 0, -1, 4, 0.0, out, C.byref(found)), sicp.ERR_NOT_READY),
            ("query bad label", lambda: L.sicp_place_query(db._db, wrong._h, SRC, None, 0, -1, 4, 0.0, out, C.byref(found)), sicp.ERR_BAD_LABEL),
            ("query_descriptors n_q", lambda: L.sicp_place_query_descriptors(db._db, 0, q_ptr, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query_descriptors NULL", lambda: L.sicp_place_query_descriptors(db._db, 1, None, 0, -1, 4, 0.0, out, C.byref(found)), BAD),
            ("query_descriptors byte", lambda: L.sicp_place_query_descriptors(db._db, 2, high.ctypes.data_as(bp), 0, -1, 2, 0.0, out, C.byref(found)), BAD),
            ("query_descriptors top_k", lambda: L.sicp_place_query_descriptors(db._db, 1, q_ptr, 0, -1, -1, 0.0, out, C.byref(found)), BAD),
            ("query_descriptors beyond", lambda: L.sicp_place_query_descriptors(db._db, 1, q_ptr, 70, 1, 4, 0.0, out, C.byref(found)), BAD),
        ]
        for name, call, status in calls:
            assert call() == status, name
            text = L.sicp_place_last_error(db._db).decode()
            assert text.startswith("sicp_place_"), (name, text)
            assert _snapshot(db) == before, name
            assert desc.min() == 77 and info.n_in == -5 and new_id.value == -7 and out[0].id == -9 and found.value == -3, name
            if name.endswith("byte"):
                assert "descriptor 1, ring 2, sector 3" in text and "(byte 51)" in text and "is 6" in text, text
            # the next valid call works
            assert db.query(entries[4], top_k=1)[0]["id"] == 4, name
        assert L.sicp_place_tables(None, None, None, None) == BAD and L.sicp_place_size(db._db, None) == BAD
        assert _snapshot(db) == before
        assert db.add(e) == 70 and db.size() == 71


def test_a_memory_limit_refuses_growth_and_keeps_the_entries():
    """Growth into the spare buffer under sicp_set_memory_limit.  With the limit at one byte the arena takes no new slab; filler
    databases then ask for exactly the block the growth will ask for (2051 entries of 64 x 256) until the arena's free blocks and
    slab space of that size are used up and one of them is refused.  From there the database's own growth must be refused: the
    status is SICP_ERR_OUT_OF_MEMORY, nothing has changed, and with the limit lifted the same call goes through."""
    lp, _, _ = _both(R=64, S=256, channel=PR.HEIGHT)
    few = PC.descriptors(5, 3, 64, 256, 200)
    many = np.zeros((2048, 64, 256), np.uint8)
    many[:, 0, 0] = np.arange(2048) % 251 + 1
    as_much = np.zeros((2051, 64, 256), np.uint8)  # an empty filler's first buffer: the size of the growth from 3 to 2051
    L = sicp.lib()
    fillers = []
    with sicp.PlaceDB(0, lp) as db:
        db.add_descriptors(few)
        before = _snapshot(db)
        first = C.c_int32(-1)
        try:
            fillers = [sicp.PlaceDB(0, lp) for _ in range(160)]
            sicp.set_memory_limit(0, 1)
            hit = False
            for f in fillers:
                st = L.sicp_place_add_descriptors(f._db, 2051, as_much.ctypes.data_as(sicp._bp), None)
                if st == sicp.ERR_OUT_OF_MEMORY:
                    hit = True
                    assert f.size() == 0
                    break
                assert st == sicp.OK
            assert hit, "160 fillers of 40 MB found room: the arena holds more free space than this test allows for"
            st = L.sicp_place_add_descriptors(db._db, 2048, many.ctypes.data_as(sicp._bp), C.byref(first))
            text = L.sicp_place_last_error(db._db).decode()
        finally:
            sicp.set_memory_limit(0, 0)
            for f in fillers:
                f.close()
        assert st == sicp.ERR_OUT_OF_MEMORY
        assert text.startswith("sicp_place_add_descriptors: ") and "out of memory" in text and text.endswith("the database is unchanged")
        assert _snapshot(db) == before and first.value == -1
        assert db.query(few[1], top_k=1)[0]["id"] == 1
        assert db.add_descriptors(many) == 3  # with the limit lifted it goes through
        assert db.size() == 2051
        assert np.array_equal(db.get(0, 3), few) and np.array_equal(db.get(2000, 10), many[1997:2007])
        top = db.query(many[1321], first=3, count=-1, top_k=1)[0]
        assert (top["match"], top["either"], top["shift"]) == (1, 1, 0) and many[top["id"] - 3, 0, 0] == many[1321, 0, 0]


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_db():
    sc = PC.scene()
    lp, rp, T = _both(num_classes=PC.SCENE_CLASSES, max_range=PC.SCENE_RANGE)
    db = sicp.PlaceDB(0, lp)
    with _engine() as e:
        for i, (xyz, lab) in enumerate(sc["entries"]):
            e.set_source(xyz, lab)
            assert db.add(e) == i
    yield db, sc
    db.close()


@pytest.mark.parametrize("k", range(4))
def test_a_query_starts_the_registration_that_closes_the_loop(scene_db, k):
    """The tolerance for "the same pose" is measured, not assumed: the two registrations' distance from each other is asserted
    at three times the larger of their distances from the ground truth (rotation and translation each); the margin allows for
    the outer loop's stopping slack."""
    db, sc = scene_db
    f = PC.loop_closure_figures(db, sc, k)
    print({k_: v for k_, v in f.items() if k_ != "candidates"}, f["candidates"][0])
    assert f["candidates"][0]["id"] == f["entry"]
    assert PC.cyclic_distance(f["candidates"][0]["shift"], PC.expected_shift(f["yaw_true_deg"], 60), 60) <= 1
    for axis in (0, 1):
        bound = 3.0 * max(f["place_vs_ground_truth"][axis], f["truth_start_vs_ground_truth"][axis])
        assert f["place_vs_truth_start"][axis] <= bound, (axis, f)
