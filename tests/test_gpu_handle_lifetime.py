"""GPU tests of what a handle keeps and what it forgets: sicp_destroy parks a handle with its streams, events, pinned mirrors,
device buffers and tick graphs, and sicp_create hands it out again as a NEW handle -- default parameters, no confusion
matrix, no clouds, no error text, its own streams -- whatever it was before (a batch leader, a stream's slot or uploader).
Every registration on a recycled handle gives the bits of the same registration on a handle made from nothing.  A second
sicp_destroy of a parked handle is refused, and a map, a stream and the pool give all device memory back."""
import ctypes
import gc
import importlib

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
IDENT = np.array([0, 0, 0, 1, 0, 0, 0.0])
MODES = (sicp.MODE_EM, sicp.MODE_GICP, sicp.MODE_SEMANTIC)
C = 4
SRC, SL, TGT, TL, _ = synth.config1_pair(seed=1, n_per_label=500)
CM = synth.confusion_matrix(C)
# the statistics that describe the registration, not how long it took
NOT_TIMING = [k for k, _ in sicp.SicpStats._fields_ if not (k.startswith("t_") or k.endswith("_ms"))]

_cache = {}


def _release_pool():
    gc.collect()
    assert sicp.lib().sicp_release_pool(0) == sicp.OK


def _params(mode):
    p = sicp.default_params(mode)
    p.num_classes = C
    return p


def _setup(e, mode):
    e.set_params(_params(mode))
    e.set_source(SRC, SL)
    e.set_target(TGT, TL)
    e.set_confusion(CM)


def _result(qt, st):
    """pose bits, outer iterations and every statistic that is not a time"""
    return (np.asarray(qt, dtype=np.float64).tobytes(), tuple((k, st[k]) for k in NOT_TIMING))


def _record(e):
    out = {}
    for mode in MODES:
        _setup(e, mode)
        out[mode] = _result(*e.align(IDENT))
    return out


def _fresh():
    """EM, GICP and SEMANTIC align() of the pair on one handle made from nothing (an empty pool), computed once"""
    if "fresh" not in _cache:
        _release_pool()
        with sicp.Engine(0) as e:
            _cache["fresh"] = _record(e)
        _release_pool()
    return _cache["fresh"]


def _last_error(e):
    return sicp.lib().sicp_last_error(e._h).decode()


def _align_status(e):
    out = np.empty(7)
    return sicp.lib().sicp_align(e._h, sicp._ptr(IDENT, sicp._dp), sicp._ptr(out, sicp._dp), None, None)


def test_recycled_handle_is_a_new_handle():
    fresh = _fresh()
    _release_pool()
    e = sicp.Engine(0)
    assert _record(e) == fresh
    # ---- dirty it: a batch it leads in another mode, a matrix of another size, the host-side solve, a refused call
    others = [sicp.Engine(0) for _ in range(2)]
    for g in [e] + others:
        _setup(g, sicp.MODE_SEMANTIC)
    sicp.align_batch([e] + others)
    e.set_confusion(synth.confusion_matrix(7))
    p = _params(sicp.MODE_GICP)
    p.lm_on_device = 0
    e.set_params(p)
    e.align(IDENT)
    p.knn = 3
    assert sicp.lib().sicp_set_params(e._h, ctypes.byref(p)) == sicp.ERR_INVALID_ARGUMENT
    assert _last_error(e) != ""
    for g in others:
        g.close()
    _release_pool()  # (the two others go; `e` is live and stays)
    # ---- destroy, create: the same context, nothing new reserved
    was = e._h.value
    e.close()
    reserved = sicp.memory_reserved(0)
    e = sicp.Engine(0)
    assert e._h.value == was  # the pool held exactly this handle
    assert sicp.memory_reserved(0) <= reserved
    # ---- and it is a new handle
    assert bytes(e.get_params()) == bytes(sicp.default_params(sicp.MODE_GICP))
    assert _last_error(e) == ""
    assert _align_status(e) == sicp.ERR_NOT_READY  # no clouds
    for n_classes in (7, C):  # (7: the size of the matrix it held last)
        p = sicp.default_params(sicp.MODE_EM)
        p.num_classes = n_classes
        e.set_params(p)
        e.set_source(SRC, SL)
        e.set_target(TGT, TL)
        assert _align_status(e) == sicp.ERR_NOT_READY  # no confusion matrix
    assert _record(e) == fresh
    e.close()


def test_stream_gives_back_handles_on_their_own_streams():
    fresh = _fresh()
    _release_pool()
    with sicp.Stream(0, _params(sicp.MODE_EM), max_in_flight=4, confusion=CM) as S:
        a, b = S.add_cloud(SRC, SL), S.add_cloud(TGT, TL)
        tickets = [S.submit(a, b, IDENT, fused_labels=k % 3 == 0, pose_covariance=k % 2 == 0) for k in range(6)]
        got = S.drain()
        assert sorted(t for t, *_ in got) == sorted(tickets) and all(status == sicp.OK for _, status, *_ in got)
        for _, _, qt, _ in got:
            assert qt.tobytes() == fresh[sicp.MODE_EM][0]
    engines = [sicp.Engine(0) for _ in range(5)]  # the four slots and the uploader
    assert len({g._h.value for g in engines}) == 5
    for g in engines:
        _setup(g, sicp.MODE_EM)
        assert _result(*g.align(IDENT)) == fresh[sicp.MODE_EM]
    for qt, st in sicp.align_batch(engines):
        assert qt.tobytes() == fresh[sicp.MODE_EM][0]
        assert st["outer_iters"] == dict(fresh[sicp.MODE_EM][1])["outer_iters"]
    with sicp.Stream(0, _params(sicp.MODE_EM), max_in_flight=4, confusion=CM):
        pass
    assert _result(*engines[0].align(IDENT)) == fresh[sicp.MODE_EM]
    for g in engines:
        g.close()
    _release_pool()
    assert sicp.memory_reserved(0) == 0


def test_second_destroy_of_a_parked_handle_is_refused():
    fresh = _fresh()
    lib = sicp.lib()
    h = ctypes.c_void_p()
    assert lib.sicp_create(0, ctypes.byref(h)) == sicp.OK
    assert lib.sicp_destroy(h) == sicp.OK
    assert lib.sicp_destroy(h) == sicp.ERR_INVALID_ARGUMENT
    a, b = sicp.Engine(0), sicp.Engine(0)
    assert a._h.value != b._h.value
    for g in (a, b):
        _setup(g, sicp.MODE_EM)
        assert _result(*g.align(IDENT)) == fresh[sicp.MODE_EM]
        g.close()


def test_map_gives_everything_back():
    _release_pool()
    with sicp.Engine(0, _params(sicp.MODE_EM)) as e:
        e.set_target(TGT, TL)
        with sicp.VoxelMap(0, sicp.default_map_params(leaf_size=0.2, num_classes=C)) as m:
            assert m.integrate(e, sicp.TARGET)["n_in"] == len(TGT)
            assert m.extract()["info"]["n_out"] > 0
    _release_pool()
    assert sicp.memory_reserved(0) == 0
