"""CPU tests of the voxel map's label fusion (sicp_map_set_confusion, sicp_map_extract_fused, sicp_map_fused_labels): the
library exports the calls and refuses NULL maps without a device; the numpy restatement the GPU tests compare against
(tests/map_fusion_ref.py) equals a slow voxel-by-voxel restatement; the confusion matrix decides a case a majority vote cannot;
and the condition under which the GPU tests may compare labels exactly holds for every case they use."""
import ctypes
import importlib

import numpy as np
import pytest

import map_cases
import map_fusion_cases as cases
import map_fusion_ref as F

sicp = importlib.import_module("semantic-icp_amd")

ENTRY_POINTS = ("sicp_map_set_confusion", "sicp_map_extract_fused", "sicp_map_fused_labels")


def test_library_exports_the_fusion_entry_points():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    for name in ("set_confusion", "extract_fused", "fused_labels"):
        assert callable(getattr(sicp.VoxelMap, name))


def test_null_maps_and_bad_arguments_are_refused_without_a_device():
    lib = sicp.lib()
    INV = sicp.ERR_INVALID_ARGUMENT
    cm = np.eye(4)
    dp, up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)
    assert lib.sicp_map_set_confusion(None, 4, cm.ctypes.data_as(dp)) == INV
    assert lib.sicp_map_set_confusion(None, 4, None) == INV
    assert lib.sicp_map_set_confusion(None, 0, None) == INV
    p = sicp.default_map_extract_params()
    assert lib.sicp_map_extract_fused(None, None, None, 0, 0, None, None, None, None, None, None, None) == INV
    assert lib.sicp_map_extract_fused(None, ctypes.byref(p), None, 0, 0, None, None, None, None, None, None, None) == INV
    out = np.full(8, 0x5A5A5A5A, np.uint32)
    conf = np.full(8, -7.0)
    for args in ((None, 0, None, 1, 1), (None, 2, None, 1, 1), (None, 0, None, 2, 1), (None, 0, None, 1, 0)):
        assert lib.sicp_map_fused_labels(None, *args, out.ctypes.data_as(up), conf.ctypes.data_as(dp)) == INV
    assert lib.sicp_map_fused_labels(None, None, 0, None, 1, 1, None, None) == INV
    assert (out == 0x5A5A5A5A).all() and (conf == -7.0).all()


def test_log_matrix_is_libm_log_entry_by_entry():
    cm = cases.matrix(19)
    L = F.log_matrix(cm)
    assert np.array_equal(L, np.log(cm))  # (numpy's log and math.log agree on every entry here)
    assert np.allclose(cm.sum(axis=0), 1.0) and (np.argmax(cm, axis=0) == np.arange(19)).all()
    Z = F.log_matrix(cases.zero_matrix())
    assert np.isneginf(Z).sum() == 10 and Z[2, 2] == 0.0


@pytest.mark.parametrize("C", [4, 19])
def test_restatement_equals_the_slow_one(C):
    m, L = cases.built(True, C)
    out = cases.reference(True, C, 1)
    assert out["n_out"] > 1000 and len(out["labels"]) == out["n_out"]
    slow = [F.fuse_slow(row, L) for row in out["hist"]]
    assert out["labels"].tolist() == [s[0] for s in slow]
    assert np.allclose(out["confidence"], [s[1] for s in slow], rtol=1e-12, atol=0)
    assert (out["labels"] == 0).sum() == (out["confidence"] == 0).sum() > 0  # voxels that saw label 0 only
    assert ((out["confidence"] > 0) & (out["confidence"] <= 1.0) | (out["labels"] == 0)).all()
    # the relabelled probe, point by point
    xyz, lab, qt = cases.probe(C)
    for own in (True, False):
        got_l, got_c = F.fused_labels(m, L, xyz, lab, qt, include_own=own, min_count=1)
        ex = m.extract()
        cell = {tuple(v): i for i, v in enumerate(np.floor(ex["xyz"] / np.float32(m.leaf)).astype(np.int64).tolist())}
        import np_ref
        fin = np.isfinite(xyz).all(axis=1)
        p = np_ref.transform_points(np_ref.qt_to_mat(qt), xyz)
        for i in range(0, len(xyz), 7):
            if not fin[i]:
                assert (got_l[i], got_c[i]) == (0, 0.0)
                continue
            v = tuple(np.floor(p[i] * (np.float32(1.0) / np.float32(m.leaf))).astype(np.int64).tolist())
            row = ex["hist"][cell[v]] if v in cell else np.zeros(C + 1, np.uint32)
            want_l, want_c = F.fuse_slow(row, L, int(lab[i]) if own else 0)
            if want_c == 0.0:
                want_l = int(lab[i])
            assert got_l[i] == want_l and np.isclose(got_c[i], want_c, rtol=1e-12, atol=0), i
    assert (got_l[:12] == lab[:12]).all() and (got_c[:14] == 0).all()  # outside every voxel, no own term: the own label stays
    bad = lab.copy()
    bad[100] = C + 1
    with pytest.raises(F.BadLabel):
        F.fused_labels(m, L, xyz, bad, qt, include_own=True)
    assert F.fused_labels(m, L, xyz, bad, qt, include_own=False)[0][100] in (C + 1, *range(1, C + 1))


def test_five_road_observations_then_two_car_observations():
    """the histogram [0, 5, 2] under two classifiers.  One rarely confuses road and car: the voxel is road, almost surely.  The
    other all but never says "car" of a road voxel (and says "road" of a car half the time): two "car" observations outweigh
    five "road" ones.  A majority vote says road both times."""
    road = map_cases.lattice([[0, 0, 0]], per_cell=5, label=1, seed=1)
    car = map_cases.lattice([[0, 0, 0]], per_cell=2, label=2, seed=2)
    m = map_cases.build([road, car], num_classes=2)
    assert m.extract()["labels"].tolist() == [1] and m.hist.tolist() == [[0, 5, 2]]
    rarely = np.array([[0.9, 0.1], [0.1, 0.9]])
    never_car_for_road = np.array([[0.9999, 0.5], [0.0001, 0.5]])
    a = F.extract_fused(m, F.log_matrix(rarely))
    b = F.extract_fused(m, F.log_matrix(never_car_for_road))
    assert a["labels"].tolist() == [1] and a["confidence"][0] > 0.99
    assert b["labels"].tolist() == [2] and b["confidence"][0] > 0.99
    assert np.isclose(a["confidence"][0], 1.0 / (1.0 + (0.1 / 0.9) ** 3), rtol=1e-12)  # 0.9^5 0.1^2 against 0.1^5 0.9^2


def test_the_exactness_condition_of_the_gpu_tests():
    """The GPU tests compare labels exactly and leave no voxel out.  That is safe while no row's two best scores are closer than
    1e-9 relative (an ulp of difference in one log is 1e-16): asserted here for every case those tests use, exact ties -- the
    twin columns', the vote's equal counts -- excluded, for they are decided by the class index on both sides."""
    seen = 0
    for name, sc, evidence in cases.score_sets():
        g, tie = F.gaps(sc, evidence)
        n_tie = int(tie.sum())
        smallest = float(g[~tie].min()) if (~tie).any() else np.inf
        print(f"{name}: rows {len(sc)}, without evidence {int((~evidence).sum())}, exact ties {n_tie}, smallest gap {smallest:.3g}")
        if name not in ("twin", "vote"):
            assert n_tie == 0, name
        assert smallest >= 1e-9, name
        seen += 1
    assert seen == 2 * len(cases.CLASS_COUNTS) + 8 + 3
