"""GPU tests of the launches that change shape at wrap_cases.N0 points (tests/wrap_cases.py; what each case reaches is held by
tests/test_wrap_cases_cpu.py): the camera's and the range image's per-point kernels where a workgroup takes a second pass of
its stride loop, the planes' and the filter's tree sums where the tree gets a third level, each at N0, N0 + 1 and N0 + three
workgroups + 77; plane_orient's ny and nx branches; the pair pass and the radius count on a cell of more points than a
workgroup's first step takes.  Every output equals the module's restatement the way the module's own tests compare it:
integers equal, floats byte-equal."""
import importlib

import numpy as np
import pytest

import camera_ref
import range_ref
import test_gpu_camera as TC
import test_gpu_cluster as TK
import test_gpu_filter as TF
import test_gpu_plane as TP
import test_gpu_range as TR
import wrap_cases as W

pytestmark = pytest.mark.gpu
sicp = importlib.import_module("semantic-icp_amd")
E, S = sicp.MODE_EM, sicp.MODE_SEMANTIC
SRC, TGT = sicp.SOURCE, sicp.TARGET
MODES = {"em": E, "semantic": S}
_refs = {}


def _engine(mode=E):
    p = sicp.default_params(mode)
    p.num_classes = 11
    return sicp.Engine(0, p)


def _same_arrays(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in b)


# ---- camera ---------------------------------------------------------------------------------------------------------------------
def _camera_reference(size, window, p, mat):
    """the restatement fed the library's matrices: the shared one when they are the restatement's own to the bit"""
    c = W.camera_case(size)
    if _same_arrays(mat, camera_ref.matrices(c["qt"])):
        return W.camera_reference(size, window)
    key = ("camera", size, window)
    if key not in _refs:
        _refs[key] = camera_ref.labels(c["xyz"], c["labels"], c["pixel_label"], p, mat)
    return _refs[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", W.SIZES)
def test_camera_image_and_labels(size, mode):
    """64 x 48 pixels, a lens and a pose, NaN and Inf rows between the points; the image call with its per-point arrays, the label
    call at windows 1 and 5"""
    c = W.camera_case(size)
    mat = sicp.camera_matrices(c["qt"])
    with _engine(MODES[mode]) as e:
        e.set_source(c["xyz"], c["labels"])
        assert e.cloud_size(SRC) == (W.POINT_SIZES[size] + W.NAN_ROWS, W.POINT_SIZES[size])
        for window in W.CAMERA_WINDOWS:
            p = sicp.default_camera_params(**dict(c["p"], window=window))
            ref = _camera_reference(size, window, p, mat)
            TC._same_image(e.camera_image(SRC, p, c["qt"], per_point=True), ref["image"])
            TC._same_labels(e.camera_labels(SRC, c["pixel_label"], p, c["qt"]), ref)
    win = ref["image"]["index"][ref["image"]["index"] >= 0]
    assert (W.finite_position(c["xyz"])[win] >= W.N0).sum() == min(W.POINT_SIZES[size] - W.N0, W.TAIL_PIXELS)


# ---- range ----------------------------------------------------------------------------------------------------------------------
def _range_reference(size, p, tab):
    c = W.range_case(size)
    if _same_arrays(tab, range_ref.tables(range_ref.params(**c["p"]))):
        return W.range_reference(size)
    key = ("range", size)
    if key not in _refs:
        _refs[key] = range_ref.vote(c["xyz"], c["labels"], c["pixel_label"], p, tab, c["origin"])
    return _refs[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", W.SIZES)
def test_range_image_and_labels(size, mode):
    """64 x 8 pixels about an origin, NaN and Inf rows between the points; the image call with its per-point arrays, the vote at
    window 3 and k = 5"""
    c = W.range_case(size)
    p = sicp.default_range_params(**c["p"])
    ref = _range_reference(size, p, sicp.range_tables(p, c["beam"]))
    with _engine(MODES[mode]) as e:
        e.set_source(c["xyz"], c["labels"])
        assert e.cloud_size(SRC) == (W.POINT_SIZES[size] + W.NAN_ROWS, W.POINT_SIZES[size])
        TR._same_image(e.range_image(SRC, p, c["origin"], c["beam"]), ref["image"])
        TR._same_vote(e.range_labels(SRC, c["pixel_label"], p, c["origin"], c["beam"]), ref)
    win = ref["image"]["index"][ref["image"]["index"] >= 0]
    assert (W.finite_position(c["xyz"])[win] >= W.N0).sum() == min(W.POINT_SIZES[size] - W.N0, W.TAIL_PIXELS)


# ---- planes and filter ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", W.SIZES)
def test_plane_tree_sums(size, mode):
    """refine = 1 and two planes: the x y z e e tree and the products' tree, four times each, over caller indices that are mostly
    NaN rows and masked-out points"""
    c = W.plane_case(size)
    ref = W.plane_reference(size)
    with _engine(MODES[mode]) as e:
        e.set_source(c["xyz"], c["labels"])
        out = e.segment_planes(SRC, TP._params(c["params"]), c["mask"])
    TP._same(out, ref)
    assert out["info"]["n_planes"] == 2 and out["info"]["n_points"] == W.TREE_SIZES[size]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("size", W.SIZES)
def test_filter_tree_sums(size, mode):
    """mean_k = 6 with dropped, protected and masked points: mean, stddev and threshold are the tree's sums"""
    c = W.filter_case(size)
    ref = W.filter_reference(size)
    with _engine(MODES[mode]) as e:
        e.set_source(c["xyz"], c["labels"])
        out = e.filter(SRC, TF._params(c), c["mask"])
    TF._same(out, ref)
    assert out["info"]["n_points"] == W.TREE_SIZES[size] and 0 < out["info"]["n_fail_stat"] < out["info"]["n_tested"]


# ---- plane_orient ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(W.ORIENT))
def test_a_plane_through_the_origin_without_nz(name):
    """d = 0 and nz = 0: the sign is ny's -- also where nx has the other sign -- and with ny = 0 nx's"""
    c = W.orient_case(name)
    out = TP._run(c)
    print(out["coeff"])
    assert out["coeff"].shape == (1, 4) and W.orient_by_hand(name, out["coeff"][0])
    TP._same(out, W.orient_reference(name))


# ---- one cell of more points than a first step takes ------------------------------------------------------------------------------
def test_the_pair_pass_on_one_full_cell():
    """two labels under same_label = 1, the second on late points only: its pairs are joined by second steps or not at all"""
    c = W.one_cell_case()
    out = TK._run(c)
    TK._same(out, W.one_cell_cluster_reference())
    assert out["count"].tolist() == [W.ONE_CELL_FIRST_LABEL, W.ONE_CELL_N - W.ONE_CELL_FIRST_LABEL]


def test_the_radius_count_on_one_full_cell():
    c = W.one_cell_filter_case()
    out = TF._run(c)
    TF._same(out, W.one_cell_filter_reference())
    assert (out["neighbors"] == 2).all()
