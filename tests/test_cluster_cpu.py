"""CPU tests of sicp_cluster: the header declares it and the library exports it, the ctypes structures have the header's layout,
and the numpy / scipy restatement the GPU tests compare against (tests/cluster_ref.py) agrees with an O(n^2) statement of the
same rules on a small form of every case family -- whose inputs have the properties they are meant to have."""
import ctypes
import importlib
import os
import subprocess
import textwrap

import numpy as np
import pytest

import cluster_cases
import cluster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")
TABLE = ("cluster_id", "label", "count", "first_index", "centroid", "bbox_min", "bbox_max")
COUNTS = ("n_points", "n_kept", "n_components", "n_clusters", "max_cluster_points", "n_clustered")


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_cluster_entry_points():
    text = open(os.path.join(ROOT, "include", "sicp.h")).read()
    for name in ("int sicp_cluster(", "int sicp_default_cluster_params(", "typedef struct sicp_cluster_params", "typedef struct sicp_cluster_info",
                 "#define SICP_CLUSTER_MAX_IGNORE 64"):
        assert name in text, name
    lib = ctypes.CDLL(sicp.build())
    assert hasattr(lib, "sicp_cluster") and hasattr(lib, "sicp_default_cluster_params")


def test_struct_layouts_match_the_header(tmp_path):
    pf = [n for n, _ in sicp.SicpClusterParams._fields_]
    inf = [n for n, _ in sicp.SicpClusterInfo._fields_]
    offs = [f"offsetof(sicp_cluster_params, {n})" for n in pf] + [f"offsetof(sicp_cluster_info, {n})" for n in inf]
    code = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "sicp.h"
        int main(void) {
          size_t v[] = {sizeof(sicp_cluster_params), sizeof(sicp_cluster_info), SICP_CLUSTER_MAX_IGNORE, %s};
          for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) printf("%%zu ", v[i]);
          return 0;
        }
        """
    ) % ", ".join(offs)
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert ctypes.sizeof(sicp.SicpClusterParams) == v[0] and ctypes.sizeof(sicp.SicpClusterInfo) == v[1]
    assert sicp.CLUSTER_MAX_IGNORE == v[2] == 64
    want = [getattr(sicp.SicpClusterParams, n).offset for n in pf] + [getattr(sicp.SicpClusterInfo, n).offset for n in inf]
    assert want == v[3:]
    assert set(inf) == set(COUNTS) | {"t_total_ms"}


def test_default_cluster_params():
    p = sicp.default_cluster_params()
    assert (p.tolerance, p.min_points, p.max_points, p.same_label, p.n_ignore) == (0.5, 10, 0, 1, 0)
    q = sicp.default_cluster_params(ignore=(1, 2), tolerance=0.3, min_points=4, max_points=900, same_label=0)
    assert (q.tolerance, q.min_points, q.max_points, q.same_label, q.n_ignore, list(q.ignore[:2])) == (0.3, 4, 900, 0, 2, [1, 2])
    with pytest.raises(AttributeError):
        sicp.default_cluster_params(leaf_size=0.3)
    with pytest.raises(ValueError):
        sicp.default_cluster_params(ignore=range(65))
    assert sicp.lib().sicp_default_cluster_params(None) == sicp.ERR_INVALID_ARGUMENT


# ---- the restatement against the slow statement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cluster_cases.NAMES)
def test_restatement_equals_the_slow_statement(name):
    c = cluster_cases.case(name, True)
    assert len(c["xyz"]) <= 600
    a, b = cluster_cases.reference(name, True), cluster_ref.cluster_slow(c["xyz"], c["labels"], **c["params"])
    for k in COUNTS:
        assert a[k] == b[k], k
    for k in TABLE:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_refusals_of_the_restatement():
    with pytest.raises(cluster_ref.GridOverflow):
        cluster_ref.cluster(cluster_cases.beyond_the_grid(), None, cluster_cases.T, 1, 0, 0)
    assert cluster_ref.cluster(cluster_cases.beyond_the_grid()[:1], None, cluster_cases.T, 1, 0, 0)["n_clusters"] == 1
    with pytest.raises(ValueError):
        cluster_ref.cluster(np.zeros((3, 3), np.float32), None)


# ---- the cases have the properties they are meant to have -----------------------------------------------------------------------
def test_the_grid_is_safe_for_every_joined_pair():
    """every pair rule 2 joins lies in cells at most one apart per axis -- on the faces case at every magnitude, and on random
    pairs at the threshold about random large coordinates"""
    rng = np.random.default_rng(3)
    for tol in (0.5, 0.3, 0.07, 1.3):
        assert float(cluster_ref.grid_inv(tol)) * float(np.float32(tol)) <= 1.0
        p = (rng.uniform(-1, 1, (20000, 3)) * 10.0 ** rng.uniform(-2, 5, (20000, 1))).astype(np.float32)
        d = rng.normal(size=(20000, 3))
        d *= (tol * (1 - 10.0 ** rng.uniform(-8, -1, 20000)) / np.linalg.norm(d, axis=1))[:, None]
        q = (p.astype(np.float64) + d).astype(np.float32)
        joined = cluster_ref.d2_f32(p, q) < cluster_ref.t2_of(tol)
        assert joined.sum() > 1000
        assert np.abs(cluster_ref.cell_coords(p, tol) - cluster_ref.cell_coords(q, tol))[joined].max() == 1


def test_street_case_holds_objects_speckle_and_ignored_classes():
    c, r = cluster_cases.case("street_05_same"), cluster_cases.reference("street_05_same")
    assert len(c["xyz"]) == 20000 and r["n_kept"] == int((~np.isin(c["labels"], (1, 2))).sum()) < 20000
    assert r["n_components"] > 500 and 10 < r["n_clusters"] < r["n_components"]  # most components are speckle
    assert r["max_cluster_points"] > 1000 and (r["count"] >= 10).all()
    assert (r["cluster_id"][np.isin(c["labels"], (1, 2))] == -1).all()
    assert (np.diff(r["first_index"]) > 0).all()
    loose = cluster_cases.reference("street_05_any")
    assert loose["n_components"] < r["n_components"]  # joining across labels merges components
    assert cluster_cases.reference("street_03_same")["n_components"] > r["n_components"]


def test_lattice_case_sits_on_the_threshold():
    c = cluster_cases.case("lattice_tie")
    assert len(c["xyz"]) == 729
    assert cluster_ref.d2_f32(c["xyz"][0], c["xyz"][1]) == cluster_ref.t2_of(0.5) == np.float32(0.25)
    tie, join = cluster_cases.reference("lattice_tie"), cluster_cases.reference("lattice_join")
    assert tie["n_clusters"] == 729 and (tie["count"] == 1).all() and np.array_equal(tie["cluster_id"], np.arange(729))
    assert join["n_clusters"] == 1 and join["count"].tolist() == [729]


@pytest.mark.parametrize("shape", cluster_cases.LONG)
def test_long_cases_are_one_component_in_either_order(shape):
    a, b = cluster_cases.reference(shape), cluster_cases.reference(shape + "_shuffled")
    n = len(cluster_cases.case(shape)["xyz"])
    assert a["n_clusters"] == b["n_clusters"] == 1 and a["count"].tolist() == b["count"].tolist() == [n]
    assert n >= 2002
    cells = cluster_ref.cell_coords(cluster_cases.case(shape)["xyz"], cluster_cases.T)
    assert len(np.unique(cells, axis=0)) > 500  # hooks across many cells


def test_comb_arms_meet_only_at_the_far_end():
    c = cluster_cases.case("comb")
    cut = cluster_ref.cluster(c["xyz"][:-2], c["labels"][:-2], **c["params"])  # without the bridge: two arms
    assert cut["n_clusters"] == 2 and cut["count"].tolist() == [1000, 1000]


def test_dense_case_is_one_cell_heavy():
    c = cluster_cases.case("dense")
    cells, n = np.unique(cluster_ref.cell_coords(c["xyz"], cluster_cases.T), axis=0, return_counts=True)
    assert n.max() > 2500
    r = cluster_cases.reference("dense")
    assert r["count"].tolist() == [5000, 1] and r["first_index"].tolist() == [0, 5000]
    m = cluster_cases.reference("dense_max")
    assert m["count"].tolist() == [1] and m["first_index"].tolist() == [5000] and (m["cluster_id"][:5000] == -1).all()
    assert m["n_components"] == 2 and m["n_clustered"] == 1


def test_faces_case_straddles_faces_edges_and_corners_both_ways():
    c, r = cluster_cases.case("faces"), cluster_cases.reference("faces")
    cells = cluster_ref.cell_coords(c["xyz"], cluster_cases.T)
    assert np.abs(cells).max() == cluster_ref.CELL_LIMIT - 1  # the largest coordinates the grid accepts
    axes = {"face": 1, "edge": 2, "corner": 3}
    joined = {}
    for k, (base, direction, sign) in enumerate(c["pairs"]):
        diff = np.abs(cells[2 * k] - cells[2 * k + 1])
        assert diff.max() == 1 and diff.sum() == axes[direction], (base, direction)
        joined[(base, direction, sign)] = r["cluster_id"][2 * k] == r["cluster_id"][2 * k + 1]
    for base in ("origin", "near", "negative"):  # where float32 resolves 2^-20 of the tolerance
        for direction in axes:
            assert joined[(base, direction, -1.0)] and not joined[(base, direction, 1.0)], (base, direction)
    assert len(set(joined.values())) == 2


def test_input_edge_cases():
    c, r = cluster_cases.case("nan_mix"), cluster_cases.reference("nan_mix")
    bad = ~np.isfinite(c["xyz"]).all(axis=1)
    assert bad[0] and 10 < bad.sum() < 60 and (r["cluster_id"][bad] == -1).all() and r["first_index"][0] > 0
    assert r["n_clusters"] == 3 and (r["cluster_id"][c["labels"] == 9] == -1).all()
    z = cluster_cases.reference("all_ignored")
    assert z["n_kept"] == 0 and z["n_clusters"] == 0 and (z["cluster_id"] == -1).all()
    one = cluster_cases.reference("one_point")
    assert one["n_clusters"] == 1 and one["centroid"].tolist() == [[1.5, -2.5, 0.25]] and one["label"].tolist() == [6]
    nl = cluster_cases.reference("no_labels")
    assert nl["n_clusters"] == 3 and (nl["label"] == 0).all()
    two = cluster_cases.reference("two_label_blob")
    assert two["label"].tolist() == [3, 9, 0xFFFFFFFF] and two["count"].tolist() == [12, 8, 5]
