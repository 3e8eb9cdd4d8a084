"""CPU tests of what tests/test_gpu_plane.py stands on (tests/plane_ref.py, tests/plane_cases.py) and of the binding's side of
sicp_segment_planes: the restated Jacobi is held against np.linalg.eigh by cov_ref's eigen-residual ratio on every refined
plane of every case; the cases have the properties they are named for; the restatement finds the road of the street scan; the
structs and defaults agree with include/sicp.h."""
import ctypes
import importlib
import os
import subprocess
import textwrap

import numpy as np
import pytest

import bootstrap_ref
import cluster_cases
import cov_cases
import cov_ref
import plane_cases
import plane_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


# ---- the binding -------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_defaults_match_the_header(tmp_path):
    code = textwrap.dedent(
        """
        #include <stdio.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %d %d %d\\n", sizeof(sicp_plane_params), sizeof(sicp_plane_info), SICP_PLANE_MAX_HYPOTHESES, SICP_PLANE_MAX_PLANES,
                 SICP_PLANE_MAX_IGNORE);
          return 0;
        }
        """
    )
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    a, b, mh, mp, mi = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(sicp.SicpPlaneParams) == a and ctypes.sizeof(sicp.SicpPlaneInfo) == b
    assert (sicp.PLANE_MAX_HYPOTHESES, sicp.PLANE_MAX_PLANES, sicp.PLANE_MAX_IGNORE) == (mh, mp, mi)
    assert (plane_ref.MAX_HYPOTHESES, plane_ref.MAX_PLANES, plane_ref.MAX_IGNORE) == (mh, mp, mi)
    p = sicp.default_plane_params()
    d = plane_ref.DEFAULTS
    assert (p.distance_threshold, p.min_cos, p.seed, p.num_hypotheses, p.max_planes, p.min_inliers, p.refine, p.n_ignore) == (
        d["distance_threshold"], d["min_cos"], d["seed"], d["num_hypotheses"], d["max_planes"], d["min_inliers"], d["refine"], 0)
    assert (0.2, 0.0, 1, 1024, 1, 100, 1) == (p.distance_threshold, p.min_cos, p.seed, p.num_hypotheses, p.max_planes, p.min_inliers, p.refine)
    assert list(p.axis) == [0.0, 0.0, 0.0] and list(p.ignore) == [0] * 16
    q = sicp.default_plane_params(ignore=(3, 9), axis=(0, 0, 1), min_cos=0.9, seed=7)
    assert (q.n_ignore, q.ignore[0], q.ignore[1], list(q.axis), q.min_cos, q.seed) == (2, 3, 9, [0.0, 0.0, 1.0], 0.9, 7)
    with pytest.raises(ValueError):
        sicp.default_plane_params(ignore=range(17))
    with pytest.raises(AttributeError):
        sicp.default_plane_params(no_such_field=1)
    assert callable(sicp.Engine.segment_planes)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_the_draws_are_the_bootstrap_generator():
    for seed in (1, 2, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0):
        g = bootstrap_ref.SplitMix64(seed)
        want = [g.next() for _ in range(40)]
        assert plane_ref.draws(seed, 0, 40).tolist() == want
        assert plane_ref.draws(seed, 17, 5).tolist() == want[17:22]
    g = bootstrap_ref.SplitMix64(5)
    want = [g.index(1000) for _ in range(12)]
    assert plane_ref.sample_indices(5, 0, 4, 1000).ravel().tolist() == want
    assert plane_ref.sample_indices(5, 1, 2, 1000).ravel().tolist() == want[6:12]


@pytest.mark.parametrize("name", plane_cases.NAMES)
def test_the_restated_jacobi_agrees_with_eigh(name):
    """a line-for-line Jacobi can share a defect with the kernel: every refined plane's normal is an eigenvector of the matrix the
    solver was given, of the eigenvalue of smallest magnitude, to cov_ref's bars"""
    ref = plane_cases.reference(name)
    if plane_cases.case(name)["params"]["refine"]:
        assert len(ref["fits"]) == ref["n_planes"]
    for Q, S, u in ref["fits"]:
        A = np.array([[Q[0], Q[1], Q[3]], [Q[1], Q[2], Q[4]], [Q[3], Q[4], Q[5]]])
        ratio = float(cov_ref.ratio(A[None], np.array([S]), np.array([u]))[0])
        unit = float(cov_ref.unit_error(np.array([u]))[0])
        w, v = np.linalg.eigh(A)
        k = int(np.argmin(np.abs(w)))
        print(f"{name}: ratio {ratio:.3f} (bar {cov_cases.GAMMA:.3f})  unit {unit:.2e} (bar {cov_ref.UNIT_BOUND:.2e})  |n . eigh| {abs(float(np.dot(v[:, k], u))):.15f}")
        assert unit <= cov_ref.UNIT_BOUND
        assert ratio <= cov_cases.GAMMA


def test_the_tree_sum_does_not_depend_on_the_run():
    """the kernel's tree -- runs of TREE_RUN, then runs of the partial sums -- is the rule's perfect tree with subtrees of +0.0"""
    rng = np.random.default_rng(3)
    for n in (1, 2, 511, 512, 513, 1613, 5000):
        v = rng.normal(size=n)
        present = rng.uniform(size=n) < 0.7
        want = plane_ref.tree(v, present, n)
        s = np.where(present, v, 0.0)
        while len(s) > 1:
            pad = np.zeros(-len(s) % 512)
            s = np.concatenate([s, pad]).reshape(-1, 512)
            while s.shape[1] > 1:
                s = s[:, 0::2] + s[:, 1::2]
            s = s[:, 0]
        assert np.float64(s[0] + 0.0).tobytes() == np.float64(want).tobytes(), n
    assert np.float64(plane_ref.tree(np.array([-0.0, -0.0]), np.array([True, True]), 2)).tobytes() == np.float64(0.0).tobytes()


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def test_cases_have_the_properties_they_are_named_for():
    R, Cs = plane_cases.reference, plane_cases.case
    for name in plane_cases.DEGENERATE:
        r = R(name)
        assert (r["n_planes"], r["rounds"], r["n_invalid_hypotheses"], r["n_assigned"]) == (0, 1, Cs(name)["params"]["num_hypotheses"], 0), name
        assert (r["plane_id"] == -1).all()
    r = R("room_corner")
    assert (r["n_planes"], r["rounds"]) == (3, 4) and (r["count"] >= 290).all()
    lab = Cs("room_corner")["labels"]
    for k in range(3):  # each plane is one wall
        assert len(set(lab[r["plane_id"] == k].tolist()) - {4}) == 1
    r = R("three_points")
    assert (r["n_planes"], r["count"].tolist(), r["n_candidates"]) == (1, [3], 3)
    for n in plane_cases.TILE_SIZES[:3]:
        assert R(f"tile_{n}")["n_candidates"] == n
    r = R(f"tile_{plane_cases.TILE_SIZES[3]}")
    assert 2 * plane_cases.TILE < r["n_candidates"] < r["n_finite"] < r["n_points"]
    for H in plane_cases.HYPOTHESES:
        r = R(f"hypotheses_{H}")
        assert r["n_planes"] >= 1 and (r["hyp_index"] < H).all()
    r = R("nan_mix")
    bad = ~np.isfinite(Cs("nan_mix")["xyz"]).all(axis=1)
    assert bad.sum() == 4 and r["n_finite"] == r["n_points"] - 4 and (r["plane_id"][bad] == -1).all() and r["n_planes"] == 1
    c, r = Cs("ignore_mask"), R("ignore_mask")
    out = (c["mask"] == 0) | np.isin(c["labels"], (3, 7))
    assert r["n_candidates"] == (~out).sum() and (r["plane_id"][out] == -1).all() and r["n_planes"] == 1
    assert len(set(Cs("interleaved")["labels"].tolist())) == 3 and R("interleaved")["n_planes"] >= 1
    assert Cs("no_labels")["labels"] is None and R("no_labels")["n_planes"] == 1
    for name in plane_cases.STREET:
        assert R(name)["n_planes"] == 4, name


def test_every_valid_hypothesis_of_the_lattice_ties_and_the_first_wins():
    c, r = plane_cases.case("lattice_ties"), plane_cases.reference("lattice_ties")
    p = c["params"]
    P = c["xyz"].astype(np.float64)
    idx = plane_ref.sample_indices(p["seed"], 0, p["num_hypotheses"], len(P))
    a, n, nn, thr, valid = plane_ref.hypotheses(P, idx, np.float64(p["distance_threshold"]) ** 2, None, 0.0)
    sc = plane_ref.scores(P, a, n, thr, valid)
    assert 0 < (~valid).sum() < len(valid) and (sc[valid] == len(P)).all()
    assert r["hyp_index"].tolist() == [int(np.flatnonzero(valid)[0])] and r["count"].tolist() == [len(P)]
    assert r["n_invalid_hypotheses"] == (~valid).sum()


def test_a_point_at_the_threshold_is_inside_and_one_ulp_beyond_is_outside():
    c, r = plane_cases.case("threshold_edge"), plane_cases.reference("threshold_edge")
    assert r["n_planes"] == 1 and r["count"].tolist() == [65]
    assert r["coeff"][0, :3].tolist() == [0.0, 0.0, 1.0]
    assert r["plane_id"][plane_cases.AT_T] == 0 and r["plane_id"][plane_cases.BEYOND_T] == -1
    assert float(c["xyz"][plane_cases.AT_T, 2]) == c["params"]["distance_threshold"] < float(c["xyz"][plane_cases.BEYOND_T, 2])
    assert (r["plane_id"][:64] == 0).all()


# ---- the road ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("H", [64, 256])
def test_the_first_plane_of_the_street_scan_is_the_road(seed, H):
    xyz, lab = cluster_cases._street_scan()
    r = plane_ref.segment_planes(xyz, lab, None, distance_threshold=0.1, axis=plane_cases.Z, min_cos=0.95, seed=seed, num_hypotheses=H)
    road = lab == 1
    share = float((r["plane_id"][road] == 0).mean())
    others = int(((r["plane_id"] == 0) & ~road).sum())
    print(f"seed {seed} H {H}: {100 * share:.2f} % of the {int(road.sum())} label-1 points, {others} points of other labels, |n_z| {abs(r['coeff'][0, 2]):.6f}")
    assert share >= 0.95
    assert abs(r["coeff"][0, 2]) >= 0.99


def test_two_seeds_give_different_hypotheses():
    a = plane_cases.reference("street_refine1_z")
    c = plane_cases.case("street_refine1_z")
    b = plane_ref.segment_planes(c["xyz"], c["labels"], c["mask"], **dict(c["params"], seed=2))
    assert a["hyp_index"].tolist() != b["hyp_index"].tolist()
    assert abs(a["coeff"][0, 2]) > 0.99 and abs(b["coeff"][0, 2]) > 0.99


def test_the_restatement_refuses_what_the_header_refuses():
    xyz = plane_cases.case("no_labels")["xyz"]
    nan, inf = float("nan"), float("inf")
    for bad in (dict(distance_threshold=0.0), dict(distance_threshold=-1.0), dict(distance_threshold=nan), dict(distance_threshold=inf),
                dict(axis=(0, nan, 1), min_cos=0.5), dict(axis=(0, 0, 1)), dict(axis=(0, 0, 1), min_cos=1.5), dict(axis=(0, 0, 1), min_cos=-0.5),
                dict(min_cos=0.5), dict(num_hypotheses=0), dict(num_hypotheses=4097), dict(max_planes=0), dict(max_planes=17),
                dict(min_inliers=2), dict(refine=2), dict(ignore=(3,)), dict(ignore=tuple(range(17)))):
        with pytest.raises(ValueError):
            plane_ref.segment_planes(xyz, None, None, **bad)
    with pytest.raises(plane_ref.TooFewPoints):
        plane_ref.segment_planes(xyz[:2])
    mask = np.zeros(len(xyz), np.uint8)
    mask[[4, 9]] = 1
    with pytest.raises(plane_ref.TooFewPoints):
        plane_ref.segment_planes(xyz, None, mask)
