"""CPU tests of the pose graph's priors: the restatement (tests/pose_graph_prior_ref.py) against central differences, the host
build of csrc/graph_prior.hpp against the restatement and against node j's record of an edge from the identity pose, the
restatement's assembly against the identity-twin through the unchanged pose_graph_ref, the reference minimiser with priors on a
noiseless trajectory, and the host program under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess
import textwrap

import numpy as np

import pose_graph_cases as cases
import pose_graph_prior_ref as P
import pose_graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Rotation angles on both sides of the series threshold (0.25) and near pi.  3.1 is as near as the oracle goes: the restated log
# (pose_graph_ref.coefficients) forms (1 + cos theta) / sin theta, whose rounding grows like 1 / (pi - theta)^2 -- at
# pi - 3e-5 it is 1e-12 in float64 and swamps the central differences even in long double.
ANGLES = cases.RESIDUAL_ANGLES + (3.1,)

PROGRAM = textwrap.dedent(
    r"""
    // reads m, loss, a, then per prior kind T[7] z[7] Omega[36]; writes per prior r[6] s w rho C[42], and Cj[42] of the edge
    // (identity, T, z, Omega) where the prior is a pose prior (zeros otherwise)
    #include <cstdio>
    #include <vector>
    #include "graph_prior.hpp"
    int main(int argc, char** argv) {
      if (argc != 3) return 2;
      FILE* f = std::fopen(argv[1], "rb");
      if (!f) return 2;
      double head[3];
      if (std::fread(head, sizeof(double), 3, f) != 3) return 2;
      const int m = (int)head[0], loss = (int)head[1];
      std::vector<double> in((size_t)m * 51), out((size_t)m * 93, 0.0);
      if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
      std::fclose(f);
      const double identity[7] = {0, 0, 0, 1, 0, 0, 0};
      for (int p = 0; p < m; ++p) {
        const double* q = in.data() + (size_t)p * 51;
        double* o = out.data() + (size_t)p * 93;
        if ((int)q[0] == sicp::graph::kPriorPosition) {
          double Om3[9], Or[3];
          for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) Om3[3 * a + b] = q[15 + 6 * a + b];
          sicp::graph::prior_position_error(q + 1, q + 8, Om3, loss, head[2], o, Or, o + 6, o + 7, o + 8);
          sicp::graph::prior_position_blocks(q + 1, Or, Om3, o[7], o + 9);
        } else {
          double Or[6];
          sicp::graph::prior_pose_error(q + 1, q + 8, q + 15, loss, head[2], o, Or, o + 6, o + 7, o + 8);
          sicp::graph::prior_pose_blocks(o, Or, q + 15, o[7], o + 9);
          double r[6], s, w, rho, Tji[7], Ci[42], B[36];
          sicp::graph::edge_error(identity, q + 1, q + 8, q + 15, loss, head[2], r, Or, &s, &w, &rho, Tji);
          sicp::graph::edge_blocks(r, Or, q + 15, w, Tji, Ci, o + 51, B);
        }
      }
      f = std::fopen(argv[2], "wb");
      if (!f) return 2;
      std::fwrite(out.data(), sizeof(double), out.size(), f);
      std::fclose(f);
      return 0;
    }
    """
)


def prior_cases(seed=0, per_angle=3):
    """One-node graphs' worth of priors, as (poses [m, 7], priors with node = arange(m)).  Pose priors whose residual has a
    prescribed rotation angle (|r| = 0 among them), then position priors on poses whose own rotation has those angles."""
    rng = np.random.default_rng(seed)
    T, kind, z, om = [], [], [], []
    for angle in ANGLES:
        for k in range(per_angle):
            r = rng.normal(size=6)
            r[3:] *= angle / np.linalg.norm(r[3:])
            if angle == 0.0 and k == 0:
                r[:] = 0.0
            zz = cases.random_pose(rng)
            T.append(R.mul(zz, R.exp(r))); kind.append(P.POSE); z.append(zz); om.append(cases.random_spd(rng, 1)[0])
    for angle in ANGLES:
        for k in range(per_angle):
            w = rng.normal(size=3)
            xi = np.concatenate([rng.normal(size=3) * 3.0, w / np.linalg.norm(w) * angle])
            Tk = R.exp(xi)
            off = rng.normal(size=3) * (0.0 if (angle == 0.0 and k == 0) else 0.5)
            T.append(Tk); kind.append(P.POSITION); z.append(Tk[4:] + off); om.append(cases.random_spd(rng, 1)[0][:3, :3])
    return np.array(T), P.make(np.arange(len(T)), kind, z, om)


def build_program(tmp_path, name, flags=()):
    c = tmp_path / (name + ".cpp")
    c.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "semantic-icp_amd", "csrc"),
                    str(c), "-o", str(exe)], check=True)
    return exe


def run_program(exe, tmp_path, T, pri, kind, a):
    m = len(T)
    rows = np.concatenate([pri["kind"][:, None].astype(np.float64), T, pri["z"], pri["omega"].reshape(m, 36)], axis=1)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([[float(m), float(kind), float(a)], rows.ravel()]).astype(np.float64).tofile(src)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    o = np.fromfile(dst, dtype=np.float64).reshape(m, 93)
    return {"r": o[:, :6], "s": o[:, 6], "w": o[:, 7], "rho": o[:, 8], "H": o[:, 9:45].reshape(m, 6, 6), "g": o[:, 45:51],
            "Hj": o[:, 51:87].reshape(m, 6, 6), "gj": o[:, 87:93]}


def test_prior_jacobians_match_central_differences():
    """both priors' dr/d delta_k against central differences of their restated residuals in long double; the criterion of
    test_pose_graph_cpu.test_jacobians_match_central_differences: the differences' own error by Richardson"""
    T, pri = prior_cases()
    m = len(T)
    pos = pri["kind"] == P.POSITION
    J = P.jacobians(T, pri)
    T80, z80 = T.astype(np.longdouble), pri["z"].astype(np.longdouble)

    def residuals(Tk):
        r = np.zeros((m, 6), dtype=np.longdouble)
        r[~pos] = P.pose_residual(Tk[~pos], z80[~pos])
        r[pos, :3] = P.position_residual(Tk[pos], z80[pos, :3])
        return r

    def differences(h):
        D = np.empty((m, 6, 6))
        for k in range(6):
            d = np.zeros((m, 6), dtype=np.longdouble)
            d[:, k] = h
            D[:, :, k] = ((residuals(R.mul(T80, R.exp(d))) - residuals(R.mul(T80, R.exp(-d)))) / (2 * h)).astype(np.float64)
        return D

    h = 1e-6
    dh, d2h = differences(h), differences(2 * h)
    bound = 2.0 * np.abs(d2h - dh).max(axis=(1, 2)) / 3.0 + 1e-19 / h * 16 * (1 + np.abs(dh).max(axis=(1, 2)))
    gap = np.abs(J - dh).max(axis=(1, 2))
    assert np.all(gap <= bound), (gap.max(), bound[np.argmax(gap / bound)], int(np.argmax(gap / bound)))
    assert not J[pos, 3:].any() and not J[pos, :, 3:].any()  # a position prior says nothing about the rotation


def test_header_host_build_matches_the_restatement_and_the_identity_twin(tmp_path):
    _, tol = cases.header_tolerance()
    exe = build_program(tmp_path, "prior")
    T, pri = prior_cases()
    F = P.floors(T, pri)
    pose = pri["kind"] == P.POSE
    ident = np.tile(P.IDENTITY, (int(pose.sum()), 1))
    for kind in (R.LOSS_NONE, R.LOSS_CAUCHY):
        got = run_program(exe, tmp_path, T, pri, kind, 1.5)
        want = P.priors(T, pri, kind, 1.5)
        for k in ("r", "s", "w", "rho", "H", "g"):
            gap = cases.relative_gap(got[k], want[k], F[k])
            assert np.all(gap <= tol), (k, kind, float(gap.max()), tol)
        assert not got["r"][~pose, 3:].any() and not got["H"][~pose, 3:].any() and not got["H"][~pose, :, 3:].any() and not got["g"][~pose, 3:].any()
        # the pose prior's record is node j's record of the edge (identity, k, z, Omega): the header's own, and the restated edge's
        E = cases.restated(ident, T[pose], pri["z"][pose], pri["omega"][pose], kind, 1.5)
        for mine, theirs, floor in (("H", "Hj", "H"), ("g", "gj", "g")):
            assert np.all(cases.relative_gap(got[mine][pose], got[theirs][pose], F[floor][pose]) <= tol), (mine, kind)
            assert np.all(cases.relative_gap(got[mine][pose], E[theirs], F[floor][pose]) <= tol), (mine, kind)
        assert np.all(cases.relative_gap(got["r"][pose], E["r"], F["r"][pose]) <= tol)


def test_the_restated_assembly_is_the_identity_twins(tmp_path):
    """pose priors and disabled edges through this file's assemble, against pose_graph_ref.assemble on the twin graph"""
    g = cases.ring(20, 4, seed=51)
    g["fixed"][:] = False
    rng = np.random.default_rng(3)
    nodes = np.array([0, 7, 7, 13])
    pri = P.make(nodes, [P.POSE] * 4, R.mul(g["truth"][nodes], R.exp(rng.normal(size=(4, 6)) * 0.05)), cases.random_spd(rng, 4))
    e_on = np.ones(len(g["ei"]), dtype=bool)
    e_on[[3, 21]] = False
    p_on = np.array([True, True, False, True])
    for kind in (R.LOSS_NONE, R.LOSS_CAUCHY):
        c, grad, H = P.assemble(g["poses"], g, pri, e_on, p_on, kind, 2.0)
        t = P.identity_twin(g, pri, e_on, p_on)
        ct, gt, Ht = R.assemble(t["poses"], t["fixed"], t["ei"], t["ej"], t["z"], t["omega"], kind, 2.0)
        n6 = 6 * len(g["poses"])
        assert abs(c - ct) <= 1e-12 * ct
        assert np.abs(grad - gt[:n6]).max() <= 1e-10 * np.abs(gt).max()
        assert abs(H - Ht[:n6][:, :n6]).max() <= 1e-10 * abs(Ht).max()


def test_reference_minimiser_with_priors_recovers_a_noiseless_trajectory():
    """9 nodes, no fixed node: three position priors on nodes that are not collinear and one pose prior, all from the truth"""
    g = cases.ring(n=9, closures=2, seed=12, noise=False)
    g["fixed"][:] = False
    truth = g["truth"]
    held = np.array([1, 4, 7])
    assert np.linalg.matrix_rank(truth[held[1:], 4:] - truth[held[0], 4:]) == 2
    rng = np.random.default_rng(0)
    pri = P.make(list(held) + [0], [P.POSITION] * 3 + [P.POSE], [truth[k, 4:] for k in held] + [truth[0]],
                 [np.eye(3) * 1e4] * 3 + [cases.random_spd(rng, 1)[0]])
    start = R.mul(truth, R.exp(rng.normal(size=(9, 6)) * 0.05))
    x, info = P.minimise(g, pri, poses=start)
    assert info["converged"]
    lam = np.linalg.eigvalsh(info["H"].toarray())[0]
    gn = np.linalg.norm(info["g"])
    assert lam > 0 and info["cost"] <= gn ** 2 / lam
    assert R.tangent_distance(x, truth) <= 2 * gn / lam
    # the same without the pose prior: the three positions alone determine the trajectory
    x3, info3 = P.minimise(g, pri, p_on=[True, True, True, False], poses=start)
    lam3 = np.linalg.eigvalsh(info3["H"].toarray())[0]
    assert info3["converged"] and lam3 > 0 and R.tangent_distance(x3, truth) <= 2 * np.linalg.norm(info3["g"]) / lam3


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    exe = build_program(tmp_path, "prior_asan", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    T, pri = prior_cases()
    got = run_program(exe, tmp_path, T, pri, R.LOSS_CAUCHY, 1.5)
    assert np.all(np.isfinite(got["H"])) and np.all(np.isfinite(got["Hj"]))


def test_the_header_declares_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "sicp.h")).read()
    for name in ("sicp_graph_add_priors", "sicp_graph_set_edges_enabled", "sicp_graph_get_edges_enabled", "sicp_graph_set_priors_enabled",
                 "sicp_graph_get_priors_enabled", "sicp_graph_prior_errors", "sicp_graph_counts"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
    assert "SICP_GRAPH_PRIOR_POSE = 0" in text and "SICP_GRAPH_PRIOR_POSITION = 1" in text
