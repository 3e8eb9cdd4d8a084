"""CPU tests of the pose graph's algebra: the restatement (tests/pose_graph_ref.py) against central differences, the host
build of csrc/graph_edge.hpp against the restatement, the reference minimiser on a noiseless graph, and the host program
under the address and undefined-behaviour sanitizers."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import pose_graph_cases as cases
import pose_graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = os.path.join(ROOT, "profiles", "pose_graph", "figures.txt")

PROGRAM = textwrap.dedent(
    r"""
    // reads m, loss, a, then per edge Ti[7] Tj[7] z[7] Omega[36]; writes per edge r[6] s w rho Ci[42] Cj[42] B[36]
    #include <cstdio>
    #include <vector>
    #include "graph_edge.hpp"
    int main(int argc, char** argv) {
      if (argc != 3) return 2;
      FILE* f = std::fopen(argv[1], "rb");
      if (!f) return 2;
      double head[3];
      if (std::fread(head, sizeof(double), 3, f) != 3) return 2;
      const int m = (int)head[0], loss = (int)head[1];
      std::vector<double> in((size_t)m * 57), out((size_t)m * 129);
      if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
      std::fclose(f);
      for (int e = 0; e < m; ++e) {
        const double* p = in.data() + (size_t)e * 57;
        double* o = out.data() + (size_t)e * 129;
        double Or[6], Tji[7];
        sicp::graph::edge_error(p, p + 7, p + 14, p + 21, loss, head[2], o, Or, o + 6, o + 7, o + 8, Tji);
        sicp::graph::edge_blocks(o, Or, p + 21, o[7], Tji, o + 9, o + 51, o + 93);
      }
      f = std::fopen(argv[2], "wb");
      if (!f) return 2;
      std::fwrite(out.data(), sizeof(double), out.size(), f);
      std::fclose(f);
      return 0;
    }
    """
)


def build_program(tmp_path, name, flags=()):
    c = tmp_path / (name + ".cpp")
    c.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", *flags, "-I", os.path.join(ROOT, "semantic-icp_amd", "csrc"),
                    str(c), "-o", str(exe)], check=True)
    return exe


def run_program(exe, tmp_path, Ti, Tj, z, omega, kind, a):
    m = len(z)
    rows = np.concatenate([Ti, Tj, z, omega.reshape(m, 36)], axis=1)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([[float(m), float(kind), float(a)], rows.ravel()]).astype(np.float64).tofile(src)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    o = np.fromfile(dst, dtype=np.float64).reshape(m, 129)
    Ci, Cj = o[:, 9:51], o[:, 51:93]
    return {"r": o[:, :6], "s": o[:, 6], "w": o[:, 7], "rho": o[:, 8], "Hi": Ci[:, :36].reshape(m, 6, 6), "gi": Ci[:, 36:],
            "Hj": Cj[:, :36].reshape(m, 6, 6), "gj": Cj[:, 36:], "B": o[:, 93:].reshape(m, 6, 6)}


def write_figures(noise, tol):
    try:
        os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
        with open(FIGURES, "w") as f:
            f.write("pose graph: the restatement (float64) against np.longdouble on tests/pose_graph_cases.edge_cases()\n")
            f.write(f"largest discrepancy relative to a block's largest magnitude: {noise:.3e}\n")
            f.write(f"tolerance of the header and kernel comparisons (32 x): {tol:.3e}\n")
    except OSError:
        pass  # (a read-only tree: the figures are a record, not a check)


def test_series_and_closed_forms_agree_at_the_threshold():
    """just below the threshold the series run, at it the closed forms"""
    below, at = R.SERIES_THETA * (1 - 1e-12), R.SERIES_THETA
    th80 = np.array([below, at], dtype=np.longdouble)
    for c in R.coefficients(th80):
        # long double carries both branches to ~1e-19; the argument moved by 1e-12 relative and the coefficients' logarithmic
        # derivatives are below 1 here
        assert abs(c[0] - c[1]) <= 2e-12 * abs(c[1])
    eps = np.finfo(np.float64).eps
    for c64, c80 in zip(R.coefficients(np.array([below, at])), R.coefficients(th80)):
        # series: a few ulp.  Closed forms in double: the numerators cancel from terms of size 3 theta down to theta^5 / 60, so
        # the worst coefficient keeps 3 * 60 / theta^4 ulp; twice that is allowed -- an error that the theta^3 factor of its
        # term brings back to rounding level of the Jacobian
        assert abs(float(c64[0]) - float(c80[0])) <= 16 * eps * abs(float(c80[0]))
        assert abs(float(c64[1]) - float(c80[1])) <= 360 / at ** 4 * eps * abs(float(c80[1]))


def test_jacobians_match_central_differences():
    """dr/d delta_i and dr/d delta_j against central differences of the restated residual; the bound is the differences' own
    error, estimated by Richardson from a second step size"""
    Ti, Tj, z, omega, r_wanted = cases.edge_cases()
    m = len(z)
    E = cases.restated(Ti, Tj, z, omega, R.LOSS_NONE, 1.0)
    assert np.allclose(E["r"], r_wanted, atol=1e-9)

    def differences(h):
        Ji, Jj = np.empty((m, 6, 6)), np.empty((m, 6, 6))
        for k in range(6):
            d = np.zeros((m, 6), dtype=np.longdouble)
            d[:, k] = h
            for J, which in ((Ji, 0), (Jj, 1)):
                ends = [Ti.astype(np.longdouble), Tj.astype(np.longdouble)]
                plus, minus = list(ends), list(ends)
                plus[which] = R.mul(ends[which], R.exp(d))
                minus[which] = R.mul(ends[which], R.exp(-d))
                zz = z.astype(np.longdouble)
                J[:, :, k] = ((R.residual(plus[0], plus[1], zz) - R.residual(minus[0], minus[1], zz)) / (2 * h)).astype(np.float64)
        return Ji, Jj

    h = 1e-6
    Dh, D2h = differences(h), differences(2 * h)
    for name, dh, d2h in (("Ji", Dh[0], D2h[0]), ("Jj", Dh[1], D2h[1])):
        # central differences err by c h^2: D(2h) - D(h) = 3 c h^2, so the error of D(h) is a third of the gap; twice that, plus
        # the differences' rounding (eps_longdouble / h)
        bound = 2.0 * np.abs(d2h - dh).max(axis=(1, 2)) / 3.0 + 1e-19 / h * 16 * (1 + np.abs(dh).max(axis=(1, 2)))
        gap = np.abs(E[name] - dh).max(axis=(1, 2))
        assert np.all(gap <= bound), (name, gap.max(), bound[np.argmax(gap / bound)])


def test_header_host_build_matches_the_restatement(tmp_path):
    noise, tol = cases.header_tolerance()
    write_figures(noise, tol)
    assert noise < 1e-12
    exe = build_program(tmp_path, "edge")
    Ti, Tj, z, omega, _ = cases.edge_cases()
    for kind in (R.LOSS_NONE, R.LOSS_CAUCHY):
        got = run_program(exe, tmp_path, Ti, Tj, z, omega, kind, 1.5)
        want = cases.restated(Ti, Tj, z, omega, kind, 1.5)
        F = cases.floors(Ti, Tj, z, omega)
        for k in cases.BLOCKS:
            gap = cases.relative_gap(got[k], want[k], F[k])
            assert np.all(gap <= tol), (k, kind, float(gap.max()), tol)


def test_reference_minimiser_recovers_a_noiseless_graph():
    g = cases.ring(n=20, closures=3, seed=11, noise=False)
    rng = np.random.default_rng(0)
    start = R.mul(g["truth"], R.exp(rng.normal(size=(20, 6)) * 0.05))
    start[0] = g["truth"][0]
    x, info = R.minimise(start, g["fixed"], g["ei"], g["ej"], g["z"], g["omega"])
    # near the minimum cost = 1/2 g^T H^-1 g <= |g|^2 / (2 lambda_min) and the distance is |H^-1 g| <= |g| / lambda_min; both
    # with a factor 2 for the change of H between the iterate and the truth
    assert info["converged"]
    lam = np.linalg.eigvalsh(info["H"].toarray())[0]
    gn = np.linalg.norm(info["g"])
    assert lam > 0 and info["cost"] <= gn ** 2 / lam
    assert R.tangent_distance(x, g["truth"]) <= 2 * gn / lam
    assert np.array_equal(x[0], g["truth"][0])


def test_host_program_is_clean_under_the_sanitizers(tmp_path):
    exe = build_program(tmp_path, "edge_asan", flags=("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    Ti, Tj, z, omega, _ = cases.edge_cases()
    got = run_program(exe, tmp_path, Ti, Tj, z, omega, R.LOSS_CAUCHY, 1.5)
    assert np.all(np.isfinite(got["B"]))
