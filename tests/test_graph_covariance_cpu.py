"""CPU tests of the pose-graph covariances: the lock-step PCG restatement (tests/graph_cov_ref.py) against sparse LU solves,
the relative pose's Jacobian against central differences, the properties of the blocks, the host build of csrc/graph_cov.hpp,
the struct layouts, the default parameters and the binding's refusals that need no device."""
import ctypes
import functools
import importlib
import os
import subprocess
import textwrap

import numpy as np
import pytest

import graph_cov_ref as V
import pose_graph_cases as cases
import pose_graph_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")
TOLERANCE = 1e-10


@functools.lru_cache(maxsize=None)
def solved(name):
    g, kind, a, qa, qb = V.case(name)
    ref, st, H = V.reference(g, qa, qb, kind, a)
    got, st2, longest = V.restated(g, qa, qb, kind, a, TOLERANCE)
    return g, qa, qb, ref, st, H, got, st2, longest


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_lock_step_pcg_matches_sparse_lu(name):
    """per query, max |pcg - lu| / max |lu| under the a-priori bound of the stopping rule (graph_cov_ref.bound)"""
    g, qa, qb, ref, st, H, got, st2, longest = solved(name)
    assert np.array_equal(st, st2)
    lam = V.lambda_min(H)
    J = V.jacobian(g, qa, qb)
    worst = 0.0
    for q in range(len(qb)):
        if st[q] != V.OK:
            assert np.isnan(got[q]).all() and np.isnan(ref[q]).all()
            continue
        scale = np.abs(ref[q]).max()
        if scale == 0.0:
            assert not got[q].any()
            continue
        gap = np.abs(got[q] - ref[q]).max() / scale
        limit = V.bound(J[q], TOLERANCE, lam) / scale
        worst = max(worst, gap / limit)
        assert gap <= limit, (q, gap, limit)
    print(f"{name}: lambda_min {lam:.3e}, {longest} iterations, worst gap / bound {worst:.3e}")


def test_chain_asks_for_the_lone_node():
    g, qa, qb, ref, st, *_ = solved("chain_and_lone_node")
    assert (st == V.UNANCHORED).sum() >= 2 and (st == V.OK).sum() >= 3


def test_relative_jacobians_match_central_differences():
    """z(delta) = (T_a exp(d_a))^-1 (T_b exp(d_b)); log(z0^-1 z) = J_a d_a + J_b d_b to first order, J_b = I.  Central differences
    at h = 1e-6 carry eps |T| / h of rounding (3e-9 for translations of 30) and h^2 of truncation; 32 x that is 1e-7."""
    rng = np.random.default_rng(5)
    h = 1e-6
    for _ in range(8):
        Ta, Tb = cases.random_pose(rng, scale=10.0), cases.random_pose(rng, scale=10.0)
        Ja = V.jacobian_a(Ta, Tb)
        num_a, num_b = np.empty((6, 6)), np.empty((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            z0 = R.mul(R.inverse(Ta), Tb)
            num_a[:, k] = (R.residual(R.mul(Ta, R.exp(d)), Tb, z0) - R.residual(R.mul(Ta, R.exp(-d)), Tb, z0)) / (2 * h)
            num_b[:, k] = (R.residual(Ta, R.mul(Tb, R.exp(d)), z0) - R.residual(Ta, R.mul(Tb, R.exp(-d)), z0)) / (2 * h)
        assert np.abs(num_a - Ja).max() <= 1e-7 * max(1.0, np.abs(Ja).max())
        assert np.abs(num_b - np.eye(6)).max() <= 1e-7


@pytest.mark.parametrize("name", [n for n in V.CASE_NAMES if n != "hub11000"])
def test_blocks_are_symmetric_and_positive_semidefinite(name):
    g, qa, qb, ref, st, *_ = solved(name)
    fixed = np.asarray(g["fixed"], dtype=bool)
    for q in np.flatnonzero(st == V.OK):
        assert np.array_equal(ref[q], ref[q].T)
        assert np.linalg.eigvalsh(ref[q])[0] >= -1e-12 * np.abs(ref[q]).max()
        if fixed[qb[q]] and fixed[qa[q]]:
            assert not ref[q].any()


def test_a_fixed_end_gives_the_other_ends_marginal():
    """a fixed: cov = marginal(b).  b fixed: cov = J_a marginal(a) J_a^T.  Both fixed (the same node twice is refused, so a graph
    with two fixed nodes): zeros."""
    g = cases.ring(closures=8)
    f = int(np.flatnonzero(g["fixed"])[0])
    nodes = np.array([5, 17, 40], dtype=np.int32)
    marg, _, _ = V.reference(g, -np.ones(3, dtype=np.int32), nodes)
    rel_a, _, _ = V.reference(g, np.full(3, f, dtype=np.int32), nodes)
    rel_b, _, _ = V.reference(g, nodes, np.full(3, f, dtype=np.int32))
    assert np.array_equal(rel_a, marg)
    for k, n in enumerate(nodes):
        Ja = V.jacobian_a(g["poses"][n], g["poses"][f])
        want = Ja @ marg[k] @ Ja.T
        assert np.abs(rel_b[k] - want).max() <= 1e-12 * np.abs(want).max()
    g["fixed"][9] = True
    both, st, _ = V.reference(g, np.array([f, 9], dtype=np.int32), np.array([9, f], dtype=np.int32))
    assert not both.any() and not st.any()
    fm, _, _ = V.reference(g, np.array([-1], dtype=np.int32), np.array([9], dtype=np.int32))
    assert not fm.any()


PROGRAM = textwrap.dedent(
    r"""
    // reads m, then per pair Ta[7] Tb[7]; writes per pair J_a[36]
    #include <cstdio>
    #include <vector>
    #include "graph_cov.hpp"
    int main(int argc, char** argv) {
      if (argc != 3) return 2;
      FILE* f = std::fopen(argv[1], "rb");
      if (!f) return 2;
      double head;
      if (std::fread(&head, sizeof(double), 1, f) != 1) return 2;
      const int m = (int)head;
      std::vector<double> in((size_t)m * 14), out((size_t)m * 36);
      if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
      std::fclose(f);
      for (int e = 0; e < m; ++e) sicp::graph::relative_jacobian_a(in.data() + 14 * e, in.data() + 14 * e + 7, out.data() + 36 * e);
      f = std::fopen(argv[2], "wb");
      if (!f) return 2;
      std::fwrite(out.data(), sizeof(double), out.size(), f);
      std::fclose(f);
      return 0;
    }
    """
)


def test_header_host_build_matches_numpy(tmp_path):
    """-Ad(T_b^-1 T_a) is products of entries of size |t| and 1: at the tolerance of the edge header's comparison, relative to
    the block's largest entry"""
    c = tmp_path / "jac.cpp"
    c.write_text(PROGRAM)
    exe = tmp_path / "jac"
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "semantic-icp_amd", "csrc"), str(c), "-o", str(exe)], check=True)
    rng = np.random.default_rng(9)
    m = 64
    Ta, Tb = cases.random_pose(rng, m, scale=10.0), cases.random_pose(rng, m, scale=10.0)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([[float(m)], np.concatenate([Ta, Tb], axis=1).ravel()]).tofile(src)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(dst).reshape(m, 6, 6)
    want = V.jacobian_a(Ta, Tb)
    _, tol = cases.header_tolerance()
    gap = np.abs(got - want).reshape(m, -1).max(axis=1) / np.abs(want).reshape(m, -1).max(axis=1)
    assert gap.max() <= tol, (gap.max(), tol)


def test_struct_layouts_match_the_header(tmp_path):
    code = textwrap.dedent(
        """
        #include <stdio.h>
        #include <stddef.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %zu %zu\\n", sizeof(sicp_graph_cov_params), sizeof(sicp_graph_cov_info),
                 offsetof(sicp_graph_cov_params, max_columns), offsetof(sicp_graph_cov_info, worst_relative_residual));
          return 0;
        }
        """
    )
    c = tmp_path / "t.c"
    c.write_text(code)
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    a, b, o1, o2 = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert ctypes.sizeof(sicp.SicpGraphCovParams) == a and ctypes.sizeof(sicp.SicpGraphCovInfo) == b
    assert sicp.SicpGraphCovParams.max_columns.offset == o1 and sicp.SicpGraphCovInfo.worst_relative_residual.offset == o2


def test_default_cov_params_literals():
    p = sicp.default_graph_cov_params()
    assert (p.tolerance, p.max_cg_iterations, p.check_every, p.max_columns, p.reserved_) == (1e-10, 0, 32, 0, 0)
    assert sicp.default_graph_cov_params(max_columns=12, tolerance=1e-6).max_columns == 12
    assert (sicp.GRAPH_COV_OK, sicp.GRAPH_COV_NOT_CONVERGED, sicp.GRAPH_COV_UNANCHORED, sicp.GRAPH_COV_BREAKDOWN) == (0, 1, 2, 3)
    assert sicp.lib().sicp_default_graph_cov_params(None) == sicp.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("bad", [dict(tolerance=0.0), dict(tolerance=1.0), dict(tolerance=float("nan")), dict(max_cg_iterations=-1),
                                 dict(check_every=0), dict(max_columns=7), dict(max_columns=-6)])
def test_the_binding_refuses_bad_parameters_without_a_device(bad):
    with pytest.raises(ValueError):
        sicp.default_graph_cov_params(**bad)
    with pytest.raises(AttributeError):
        sicp.default_graph_cov_params(no_such_field=1)
