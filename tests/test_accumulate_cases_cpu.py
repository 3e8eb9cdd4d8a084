"""CPU tests of what tests/test_gpu_accumulate_paths.py stands on (tests/accumulate_cases.py): the Python restatement of
acc_geometry against csrc/kernels.h compiled for the host, every edge size on the intended side of its boundary, the
dynamic hand-out's handle counts, the np.longdouble restatement against the oracle, and -- on the oracle alone -- that a
single removed slot at each edge moves the 28 sums by more than 1000 bars (a test that passes with the slot missing has no
teeth)."""
import os
import subprocess
import textwrap

import numpy as np
import pytest

import accumulate_cases as A
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEOMETRY_TOTALS = sorted({0, 1, 2, 3, 4, 5, 7, 8, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385, 16388, 2048 * 1024 - 1,
                          2048 * 1024, 2048 * 1024 + 1, 2048 * 1024 + 4, 3 * 2048 * 1024 + 5, 5 * 10 ** 8}
                         | {n * K for K, sizes in A.EDGE_SIZES.items() for n in sizes}
                         | {v[2] * v[1] for v in A.DYNAMIC_CASES.values()})

CODE = textwrap.dedent(
    r"""
    #include <cstdio>
    #include <cstdlib>
    #include "kernels.h"
    int main(int argc, char** argv) {
      for (int k = 1; k < argc; ++k) {
        const int total = std::atoi(argv[k]);
        for (int K : {1, 4, 20}) {
          const sicp::AccGeometry g = sicp::acc_geometry(total, sicp::acc_slots_per_group(K));
          std::printf("%d %d %d %d %d %d %d\n", total, K, sicp::acc_slots_per_group(K), g.n_groups, g.steps, g.chunk_groups, g.n_chunks);
        }
      }
      return 0;
    }
    """
)


def test_python_acc_geometry_equals_the_header(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = tmp_path / "geo.cpp"
    src.write_text(CODE)
    exe = tmp_path / "geo"
    cmd = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-I", os.path.join(ROOT, "semantic-icp_amd", "csrc"), "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)] + [str(t) for t in GEOMETRY_TOTALS], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]
    assert len(rows) == 3 * len(GEOMETRY_TOTALS)
    for total, K, spg, n_groups, steps, chunk_groups, n_chunks in rows:
        assert A.slots_per_group(K) == spg
        assert A.acc_geometry(total, spg) == dict(n_groups=n_groups, steps=steps, chunk_groups=chunk_groups, n_chunks=n_chunks), (total, K)


def test_a_chunk_is_2048_slots_up_to_1024_chunks():
    for K in (1, 4, 20):
        spg = A.slots_per_group(K)
        g = A.acc_geometry(1024 * A.CHUNK_SLOTS, spg)
        assert g["chunk_groups"] * spg == A.CHUNK_SLOTS and g["n_chunks"] == 1024 and g["steps"] == 8 // spg
        g = A.acc_geometry(1024 * A.CHUNK_SLOTS + spg, spg)
        assert g["chunk_groups"] * spg == 2 * A.CHUNK_SLOTS and g["n_chunks"] == 513


@pytest.mark.parametrize("K", sorted(A.EDGE_SIZES))
def test_every_edge_size_lies_on_the_intended_side(K):
    assert {k for k in A.EDGE_EXPECT if k[0] == K} == {(K, n) for n in A.EDGE_SIZES[K]}
    for n in A.EDGE_SIZES[K]:
        assert (A.n_chunks(n, K), A.ragged_last_group(n, K)) == A.EDGE_EXPECT[(K, n)], (K, n)
    per_chunk = A.CHUNK_SLOTS / K
    sizes = A.EDGE_SIZES[K]
    # both sides of the first chunk boundary, and of the 8-chunk parking boundary
    assert max(n for n in sizes if A.n_chunks(n, K) == 1) == int(per_chunk)
    assert min(n for n in sizes if A.n_chunks(n, K) == 2) == int(per_chunk) + 1
    assert {A.n_chunks(n, K) for n in sizes} >= {A.COMB_CHUNKS, A.COMB_CHUNKS + 1}
    assert min(n for n in sizes if A.n_chunks(n, K) == A.COMB_CHUNKS + 1) - max(n for n in sizes if A.n_chunks(n, K) == A.COMB_CHUNKS) <= 2
    if K == 1:   # two source points per group: odd sizes leave the second one past the end
        assert all(A.ragged_last_group(n, 1) == n % 2 for n in sizes) and {n % 2 for n in sizes} == {0, 1}
    if K == 20:  # chunk boundaries inside a source point's slots: 2048 is no multiple of 20
        assert A.CHUNK_SLOTS % K != 0 and all((c * A.CHUNK_SLOTS) % K != 0 for c in (1, 2, 8))
    # one lane of the first wave, one wave, one workgroup step: sizes on either side of 64 / 256 groups
    if K == 4:
        assert {255, 256, 257} <= set(sizes)


@pytest.mark.parametrize("cus", [256, 304, 64])
def test_handle_counts_of_the_dynamic_hand_out(cus):
    for name, (mode, knn, n_s) in A.DYNAMIC_CASES.items():
        n = A.handles_for_dynamic(cus, n_s, knn)
        assert n <= A.MAX_PAIRS, (name, cus, n)
        assert n * A.n_chunks(n_s, knn) >= A.dynamic_threshold(cus) > (n - 1) * A.n_chunks(n_s, knn)
        assert A.n_chunks(n_s, knn) < A.dynamic_threshold(cus)                     # a lone pair: static ranges
        assert (n_s * knn) % A.CHUNK_SLOTS != 0                                    # ragged last chunk
    assert A.dynamic_threshold(256) == 32768
    assert A.n_chunks(130877, 4) == 256 and A.n_chunks(59999, 20) == 586
    assert (A.handles_for_dynamic(256, 130877, 4), A.handles_for_dynamic(256, 59999, 20)) == (128, 56)
    # K = 1: even the largest synthetic scan is short of the threshold over the 256 pairs of a launch
    assert A.MAX_PAIRS * A.n_chunks(150000, 1) < A.dynamic_threshold(256)


def test_residency_boundary_of_the_persistent_solve():
    assert (A.largest_source_with_chunks(255, 20), A.n_chunks(26112, 20), A.n_chunks(26113, 20)) == (26112, 255, 256)
    assert A.solo_fits(26112, 20, 256) and not A.solo_fits(26113, 20, 256)
    for cus in (64, 256, 304):
        n = A.largest_source_with_chunks(min(cus, 257) - 1, 20)
        assert A.solo_fits(n, 20, cus) and not A.solo_fits(n + 1, 20, cus)


# ---- the oracle alone -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_slots():
    """the 20 000-point pair with the oracle's own covariances and neighbours at the true pose, gate wide open"""
    src, sl, tgt, tl, qt = A.pair20k()
    scov = O.covariances(src, None, 20, 1e-3, kdtree=True)[0]
    tcov = O.covariances(tgt, None, 20, 1e-3, kdtree=True)[0]
    idx20, _ = O.knn(O.transform_points(O.se3_matrix(qt), src), tgt, 20, kdtree=True)
    w20 = np.random.default_rng(3).uniform(0.05, 1.0, idx20.shape)
    idx20 = idx20.astype(np.int32)
    idx20.setflags(write=False); w20.setflags(write=False)
    return src, scov, tgt, tcov, qt, idx20, w20


@pytest.mark.parametrize("mode,knn,sq,a", [(O.MODE_EM, 4, 1, 3.0), (O.MODE_GICP, 1, 1, 3.0), (O.MODE_SEMANTIC, 1, 0, 1.5), (O.MODE_EM, 20, 0, 0.05),
                                           (O.MODE_EM, 4, 1, 0.05), (O.MODE_GICP, 1, 0, 50.0)])
def test_longdouble_restatement_equals_the_oracle(oracle_slots, mode, knn, sq, a):
    src, scov, tgt, tcov, qt, idx20, w20 = oracle_slots
    n = 1500
    idx, w = idx20[:n, :knn].copy(), w20[:n, :knn].copy()
    idx[::7, 0] = -1
    p = A.oracle_params(mode, knn=knn, use_sqloss=sq, cauchy_a=a)
    ref = O.accumulate(p, qt, src[:n], scov[:n], tgt, tcov, idx, w if mode == O.MODE_EM else None)
    ld = A.accumulate_longdouble(p, qt, src[:n], scov[:n], tgt, tcov, idx, w if mode == O.MODE_EM else None)
    q, err = A.excess(ld.astype(np.float64), ref, A.project_bars(ref))
    print(f"{A.case_id(mode, knn, sq, a)}: oracle against longdouble, worst err / bar = {q:.3g}")
    assert q <= 1.0, (q, err)


@pytest.mark.parametrize("mode,knn,n_s", A.EDGE_CASES, ids=[A.case_id(*c) for c in A.EDGE_CASES])
def test_a_removed_slot_at_each_edge_moves_the_reference(oracle_slots, mode, knn, n_s):
    src, scov, tgt, tcov, qt, idx20, w20 = oracle_slots
    idx, w = idx20[:n_s, :knn].copy(), w20[:n_s, :knn].copy() if mode == O.MODE_EM else None
    p = A.oracle_params(mode, knn=knn)
    ref = O.accumulate(p, qt, src[:n_s], scov[:n_s], tgt, tcov, idx, w)
    for what, less in A.removals(idx).items():
        assert (less < 0).sum() >= 1 and (less != idx).sum() == (less < 0).sum(), what
        other = O.accumulate(p, qt, src[:n_s], scov[:n_s], tgt, tcov, less, w)
        assert A.moved_beyond(ref, other), (what, np.abs(other - ref) / A.project_bars(ref))
