"""CPU tests of sicp_evaluate: the ABI (symbols, struct layout, refusals before any device call) and the numpy restatement
of its semantics (tests/evaluate_ref.py) against a literal transcription of ROCMetrics::evaluate (exec/roc_metrics.h:21-41)."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess
import tempfile
import textwrap

import numpy as np

import evaluate_ref as ref
import np_ref
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")
FIELDS = ("n_source", "inliers", "label_agree", "label_outside", "sum_d2", "fitness", "inlier_rmse", "reserved_")


def test_entry_points_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "sicp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sicp_evaluate", "sicp_evaluate_batch"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert hasattr(C.CDLL(sicp.build()), name), name


def test_result_struct_matches_the_c_compiler():
    offsets = ", ".join(f"offsetof(sicp_evaluate_result, {f})" for f in FIELDS)
    code = textwrap.dedent(
        """
        #include <stddef.h>
        #include <stdio.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu" FORMAT "\\n", sizeof(sicp_evaluate_result), OFFSETS);
          return 0;
        }
        """
    ).replace("FORMAT", ' " %zu"' * len(FIELDS)).replace("OFFSETS", offsets)
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()))
    R = sicp.SicpEvaluateResult
    assert C.sizeof(R) == got[0] == 64
    assert [getattr(R, f).offset for f in FIELDS] == got[1:]
    assert "reserved_" not in R().as_dict()


def test_refusals_happen_before_any_device_call():
    """with NULL handles nothing can reach the device: every refusal below is decided by the arguments alone"""
    lib = sicp.lib()
    qt = np.array([0, 0, 0, 1, 0, 0, 0.0])
    qp = qt.ctypes.data_as(C.POINTER(C.c_double))
    r = sicp.SicpEvaluateResult()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    before = bytes(r)
    conf = np.full(9, 77, dtype=np.int64)
    cp = conf.ctypes.data_as(C.POINTER(C.c_int64))
    idx = np.full(4, 77, dtype=np.int32)
    d2 = np.full(4, 77, dtype=np.float32)
    ip, fp = idx.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_float))
    bad = sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_evaluate(None, qp, 25.0, 3, cp, ip, fp, C.byref(r)) == bad          # NULL handle
    assert lib.sicp_evaluate(None, None, 25.0, 0, None, None, None, C.byref(r)) == bad  # ... and qt
    assert lib.sicp_evaluate(None, qp, 25.0, 0, None, None, None, None) == bad          # ... and out
    for gate in (float("nan"), 0.0, -1.0, -float("inf")):
        assert lib.sicp_evaluate(None, qp, gate, 3, cp, ip, fp, C.byref(r)) == bad
    for classes in (0, -1, 256):
        assert lib.sicp_evaluate(None, qp, 25.0, classes, cp, ip, fp, C.byref(r)) == bad
    assert bytes(r) == before and (conf == 77).all() and (idx == 77).all() and (d2 == 77).all()

    status = np.full(2, 77, dtype=np.int32)
    sp = status.ctypes.data_as(C.POINTER(C.c_int32))
    hs = (C.c_void_p * 2)(None, None)
    qts = np.tile(qt, 2)
    qsp = qts.ctypes.data_as(C.POINTER(C.c_double))
    outs = (sicp.SicpEvaluateResult * 2)()
    C.memset(outs, 0x5A, C.sizeof(outs))
    outs_before = bytes(outs)
    conf2 = np.full(18, 77, dtype=np.int64)
    cp2 = conf2.ctypes.data_as(C.POINTER(C.c_int64))
    assert lib.sicp_evaluate_batch(None, 2, qsp, 25.0, 3, cp2, outs, sp) == bad   # NULL array
    assert lib.sicp_evaluate_batch(hs, 0, qsp, 25.0, 3, cp2, outs, sp) == bad     # n < 1
    assert lib.sicp_evaluate_batch(hs, -3, qsp, 25.0, 3, cp2, outs, sp) == bad
    assert lib.sicp_evaluate_batch(hs, 2, qsp, 25.0, 3, cp2, outs, sp) == bad     # NULL handles
    assert lib.sicp_evaluate_batch(hs, 2, None, 25.0, 3, cp2, outs, sp) == bad
    assert lib.sicp_evaluate_batch(hs, 2, qsp, 25.0, 3, cp2, None, sp) == bad
    for gate in (float("nan"), 0.0, -2.0):
        assert lib.sicp_evaluate_batch(hs, 2, qsp, gate, 3, cp2, outs, sp) == bad
    for classes in (0, 256):
        assert lib.sicp_evaluate_batch(hs, 2, qsp, 25.0, classes, cp2, outs, sp) == bad
    assert (status == 77).all() and (conf2 == 77).all() and bytes(outs) == outs_before


def test_restatement_matches_the_roc_metrics_loop():
    """300 x 300 labelled points: the restatement's inliers, label pairs and table are those ROCMetrics::evaluate prints"""
    src, sl, tgt, tl, T_gt, _ = synth.lidar_pair(seed=7, n_points=300)
    C_ = 11
    for M in (np.eye(4), T_gt):
        qt = np_ref.mat_to_qt(M)
        got = ref.evaluate(src, tgt, qt, 25.0, sl, tl, C_)
        lines = ref.roc_metrics_loop(np_ref.transform_points(np_ref.qt_to_mat(qt), src), sl, tgt, tl)
        assert got["n_source"] == 300 and 0 < len(lines)
        assert got["inliers"] == len(lines)
        inl = got["nn_idx"] >= 0
        assert [(int(a), int(b)) for a, b in zip(sl[inl], tl[got["nn_idx"][inl]])] == lines
        want = np.zeros((C_, C_), dtype=np.int64)
        for a, b in lines:
            want[a - 1, b - 1] += 1
        assert np.array_equal(got["confusion"], want) and got["label_outside"] == 0
        assert got["label_agree"] == sum(a == b for a, b in lines) == int(np.trace(want))
        assert got["fitness"] == len(lines) / 300
        assert got["inlier_rmse"] == math.sqrt(got["sum_d2"] / len(lines))


def test_restatement_edges():
    rng = np.random.default_rng(3)
    src = rng.uniform(0, 4, (50, 3)).astype(np.float32)
    tgt = rng.uniform(0, 4, (60, 3)).astype(np.float32)
    src[[3, 17]] = np.nan
    tgt[5, 1] = np.inf
    sl, tl = rng.integers(1, 6, 50).astype(np.uint32), rng.integers(1, 6, 60).astype(np.uint32)
    qt = np.array([0, 0, 0, 1, 0, 0, 0.0])
    got = ref.evaluate(src, tgt, qt, np.inf, sl, tl, 3)
    assert got["n_source"] == got["inliers"] == 48 and (got["nn_idx"][[3, 17]] == -1).all() and np.isnan(got["nn_d2"][[3, 17]]).all()
    assert 5 not in got["nn_idx"]
    assert got["label_outside"] > 0 and got["label_outside"] + got["confusion"].sum() == 48
    none = ref.evaluate(src, tgt, qt, 1e-12, sl, tl, 3)
    assert none["inliers"] == 0 and math.isnan(none["inlier_rmse"]) and none["fitness"] == 0.0 and none["sum_d2"] == 0.0
    assert np.array_equal(none["nn_d2"], got["nn_d2"], equal_nan=True)  # (the d^2 stays as found)
    # the gate is strict and in float32: a d^2 equal to (float) max_dist_sq is no inlier
    d = float(np.nanmin(got["nn_d2"]))
    assert ref.evaluate(src, tgt, qt, d, sl, tl)["inliers"] == 0
    assert ref.evaluate(src, tgt, qt, float(np.nextafter(np.float32(d), np.float32(np.inf))), sl, tl)["inliers"] >= 1
