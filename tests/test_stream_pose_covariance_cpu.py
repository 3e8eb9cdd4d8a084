"""CPU tests of the pose covariance of stream registrations: the ABI only (the entry point and the submit flag in the header,
the library and the binding; refusals that happen before any device call)."""
import ctypes as C
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


def _header():
    src = open(os.path.join(ROOT, "include", "sicp.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_take_is_declared_and_exported():
    assert re.search(r"\bsicp_stream_take_pose_covariance\s*\(", _header())
    assert hasattr(C.CDLL(sicp.build()), "sicp_stream_take_pose_covariance")


def test_submit_flag_is_8_in_the_header_and_the_binding():
    m = re.search(r"\bSICP_SUBMIT_POSE_COVARIANCE\s*=\s*(\w+)", _header())
    assert m and int(m.group(1), 0) == 8
    assert sicp.SUBMIT_POSE_COVARIANCE == 8
    # the older flags keep their values; 4 stays unassigned
    assert (sicp.SUBMIT_FUSED_LABELS, sicp.SUBMIT_FRESH_FEATURES) == (1, 2)
    assert not re.search(r"\bSICP_SUBMIT_\w+\s*=\s*4\b", _header())


def test_null_stream_is_refused_before_any_device_call():
    lib = sicp.lib()
    r = sicp.SicpPoseCovarianceResult()
    C.memset(C.byref(r), 0x5A, C.sizeof(r))
    before = bytes(r)
    assert lib.sicp_stream_take_pose_covariance(None, 1, 1.0, 1.0, C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_stream_take_pose_covariance(None, 1, -1.0, 1.0, C.byref(r)) == sicp.ERR_INVALID_ARGUMENT
    assert lib.sicp_stream_take_pose_covariance(None, 1, 1.0, 1.0, None) == sicp.ERR_INVALID_ARGUMENT
    assert bytes(r) == before
