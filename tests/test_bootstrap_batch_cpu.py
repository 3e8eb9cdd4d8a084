"""CPU tests of sicp_bootstrap_batch (the bootstrap of many pairs in one call): the symbol is declared and exported, and
the call refuses bad arguments before it touches a device -- so on a machine without a GPU it answers a status and does
not crash."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sicp = importlib.import_module("semantic-icp_amd")


def test_bootstrap_batch_is_declared_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sicp.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sicp_bootstrap_batch\s*\(\s*sicp_handle\s*\*\s*hs\s*,\s*int32_t\s+n\s*,", src)
    lib = C.CDLL(sicp.build())
    assert hasattr(lib, "sicp_bootstrap_batch")
    assert hasattr(sicp, "bootstrap_batch")


def _call(hs, n, params=True, out=True, status=None):
    p = sicp.default_bootstrap_params()
    qt = np.full((max(n, 1), 7), 7.0)
    st = status if status is not None else np.full(max(n, 1), 99, dtype=np.int32)
    rc = sicp.lib().sicp_bootstrap_batch(hs, n, C.byref(p) if params else None,
                                         qt.ctypes.data_as(C.POINTER(C.c_double)) if out else None,
                                         st.ctypes.data_as(C.POINTER(C.c_int32)), None)
    return rc, qt, st


def test_refusals_come_before_any_device_call():
    none2 = (C.c_void_p * 2)(None, None)
    for hs, n, kw in ((none2, 0, {}), (none2, -3, {}), (None, 2, {}), (none2, 2, {}), (none2, 1, dict(params=False)),
                      (none2, 1, dict(out=False))):
        rc, qt, st = _call(hs, n, **kw)
        assert rc == sicp.ERR_INVALID_ARGUMENT
        assert (qt == 7.0).all() and (st == 99).all()  # nothing written


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="GPU present")
def test_without_a_gpu_the_python_wrapper_raises_a_status():
    with pytest.raises(sicp.SicpError) as e:
        sicp.bootstrap_batch([])
    assert e.value.status == sicp.ERR_INVALID_ARGUMENT
    with pytest.raises(sicp.SicpError) as e:
        sicp.Engine(0)
    assert e.value.status == sicp.ERR_NO_DEVICE
