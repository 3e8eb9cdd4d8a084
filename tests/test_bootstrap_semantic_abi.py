"""The C ABI of the label-aware bootstrap without a GPU: the ctypes struct against the C compiler's layout of
include/sicp.h, the defaults, the exported symbols and the Python helper's ignore list."""
import ctypes
import importlib
import os
import subprocess
import tempfile
import textwrap

import pytest

sicp = importlib.import_module("semantic-icp_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sicp_default_bootstrap_label_params", "sicp_bootstrap_semantic", "sicp_bootstrap_semantic_batch",
                "sicp_bootstrap_semantic_keypoints", "sicp_bootstrap_semantic_score")


def test_label_params_layout_matches_the_header():
    code = textwrap.dedent(
        """
        #include <stddef.h>
        #include <stdio.h>
        #include "sicp.h"
        int main(void) {
          printf("%zu %zu %zu %zu %zu %d\\n", sizeof(sicp_bootstrap_label_params), offsetof(sicp_bootstrap_label_params, match_same_label),
                 offsetof(sicp_bootstrap_label_params, score_same_label), offsetof(sicp_bootstrap_label_params, n_ignore),
                 offsetof(sicp_bootstrap_label_params, ignore), SICP_BOOTSTRAP_MAX_IGNORE);
          return 0;
        }
        """
    )
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(code)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size, o_match, o_score, o_n, o_ignore, cap = map(int, subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split())
    L = sicp.SicpBootstrapLabelParams
    assert ctypes.sizeof(L) == size
    assert (L.match_same_label.offset, L.score_same_label.offset, L.n_ignore.offset, L.ignore.offset) == (o_match, o_score, o_n, o_ignore)
    assert sicp.BOOTSTRAP_MAX_IGNORE == cap == 64


def test_entry_points_are_exported_and_the_defaults_are_the_documented_ones():
    lib = ctypes.CDLL(sicp.build())
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    lp = sicp.default_bootstrap_label_params()
    assert (lp.match_same_label, lp.score_same_label, lp.n_ignore, lp.reserved_) == (1, 1, 0, 0)
    assert list(lp.ignore) == [0] * 64
    assert sicp.lib().sicp_default_bootstrap_label_params(None) == sicp.ERR_INVALID_ARGUMENT
    assert sicp.version().split()[1].startswith("0.6")


def test_the_python_helper_fills_the_ignore_list():
    lp = sicp.default_bootstrap_label_params(ignore=(7, 0xFFFFFFFF, 0), score_same_label=0)
    assert (lp.n_ignore, list(lp.ignore[:3]), lp.score_same_label, lp.match_same_label) == (3, [7, 0xFFFFFFFF, 0], 0, 1)
    assert sicp.default_bootstrap_label_params(ignore=range(64)).n_ignore == 64
    with pytest.raises(ValueError):
        sicp.default_bootstrap_label_params(ignore=range(65))
    with pytest.raises(AttributeError):
        sicp.default_bootstrap_label_params(no_such_field=1)
