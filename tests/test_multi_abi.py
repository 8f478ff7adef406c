"""The multi-vector entry points refuse bad arguments with
SPMV_ERROR_INVALID_VALUE and a spmv_last_error text before a device is opened
(no GPU needed: the checks that need no plan come first, so a NULL plan with
otherwise valid arguments is the last refusal).  The NULL X / Y refusal needs
a plan's n and m: tests/test_gpu_multi.py."""
import ctypes as C

import numpy as np
import pytest

import singlespmv_amd as sp

INVALID = 1
BAD = [  # (k, ldx, ldy, flags, text)
    (2, 2, 2, sp.X_STAGED, "STAGED"),
    (2, 2, 2, sp.Y_STAGED, "STAGED"),
    (2, 2, 2, sp.X_DEVICE | sp.Y_DEVICE | sp.Y_STAGED, "STAGED"),
    (0, 2, 2, 0, "k outside"),
    (-1, 2, 2, 0, "k outside"),
    (33, 40, 40, 0, "k outside"),
    (4, 3, 4, 0, "ldx < k"),
    (4, 4, 3, 0, "ldy < k"),
    (4, -4, 4, 0, "ldx < k"),
    (1, 0, 1, 0, "ldx < k"),
    (2, 2, 2, 0, "plan is NULL"),
    (32, 32, 32, sp.X_DEVICE | sp.Y_DEVICE | sp.ASYNC, "plan is NULL"),
]


def _last():
    return sp.lib().spmv_last_error().decode()


@pytest.mark.parametrize("k,ldx,ldy,flags,text", BAD)
def test_multi_refusals_without_device(k, ldx, ldy, flags, text):
    L = sp.lib()
    X = np.zeros((4, 40))
    Y = np.zeros((4, 40))
    assert L.spmv_execute_multi(None, k, X.ctypes.data, ldx, Y.ctypes.data, ldy, flags) == INVALID
    assert text in _last(), _last()
    assert not Y.any()
    w = (C.c_int32 * 32)()
    nb = C.c_int32(-7)
    assert L.spmv_multi_path(None, k, X.ctypes.data, ldx, Y.ctypes.data, ldy, flags, w, 32, C.byref(nb)) == INVALID
    assert text in _last(), _last()
    assert nb.value == -7
    if not flags & (sp.X_STAGED | sp.Y_STAGED):
        ms = C.c_double(-1.0)
        assert L.spmv_time_multi(None, k, X.ctypes.data, ldx, Y.ctypes.data, ldy, 1, C.byref(ms)) == INVALID
        assert text in _last(), _last()
        assert ms.value == -1.0


def test_multi_max_matches_header():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "spmv_hip.h")).read()
    assert int(re.search(r"#define SPMV_MULTI_MAX (\d+)", hdr).group(1)) == sp.MULTI_MAX == 32
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    assert {"spmv_execute_multi", "spmv_time_multi", "spmv_multi_path"} <= set(sp.EXPORTS)
