"""The axpby entry points (y = alpha * A x + beta * y) are exported, declared
as the header says, and refuse a NULL plan with SPMV_ERROR_INVALID_VALUE and a
spmv_last_error text before a device is opened (no GPU needed).  The refusals
that need a plan's n and m: tests/test_gpu_axpby.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import singlespmv_amd as sp

INVALID = 1
NAMES = ("spmv_execute_axpby", "spmv_time_axpby", "spmv_axpby_path")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last():
    return sp.lib().spmv_last_error().decode()


def _header():
    return open(os.path.join(ROOT, "include", "spmv_hip.h")).read()


def test_symbols_exported_and_listed():
    L = sp.lib()
    for name in NAMES:
        assert getattr(L, name, None) is not None, f"{name} is not exported by libspmv_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert set(NAMES) <= set(sp.EXPORTS)
    for name in ("execute_axpby", "time_axpby", "axpby_path"):
        assert callable(getattr(sp.Plan, name))


def test_header_prototypes_and_version():
    hdr = _header()
    protos = {
        "spmv_execute_axpby": r"int spmv_execute_axpby\(spmv_plan_t plan, double alpha, const double \*x, double beta, "
                              r"double \*y, uint32_t flags\);",
        "spmv_time_axpby": r"int spmv_time_axpby\(spmv_plan_t plan, double alpha, const double \*x_dev, double beta, "
                           r"double \*y_dev, int32_t iters, double \*ms\);",
        "spmv_axpby_path": r"int spmv_axpby_path\(spmv_plan_t plan, int32_t \*fused\);",
    }
    for name, pat in protos.items():
        assert re.search(pat.replace(" ", r"\s+"), hdr), f"{name}: prototype not found in spmv_hip.h"
        assert len(re.findall(rf"\b{name}\(", hdr)) == 1, f"{name} is declared more than once"
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    assert sp.API_VERSION == 3
    # the contract is written once, with what stays out of scope
    for word in ("dadd_rn(dmul_rn(alpha", "SPMV_Y_STAGED is refused", "spmv_execute_multi, HIP graphs, spmv_profile"):
        assert word in hdr, word


@pytest.mark.parametrize("alpha,beta,flags", [(1.0, 1.0, 0), (-2.5, 0.75, sp.X_DEVICE | sp.Y_DEVICE | sp.ASYNC),
                                              (2.0, -0.0, 0), (1.0, 1.0, sp.Y_STAGED), (1.0, 1.0, 0x100)])
def test_null_plan_refusals(alpha, beta, flags):
    """A NULL plan is the first refusal, whatever the scalars and flags; y is not touched."""
    L = sp.lib()
    x = np.ones(4)
    y = np.full(4, 7.0)
    assert L.spmv_execute_axpby(None, alpha, x.ctypes.data, beta, y.ctypes.data, flags) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert (y == 7.0).all()
    ms = C.c_double(-1.0)
    assert L.spmv_time_axpby(None, alpha, x.ctypes.data, beta, y.ctypes.data, 1, C.byref(ms)) == INVALID
    assert ms.value == -1.0 and (y == 7.0).all()
    fused = C.c_int32(-7)
    assert L.spmv_axpby_path(None, C.byref(fused)) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert fused.value == -7
