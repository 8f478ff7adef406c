"""The value-refresh entry points (spmv_plan_update_prepare,
spmv_plan_update_values) refuse bad arguments with SPMV_ERROR_INVALID_VALUE and
a spmv_last_error text before a device is opened (no GPU needed: the checks
that need no plan come first, so a NULL plan with valid flags is the refusal
that follows the flag check).  The refusals that need a plan's nnz (NULL
col_idx / val, SPMV_ASYNC without SPMV_VAL_DEVICE, "not prepared") are in
tests/test_gpu_update_values.py."""
import os
import re

import numpy as np
import pytest

import singlespmv_amd as sp

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last():
    return sp.lib().spmv_last_error().decode()


PREPARE_BAD = [  # (flags, text)
    (sp.X_DEVICE, "flag bits"),
    (sp.ASYNC, "flag bits"),
    (sp.VAL_DEVICE, "flag bits"),
    (sp.CSR_DEVICE | sp.VAL_DEVICE, "flag bits"),
    (0x80, "flag bits"),
    (0x80000000, "flag bits"),
    (0, "plan is NULL"),
    (sp.CSR_DEVICE, "plan is NULL"),
]

VALUES_BAD = [  # (flags, text)
    (sp.X_DEVICE, "flag bits"),
    (sp.Y_DEVICE | sp.VAL_DEVICE, "flag bits"),
    (sp.CSR_DEVICE, "flag bits"),
    (sp.X_STAGED | sp.ASYNC, "flag bits"),
    (0x80, "flag bits"),
    (0, "plan is NULL"),
    (sp.VAL_DEVICE, "plan is NULL"),
    (sp.VAL_DEVICE | sp.ASYNC, "plan is NULL"),
    (sp.ASYNC, "plan is NULL"),  # the ASYNC-without-device check needs no plan but comes after it
]


@pytest.mark.parametrize("flags,text", PREPARE_BAD)
def test_prepare_refusals_without_device(flags, text):
    rp = np.array([0, 1, 2], np.int64)
    col = np.array([0, 1], np.int32)
    assert sp.lib().spmv_plan_update_prepare(None, rp.ctypes.data, col.ctypes.data, flags) == INVALID
    assert text in _last(), _last()
    assert rp.tolist() == [0, 1, 2] and col.tolist() == [0, 1]


@pytest.mark.parametrize("flags,text", VALUES_BAD)
def test_values_refusals_without_device(flags, text):
    val = np.array([1.0, 2.0])
    assert sp.lib().spmv_plan_update_values(None, val.ctypes.data, flags) == INVALID
    assert text in _last(), _last()
    assert val.tolist() == [1.0, 2.0]


def test_flag_texts_name_their_function():
    L = sp.lib()
    assert L.spmv_plan_update_prepare(None, None, None, 0x1) == INVALID
    assert "spmv_plan_update_prepare" in _last() and "SPMV_CSR_DEVICE" in _last()
    assert L.spmv_plan_update_values(None, None, 0x1) == INVALID
    assert "spmv_plan_update_values" in _last() and "SPMV_VAL_DEVICE" in _last()


def test_update_symbols_header_and_version():
    hdr = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    assert {"spmv_plan_update_prepare", "spmv_plan_update_values"} <= set(sp.EXPORTS)
    assert re.search(r"int\s+spmv_plan_update_prepare\s*\(\s*spmv_plan_t\s+plan,\s*const int64_t \*row_ptr,"
                     r"\s*const int32_t \*col_idx,\s*uint32_t flags\)", hdr)
    assert re.search(r"int\s+spmv_plan_update_values\s*\(\s*spmv_plan_t\s+plan,\s*const double \*val,"
                     r"\s*uint32_t flags\)", hdr)
    assert int(re.search(r"#define SPMV_CSR_DEVICE (0x[0-9a-f]+)u", hdr).group(1), 16) == sp.CSR_DEVICE == 0x20
    assert int(re.search(r"#define SPMV_VAL_DEVICE (0x[0-9a-f]+)u", hdr).group(1), 16) == sp.VAL_DEVICE == 0x40
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    for name in ("spmv_plan_update_prepare", "spmv_plan_update_values"):
        assert hasattr(sp.lib(), name)
    assert callable(sp.Plan.prepare_update) and callable(sp.Plan.update_values)
