"""The dot entry points (y = A x with w . y and y . y from the same pass) are
exported, declared as the header says, and refuse a NULL plan with
SPMV_ERROR_INVALID_VALUE and a spmv_last_error text before a device is opened
(no GPU needed).  The refusals that need a plan's n and m:
tests/test_gpu_dot.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import singlespmv_amd as sp

INVALID = 1
NAMES = ("spmv_execute_dot", "spmv_time_dot", "spmv_dot_path")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last():
    return sp.lib().spmv_last_error().decode()


def _header():
    return open(os.path.join(ROOT, "include", "spmv_hip.h")).read()


def test_symbols_exported_and_listed():
    L = sp.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", sp.LIB_PATH], text=True)
    dynamic = {ln.split()[-1] for ln in out.splitlines() if ln.split()}
    for name in NAMES:
        assert name in dynamic, f"{name} is not a dynamic symbol of libspmv_hip.so"
        assert getattr(L, name, None) is not None, f"{name} is not exported by libspmv_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert set(NAMES) <= set(sp.EXPORTS)
    for name in ("execute_dot", "time_dot", "dot_path"):
        assert callable(getattr(sp.Plan, name))


def test_header_prototypes_flags_and_version():
    hdr = _header()
    protos = {
        "spmv_execute_dot": r"int spmv_execute_dot\(spmv_plan_t plan, const double \*x, double \*y, "
                            r"const double \*w, double \*dots, uint32_t flags\);",
        "spmv_time_dot": r"int spmv_time_dot\(spmv_plan_t plan, const double \*x_dev, double \*y_dev, "
                         r"const double \*w_dev, double \*dots_dev, int32_t iters, double \*ms\);",
        "spmv_dot_path": r"int spmv_dot_path\(spmv_plan_t plan, int32_t \*fused\);",
    }
    for name, pat in protos.items():
        assert re.search(pat.replace(" ", r"\s+"), hdr), f"{name}: prototype not found in spmv_hip.h"
        assert len(re.findall(rf"\b{name}\(", hdr)) == 1, f"{name} is declared more than once"
    # only functions and flags are new: no struct change, the version stays 3
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    assert sp.API_VERSION == 3
    flags = {name: int(v, 16) for name, v in re.findall(r"#define (SPMV_[A-Z_]+)\s+(0x[0-9a-f]+)u", hdr)}
    assert flags["SPMV_W_DEVICE"] == 0x80 == sp.W_DEVICE and flags["SPMV_DOTS_DEVICE"] == 0x100 == sp.DOTS_DEVICE
    execute_flags = [flags[k] for k in ("SPMV_X_DEVICE", "SPMV_Y_DEVICE", "SPMV_ASYNC", "SPMV_X_STAGED",
                                        "SPMV_Y_STAGED", "SPMV_W_DEVICE", "SPMV_DOTS_DEVICE")]
    assert len(set(execute_flags)) == 7 and all(f & (f - 1) == 0 for f in execute_flags)
    # the contract is written once, with what stays out of scope
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)  # comment lines joined
    for word in ("dmul_rn(w[r], y[r])", "no floating-point atomic takes part", "(m + 8) * 2^-53",
                 "unknown flag bits; SPMV_Y_STAGED (y always travels back", "dropped by a select, never by a zero weight",
                 "none for spmv_execute_multi, HIP graphs, spmv_profile, spmv_dist_*"):
        assert word in flat, word


@pytest.mark.parametrize("flags", [0, sp.X_DEVICE | sp.Y_DEVICE | sp.W_DEVICE | sp.DOTS_DEVICE | sp.ASYNC, sp.Y_STAGED,
                                   0x200, sp.ASYNC])
def test_null_plan_refusals(flags):
    """A NULL plan is the first refusal, whatever the flags; y and dots are not touched."""
    L = sp.lib()
    x = np.ones(4)
    w = np.ones(4)
    y = np.full(4, 7.0)
    dots = np.full(2, -3.0)
    assert L.spmv_execute_dot(None, x.ctypes.data, y.ctypes.data, w.ctypes.data, dots.ctypes.data, flags) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert L.spmv_execute_dot(None, x.ctypes.data, y.ctypes.data, None, None, flags) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert (y == 7.0).all() and (dots == -3.0).all()
    ms = C.c_double(-1.0)
    assert L.spmv_time_dot(None, x.ctypes.data, y.ctypes.data, w.ctypes.data, dots.ctypes.data, 1, C.byref(ms)) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert ms.value == -1.0 and (y == 7.0).all() and (dots == -3.0).all()
    fused = C.c_int32(-7)
    assert L.spmv_dot_path(None, C.byref(fused)) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert fused.value == -7
