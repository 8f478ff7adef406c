"""The solver's entry points (spmv_cg_solve, spmv_cg_path) are exported,
declared as the header says, mirrored in Python, and refuse a NULL plan with
SPMV_ERROR_INVALID_VALUE and a spmv_last_error text before a device is opened
(no GPU needed).  The refusals that need a plan: tests/test_gpu_cg.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import singlespmv_amd as sp

INVALID = 1
NAMES = ("spmv_cg_solve", "spmv_cg_path")
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
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert set(NAMES) <= set(sp.EXPORTS)
    assert "cg_graph_release" not in " ".join(dynamic), "the solver's helper is a dynamic symbol"
    for name in ("cg", "cg_path"):
        assert callable(getattr(sp.Plan, name))


def test_header_prototypes_flags_and_struct():
    hdr = _header()
    protos = {
        "spmv_cg_solve": r"int spmv_cg_solve\(spmv_plan_t plan, const double \*b, double \*x, const double \*dinv, "
                         r"double rtol, int32_t max_iters, int32_t check_every, uint32_t flags, "
                         r"spmv_cg_info_t \*info\);",
        "spmv_cg_path": r"int spmv_cg_path\(spmv_plan_t plan, int32_t \*launches_per_iteration\);",
    }
    for name, pat in protos.items():
        assert re.search(pat.replace(" ", r"\s+"), hdr), f"{name}: prototype not found in spmv_hip.h"
        assert len(re.findall(rf"\b{name}\(", hdr)) == 1, f"{name} is declared more than once"
    # only functions, flags and a struct of its own are new: the version stays 3
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    flags = {name: int(v, 16) for name, v in re.findall(r"#define (SPMV_[A-Z_]+)\s+(0x[0-9a-f]+)u", hdr)}
    assert flags["SPMV_CG_DEVICE"] == 0x200 == sp.CG_DEVICE and flags["SPMV_CG_GRAPH"] == 0x400 == sp.CG_GRAPH
    call_flags = [flags[k] for k in ("SPMV_X_DEVICE", "SPMV_Y_DEVICE", "SPMV_ASYNC", "SPMV_X_STAGED", "SPMV_Y_STAGED",
                                     "SPMV_CSR_DEVICE", "SPMV_VAL_DEVICE", "SPMV_W_DEVICE", "SPMV_DOTS_DEVICE",
                                     "SPMV_CG_DEVICE", "SPMV_CG_GRAPH")]
    assert len(set(call_flags)) == 11 and all(f & (f - 1) == 0 for f in call_flags)
    assert re.search(r"enum \{ SPMV_CG_CONVERGED = 0, SPMV_CG_MAX_ITERS = 1, SPMV_CG_BREAKDOWN = 2 \};", hdr)
    assert sp.CG_STATUS == {0: "converged", 1: "max_iters", 2: "breakdown"}
    # spmv_cg_info_t and its mirror: two int32, four doubles, no padding
    body = re.search(r"typedef struct spmv_cg_info \{(.*?)\} spmv_cg_info_t;", hdr, re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+([a-z, ]+);", body)
    names = [(t, n.strip()) for t, ns in fields for n in ns.split(",")]
    assert names == [("int32_t", "status"), ("int32_t", "iterations"), ("double", "rr"), ("double", "bb"),
                     ("double", "rz"), ("double", "pq")]
    assert [n for n, _ in sp.CgInfo._fields_] == [n for _, n in names] and C.sizeof(sp.CgInfo) == 40
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)  # comment lines joined
    for word in ("never an FMA", "rr <= rtol * rtol * bb", "tested before the first iteration too",
                 "no floating-point atomic takes part, except the y-atomics COO plans already have",
                 "not of check_every, of SPMV_CG_GRAPH", "max_iters < 0; check_every < 1; rtol < 0 or NaN",
                 "Not covered: other Krylov methods, non-symmetric A"):
        assert word in flat, word


@pytest.mark.parametrize("flags", [0, sp.CG_DEVICE, sp.CG_GRAPH, sp.CG_DEVICE | sp.CG_GRAPH, sp.X_DEVICE, 0x800])
def test_null_plan_refusals(flags):
    """A NULL plan is the first refusal, whatever the flags; x and info are not touched."""
    L = sp.lib()
    b = np.ones(4)
    x = np.full(4, 7.0)
    info = sp.CgInfo(-5, -6, -1.0, -2.0, -3.0, -4.0)
    assert L.spmv_cg_solve(None, b.ctypes.data, x.ctypes.data, None, 1e-8, 10, 1, flags, C.byref(info)) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert L.spmv_cg_solve(None, None, None, None, -1.0, -1, 0, flags, None) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert (x == 7.0).all() and (b == 1.0).all()
    assert (info.status, info.iterations, info.rr, info.bb, info.rz, info.pq) == (-5, -6, -1.0, -2.0, -3.0, -4.0)
    n = C.c_int32(-7)
    assert L.spmv_cg_path(None, C.byref(n)) == INVALID
    assert "plan is NULL" in _last(), _last()
    assert n.value == -7


def test_python_refuses_before_the_library():
    """Plan.cg checks its vectors through _check_vec (no plan handle is
    needed to get there: the checks come first)."""
    class Fake(sp.Plan):
        def __init__(self):
            self.m = self.n = 4
            self.device = 0
            self._h = None

        def destroy(self):
            pass

    plan = Fake()
    good = np.ones(4)
    for b, x, dinv, word in ((np.ones(3), good.copy(), None, "b holds 3"),
                             (good, np.ones(4, np.float32), None, "x must be float64"),
                             (good, good.copy(), np.ones(8)[::2], "dinv must be C-contiguous"),
                             (good, [1.0] * 4, None, "x must be a numpy array"),
                             (None, good.copy(), None, "b must be a numpy array")):
        with pytest.raises(ValueError, match=word):
            plan.cg(b, x, dinv)
    ro = good.copy()
    ro.setflags(write=False)
    with pytest.raises(ValueError, match="x is read-only"):
        plan.cg(good, ro)
