"""spmv_csr_transpose (the host transposition, the reference of the device
pipeline) against numpy's stable argsort, byte for byte; its refusals; and the
five transpose entry points' export and declaration.  No GPU needed; the
device side is tests/test_gpu_transpose.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import signed_inputs as si
import singlespmv_amd as sp
import transpose_inputs as ti

INVALID = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spmv_csr_transpose", "spmv_csr_transpose_device", "spmv_plan_create_csr_transposed",
         "spmv_plan_create_csr_device_transposed", "spmv_plan_is_transposed")


def _inputs():
    for name in si.STRUCTURES:
        yield pytest.param(("structure", name), id=f"{name}")
        yield pytest.param(("twin", name), id=f"{name}-twin")
    for name in ti.edges():
        yield pytest.param(("edge", name), id=name)


def _load(key):
    kind, name = key
    if kind == "edge":
        return ti.edges()[name]
    if kind == "twin":
        t = ti.twin(name, "spread")
        return t["m"], t["n"], t["rp"], t["col"], t["val"]
    c = si.case(name, "spread")
    return c["m"], c["n"], c["rp"], c["col"], c["val"]


@pytest.mark.parametrize("key", _inputs())
def test_host_transposition_equals_stable_argsort(key):
    m, n, rp, col, val = _load(key)
    want = ti.np_transpose(m, n, rp, col, val)
    got = sp.csr_transpose(m, n, rp, col, val, perm=True)
    ti.assert_same_csr(got, want, str(key))
    t_rp, t_col, t_val, perm = got
    # perm is a permutation, and the outputs are the inputs seen through it
    assert np.array_equal(np.sort(perm), np.arange(len(col)))
    row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    assert np.array_equal(t_col, row[perm]) and np.array_equal(ti.bits(t_val), ti.bits(val)[perm])
    assert np.array_equal(np.asarray(col)[perm], np.repeat(np.arange(n, dtype=np.int32), np.diff(t_rp)))
    # pattern-only and perm = NULL calls give the same arrays
    ti.assert_same_csr(sp.csr_transpose(m, n, rp, col), (want[0], want[1], None), f"{key} pattern only")
    ti.assert_same_csr(sp.csr_transpose(m, n, rp, col, val), want[:3], f"{key} without perm")
    ti.assert_same_csr(sp.csr_transpose(m, n, rp, col, None, perm=True), (want[0], want[1], None, want[3]),
                       f"{key} pattern and perm")


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_transposing_twice_returns_the_case(name):
    c = si.case(name, "cancel")
    t = sp.csr_transpose(c["m"], c["n"], c["rp"], c["col"], c["val"])
    back = sp.csr_transpose(c["n"], c["m"], *t)
    ti.assert_same_csr(back, (c["rp"], c["col"], np.ascontiguousarray(c["val"])), name)


@pytest.mark.parametrize("name", ["short", "rect513x40", "rect7x1000", "banded"])
def test_shuffling_inside_rows_changes_nothing(name):
    """Duplicate-free rows: the order of a row's entries does not reach A^T."""
    c = si.case(name, "spread")
    rp, col, val = c["rp"], c["col"], c["val"]
    rng = np.random.default_rng(5)
    row = np.repeat(np.arange(c["m"]), np.diff(rp))
    assert len(np.unique(row.astype(np.int64) * c["n"] + col)) == len(col), "the structure has duplicate entries"
    order = np.argsort(row + rng.random(len(col)))  # shuffled within each row
    assert not np.array_equal(order, np.arange(len(col)))
    want = sp.csr_transpose(c["m"], c["n"], rp, col, val)
    got = sp.csr_transpose(c["m"], c["n"], rp, col[order], val[order])
    ti.assert_same_csr(got, want, name)


@pytest.mark.parametrize("name", list(ti.refused()))
def test_refusals_leave_the_outputs_untouched(name):
    m, n, nnz, rp, col = ti.refused()[name]
    val = np.arange(1.0, nnz + 1)
    t_rp = np.full(n + 1, -77, np.int64)
    t_col = np.full(nnz, -77, np.int32)
    t_val = np.full(nnz, -77.0)
    perm = np.full(nnz, -77, np.int64)
    st = sp.lib().spmv_csr_transpose(m, n, nnz, None if rp is None else rp.ctypes.data, col.ctypes.data,
                                     val.ctypes.data, t_rp.ctypes.data, t_col.ctypes.data, t_val.ctypes.data,
                                     perm.ctypes.data)
    assert st == INVALID, (name, st)
    assert sp.lib().spmv_last_error().decode(), "no error text"
    assert (t_rp == -77).all() and (t_col == -77).all() and (t_val == -77.0).all() and (perm == -77).all()


def test_val_without_t_val_is_refused():
    rp = np.array([0, 1], np.int64)
    col = np.zeros(1, np.int32)
    val = np.ones(1)
    t_rp = np.full(2, -77, np.int64)
    t_col = np.full(1, -77, np.int32)
    st = sp.lib().spmv_csr_transpose(1, 1, 1, rp.ctypes.data, col.ctypes.data, val.ctypes.data, t_rp.ctypes.data,
                                     t_col.ctypes.data, None, None)
    assert st == INVALID and (t_rp == -77).all() and (t_col == -77).all()


def test_symbols_exported_and_listed():
    L = sp.lib()
    for name in NAMES:
        assert getattr(L, name, None) is not None, f"{name} is not exported by libspmv_hip.so"
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    assert set(NAMES) <= set(sp.EXPORTS)
    assert callable(sp.csr_transpose) and isinstance(sp.Plan.transposed, property)


def test_header_prototypes_and_version():
    hdr = open(os.path.join(ROOT, "include", "spmv_hip.h")).read()
    protos = {
        "spmv_csr_transpose":
            r"int spmv_csr_transpose\(int64_t m, int64_t n, int64_t nnz, const int64_t \*row_ptr, "
            r"const int32_t \*col_idx, const double \*val, int64_t \*t_row_ptr, int32_t \*t_col_idx, "
            r"double \*t_val, int64_t \*perm\);",
        "spmv_csr_transpose_device":
            r"int spmv_csr_transpose_device\(int32_t device, int64_t m, int64_t n, int64_t nnz, "
            r"const int64_t \*d_row_ptr, const int32_t \*d_col_idx, const double \*d_val, int64_t \*d_t_row_ptr, "
            r"int32_t \*d_t_col_idx, double \*d_t_val, int64_t \*d_perm\);",
        "spmv_plan_create_csr_transposed":
            r"int spmv_plan_create_csr_transposed\(int64_t m, int64_t n, int64_t nnz, const int64_t \*row_ptr, "
            r"const int32_t \*col_idx, const double \*val, const spmv_options_t \*opt, spmv_plan_t \*plan\);",
        "spmv_plan_create_csr_device_transposed":
            r"int spmv_plan_create_csr_device_transposed\(int64_t m, int64_t n, int64_t nnz, "
            r"const int64_t \*d_row_ptr, const int32_t \*d_col_idx, const double \*d_val, "
            r"const spmv_options_t \*opt, spmv_plan_t \*plan\);",
        "spmv_plan_is_transposed": r"int spmv_plan_is_transposed\(spmv_plan_t plan, int32_t \*transposed\);",
    }
    for name, pat in protos.items():
        assert re.search(pat.replace(" ", r"\s+"), hdr), f"{name}: prototype not found in spmv_hip.h"
        assert len(re.findall(rf"\b{name}\(", hdr)) == 1, f"{name} is declared more than once"
    assert int(re.search(r"#define SPMV_HIP_API_VERSION (\d+)", hdr).group(1)) == 3 == sp.lib().spmv_api_version()
    assert sp.API_VERSION == 3


def test_null_plan_is_refused():
    t = C.c_int32(-7)
    assert sp.lib().spmv_plan_is_transposed(None, C.byref(t)) == INVALID and t.value == -7
