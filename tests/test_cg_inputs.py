"""tests/cg_inputs.py on the CPU: every case is symmetric with a dominant
positive diagonal, the NumPy reference of spmv_cg_solve's iteration converges
within 1000 iterations to a true relative residual <= 2 * rtol (the condition
tests/test_gpu_cg.py inherits), and its own rounding error after five
iterations (d_ref, float64 against longdouble) is recorded."""
import numpy as np
import pytest

import cg_inputs as ci

CASES = [pytest.param(name, use_dinv, id=f"{name}-{'dinv' if use_dinv else 'plain'}")
         for name in ci.NAMES for use_dinv in (False, True)]


@pytest.mark.parametrize("name", ci.NAMES)
def test_case_shape_and_symmetry(name):
    c = ci.case(name)
    m, rp, col, val = c["m"], c["rp"], c["col"], c["val"]
    assert m % 64 != 0 and len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(col) == len(val)
    for r in range(0, m, max(1, m // 97)):  # columns strictly ascending within a row
        assert (np.diff(col[rp[r]:rp[r + 1]]) > 0).all()
    assert ci.is_symmetric(c)
    off = np.zeros(m)
    np.add.at(off, c["row"], np.abs(val))
    off -= np.abs(c["diag"])
    assert (c["diag"] > off).all(), "the diagonal does not dominate"
    assert np.array_equal(ci.bits(c["dinv"]), ci.bits(1.0 / c["diag"]))
    assert not c["b"].flags.writeable and not c["val"].flags.writeable


def test_case_structure():
    n = {name: np.diff(ci.case(name)["rp"]) for name in ci.NAMES}
    assert [ci.case(name)["m"] for name in ci.NAMES] == [3001, 4099, 3233, 5003, 1, 65, 130]
    assert 8.5 < n["rand8"].mean() < 9.1  # 8 off-diagonals and the diagonal
    assert 2900 < n["skew"].max() < 3100 and n["skew"].argmax() == 0 and 4.5 < np.median(n["skew"]) <= 6
    assert n["lap2d"].max() == 5 and n["lap2d"].min() == 3 and n["lap1d"].max() == 3 and n["tiny65"].max() == 3


def test_an_asymmetric_matrix_is_seen():
    c = dict(ci.case("tiny65"))
    val = c["val"].copy()
    val[1] += 1.0  # A[0, 1] alone
    c["val"] = val
    assert not ci.is_symmetric(c)


@pytest.mark.parametrize("name,use_dinv", CASES)
def test_reference_converges(name, use_dinv):
    ref = ci.reference(name, use_dinv)
    print(f"cg-ref {name} dinv={int(use_dinv)} ref_iters={ref['ref_iters']} true_relres={ref['true_relres']:.3e} "
          f"recurred={ref['recurred_relres']:.3e} d_ref={ref['d_ref']:.3e}")
    assert ref["status"] == ci.CONVERGED and 0 < ref["ref_iters"] <= 1000
    assert ref["recurred_relres"] <= ci.RTOL
    assert ref["true_relres"] <= 2 * ci.RTOL
    if ci.case(name)["m"] > ci.FIXED:  # (tiny1 is solved by its first step)
        assert ref["status5"] == ci.MAX_ITERS
    # rounding error, not another iterate: 1e-16 .. 1e-15.  skew without dinv is
    # the exception (2.6e-7): the hub's diagonal is an eigenvalue 600 times the
    # others', its Ritz value converges in two steps, and from there the
    # rounding errors of the recurrence grow with every step in any precision
    assert 0 <= ref["d_ref"] < (1e-5 if (name, use_dinv) == ("skew", False) else 1e-14)


def test_reference_edges():
    c = ci.case("tiny65")
    zero = np.zeros(c["m"])
    x, info = ci.ref_cg(c, zero, zero, None, ci.RTOL, 10)
    assert info["status"] == ci.CONVERGED and info["iterations"] == 0 and not x.any()
    x, info = ci.ref_cg(c, c["b"], c["x0"], None, ci.RTOL, 0)
    assert info["status"] == ci.MAX_ITERS and info["iterations"] == 0 and np.array_equal(x, c["x0"])
    x, info = ci.ref_cg(c, c["b"], c["x0"], None, ci.RTOL, 10, scale=-1.0)
    assert info["status"] == ci.BREAKDOWN and info["iterations"] == 0 and np.array_equal(x, c["x0"]) and info["pq"] < 0
    b = c["b"].copy()
    b[7] = np.nan
    _, info = ci.ref_cg(c, b, c["x0"], None, ci.RTOL, 10)
    assert info["status"] == ci.BREAKDOWN and info["iterations"] == 0
    # 2 A x = b: half the solution of A x = b
    x1, _ = ci.ref_cg(c, c["b"], zero, None, ci.RTOL, 100)
    x2, _ = ci.ref_cg(c, c["b"], zero, None, ci.RTOL, 100, scale=2.0)
    assert np.array_equal(ci.bits(x2), ci.bits(0.5 * x1))
