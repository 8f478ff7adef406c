"""Every format and kernel path on signed data: wide dynamic range
(`spread`) and rows that cancel to rounding noise (`cancel`), checked per row
against an extended-precision reference with a bound derived from the row
length (tests/signed_inputs.py: (len + 8) 2^-53 sum |a x|), and bit for bit
against the sequential sum where the layout is sequential.
Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest

import signed_inputs as si
import singlespmv_amd as sp
from test_gpu_parity import _device_csr, assert_bin_rows

pytestmark = pytest.mark.gpu

CONFIGS = (
    [(f"csr-lanes{k}", "csr", {"csr_lanes": k}) for k in (0, 1, 2, 4, 8, 16, 32, 64)]
    + [(f"ss-sigma{k}", "ss", {"ss_sigma": k}) for k in (4, 16, 32, 64)]
    + [("ss", "ss", {}), ("ell", "ell", {}), ("hyb", "hyb", {}), ("hyb-width4", "hyb", {"ell_width": 4}),
       ("jds", "jds", {}), ("jds-width9000", "jds", {"ell_width": 9000}), ("coo", "coo", {}),
       ("css", "css", {}), ("css-shift8", "css", {"css_slab_shift": 8}),
       ("bin", "bin", {}), ("bin-long40", "bin", {"bin_long_len": 40}), ("bin-nolong", "bin", {"bin_long_len": -1}),
       ("bin-order1", "bin", {"bin_product_order": 1}), ("bin-order2", "bin", {"bin_product_order": 2}),
       ("bin-strip1000", "bin", {"bin_strip_cols": 1000}), ("dia", "dia", {}), ("auto", "auto", {})])

CASES = [pytest.param(name, family, fmt, kw, id=f"{name}-{family}-{cid}")
         for name in si.STRUCTURES for family in sorted(si.FAMILIES) for cid, fmt, kw in CONFIGS
         if fmt != "dia" or name == "banded"]


def _build(c, fmt, kw):
    try:
        return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)
    except sp.SpmvError as e:
        if "not supported" in str(e):
            pytest.skip(f"the builder refuses this configuration: {e}")
        raise


def _execute_twice(plan, c):
    """y over a NaN-filled and over a -1.2345e300-filled buffer (a kernel
    computing 0 * y_old + acc passes the second, not the first)."""
    ya = np.full(c["m"], np.nan)
    plan.execute(c["x"], ya)
    yb = np.full(c["m"], -1.2345e300)
    plan.execute(c["x"], yb)
    return ya, yb


def _check_y(plan, c, ya, yb, what):
    """The checks every plan's y must pass; returns the largest err/row_tol."""
    rp, col, val, x = c["rp"], c["col"], c["val"], c["x"]
    info = plan.info()
    worst = si.assert_rows(ya, rp, col, val, x, what, ref=c["ref"])
    if info["format"] == "coo":
        # f64 atomics: a row split across 128-entry units may round differently
        # run to run; a row inside one unit gets exactly one atomic
        worst = max(worst, si.assert_rows(yb, rp, col, val, x, what + " (2nd execute)", ref=c["ref"]))
        inside = (rp[:-1] // 128 == (rp[1:] - 1) // 128) & (np.diff(rp) > 0)
        assert np.array_equal(ya[inside], yb[inside]), f"{what}: rows inside one unit differ run to run"
        assert (ya[np.diff(rp) == 0] == 0).all() and (yb[np.diff(rp) == 0] == 0).all()
    else:
        assert np.array_equal(ya, yb), f"{what}: y depends on what y held before"
    assert sp.verify_result(sp.SpMat(c["m"], c["n"], c["row"], col, val), x, ya), f"{what}: VerifyResult (1e-6) failed"
    if info["format"] == "bin":
        assert_bin_rows(plan, ya, rp, col, val, x, what=what)
    if si.plan_is_sequential(info):  # rows ascend in column order, DIA runs without duplicates
        assert np.array_equal(ya, c["y_oracle"]), f"{what}: {info['format']} is sequential, must be bit-exact"
    return worst


@pytest.mark.parametrize("name,family,fmt,kw", CASES)
def test_signed_parity(name, family, fmt, kw, request):
    c = si.case(name, family)
    lens = np.diff(c["rp"])
    plan = _build(c, fmt, kw)
    info = plan.info()
    what = request.node.callspec.id
    # the configuration reaches the path it is here for
    if fmt != "auto":
        assert info["format"] == fmt, info["format"]
    if fmt == "csr":
        lanes = kw["csr_lanes"]
        if lanes == 0 and name in ("staircase", "powerlaw"):
            assert info["kernel"] == "csr_adaptive_kernel", info["kernel"]
        elif name == "banded":
            assert info["kernel"].startswith("csr_slabx_kernel"), info["kernel"]
        elif name == "uniform16":
            assert info["kernel"].startswith("csr_slab2_kernel"), info["kernel"]
        if lanes:
            assert info["csr_lanes"] == lanes
    if name == "staircase":
        if fmt == "hyb":
            assert info["n_kernels"] == 2 and info["overflow_nnz"] > 0
        if fmt == "jds" and not kw:
            assert info["overflow_nnz"] > 0
        if fmt == "css":  # rows beyond 64 entries are split at this size; the 9000-entry row into 141 pieces
            assert info["css_split_rows"] > 0
    if kw.get("ell_width") == 9000:
        assert info["overflow_nnz"] == 0 and si.plan_is_sequential(info)
    if kw.get("bin_long_len") == 40 and (lens >= 40).any():
        assert info["bin_long_rows"] > 0 and info["bin_long_len"] == 40
    if kw.get("bin_long_len") == -1:  # no run path: plan info reports threshold 0 (none)
        assert info["bin_long_len"] == 0 and info["bin_long_rows"] == 0 and si.plan_is_sequential(info)
    if fmt == "dia":
        assert si.plan_is_sequential(info)
    ya, yb = _execute_twice(plan, c)
    worst = _check_y(plan, c, ya, yb, what)
    print(f"signed-parity {what} format={info['format']} err/row_tol={worst:.3f}")
    plan.destroy()


@pytest.mark.parametrize("fmt", ["csr", "ss", "css", "bin", "coo"])
@pytest.mark.parametrize("family", ["cancel", "spread"])
@pytest.mark.parametrize("name", ["powerlaw", "banded"])
def test_signed_device_build(name, family, fmt):
    """Plan.from_device_csr on signed values (`cancel`; `spread` adds tiny
    and huge magnitudes): the y of the host build, bit for bit (COO, whose
    atomics are unordered: within row_tol)."""
    c = si.case(name, family)
    what = f"{name}-{family}-{fmt}@device"
    ph = sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, build="host")
    pd = sp.Plan.from_device_csr(c["m"], c["n"], *_device_csr(c["rp"].copy(), c["col"].copy(), c["val"].copy()), fmt=fmt)
    assert pd.built_on_device() and not ph.built_on_device()
    assert pd.info()["format"] == ph.info()["format"] == fmt and pd.info()["kernel"] == ph.info()["kernel"]
    yh, _ = _execute_twice(ph, c)
    ya, yb = _execute_twice(pd, c)
    worst = _check_y(pd, c, ya, yb, what)
    if fmt != "coo":
        assert np.array_equal(ya, yh), f"{what}: differs from the host build"
    print(f"signed-parity {what} format={fmt} err/row_tol={worst:.3f}")
    ph.destroy()
    pd.destroy()
