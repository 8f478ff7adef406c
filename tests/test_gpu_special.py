"""Every format and kernel path on a poisoned x (NaN / +-Inf in a few
columns, and NaN in all but a few) and on values whose products are subnormal
(`tiny`) or reach 2^1000 (`huge`).

A term a kernel should not have added is 0 * x[c] = 0 on finite data and NaN
once x[c] is not finite: rows out of the poison's reach must be bit for bit
what the same plan gives on the clean x, rows that reference a poisoned column
must be non-finite (tests/special_values.py: the reach of every layout, the
bounds, the checkers).  Needs an MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

import signed_inputs as si
import singlespmv_amd as sp
import special_values as sv
from test_gpu_signed import CONFIGS as SIGNED_CONFIGS

pytestmark = pytest.mark.gpu

CONFIGS = SIGNED_CONFIGS + [("csr-exact", "csr", {"crs_exact": True})]

POISON_CASES = [pytest.param(name, fmt, kw, id=f"{name}-{cid}")
                for name in si.STRUCTURES for cid, fmt, kw in CONFIGS if fmt != "dia" or name == "banded"]
EXTREME_CASES = [pytest.param(name, fmt, kw, family, id=f"{name}-{cid}-{family}")
                 for name in si.STRUCTURES for cid, fmt, kw in CONFIGS if fmt != "dia" or name == "banded"
                 for family in sorted(sv.EXTREME)]


def _build(c, fmt, kw):
    try:
        return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)
    except sp.SpmvError as e:
        if "not supported" in str(e):
            pytest.skip(f"the builder refuses this configuration: {e}")
        raise


def _assert_path(name, fmt, kw, info, lens):
    """The configuration reaches the path it is here for (as test_signed_parity)."""
    if kw.get("crs_exact"):  # DIA on the band, else BIN / ELL / one-lane CSR: always a sequential layout
        assert info["format"] in ("dia", "bin", "ell", "csr") and si.plan_is_sequential(info), info
        if name == "banded":
            assert info["format"] == "dia", info["format"]
        if name in ("staircase", "powerlaw"):
            assert info["format"] == "csr" and info["csr_lanes"] == 1, info
        return
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
        if fmt == "css":
            assert info["css_split_rows"] > 0
    if kw.get("ell_width") == 9000:
        assert info["overflow_nnz"] == 0 and si.plan_is_sequential(info)
    if fmt == "bin" and not kw and name in ("staircase", "powerlaw"):  # the long rows' run path
        assert info["bin_long_rows"] > 0 and info["bin_long_len"] > 0, info
    if kw.get("bin_long_len") == 40 and (lens >= 40).any():
        assert info["bin_long_rows"] > 0 and info["bin_long_len"] == 40
    if kw.get("bin_long_len") == -1:
        assert info["bin_long_len"] == 0 and info["bin_long_rows"] == 0 and si.plan_is_sequential(info)
    if fmt == "dia":
        assert si.plan_is_sequential(info)


@functools.lru_cache(maxsize=None)
def _reached(name, which, kind):
    """Rows whose reach (of a layout of `kind`: exact / padded / dia) meets a
    poisoned column of the forward or inverse case -- once per structure."""
    c = (sv.forward_case if which == "forward" else sv.inverse_case)(name)
    info = {"format": {"exact": "csr", "padded": "ell", "dia": "dia"}[kind]}
    out = sv.rows_touching(*sv.reach(info, c["rp"], c["col"], c["m"], c["n"]), c["poisoned"])
    out.setflags(write=False)
    return out


def _coo_split_rows(rp):
    """COO rows split across 128-entry units: unordered f64 atomics, y may
    round differently run to run (test_gpu_signed._check_y)."""
    inside = (rp[:-1] // 128 == (rp[1:] - 1) // 128) | (np.diff(rp) == 0)
    return ~inside


def _run(plan, x, m):
    y = np.full(m, np.nan)
    plan.execute(np.ascontiguousarray(x), y)
    return y


@pytest.mark.parametrize("name,fmt,kw", POISON_CASES)
def test_poisoned_x(name, fmt, kw, request):
    """One plan from the forward case's val (stored zeros on every second
    poisoned column), three executes over a NaN-filled y: the clean x, the
    forward poison (NaN, +Inf, -Inf in columns 0, n - 1 and a few more), the
    inverse poison (NaN everywhere but on the columns of a few short rows)."""
    f = sv.forward_case(name)
    m, n, rp, col, val = f["m"], f["n"], f["rp"], f["col"], f["val"]
    lens = np.diff(rp)
    what = request.node.callspec.id
    plan = _build(f, fmt, kw)
    info = plan.info()
    _assert_path(name, fmt, kw, info, lens)
    fm = info["format"]
    kind = "exact" if fm in sv.EXACT_REACH else "padded" if fm in sv.PADDED_REACH else "dia"
    loose = _coo_split_rows(rp) if fm == "coo" else None

    # 1. clean x
    y0 = _run(plan, f["x_clean"], m)
    si.assert_rows(y0, rp, col, val, f["x_clean"], what + " (clean x)", ref=f["ref"])
    assert (sv.bits(y0[lens == 0]) == 0).all(), f"{what}: an empty row is not +0.0"
    if si.plan_is_sequential(info):
        assert np.array_equal(y0, f["y_clean"]), f"{what}: {fm} is sequential, must be bit-exact"

    # 2. forward poison, 3. inverse poison
    extra = {}
    for which, c in (("forward", f), ("inverse", sv.inverse_case(name))):
        y = _run(plan, c["x"], m)
        reached = _reached(name, which, kind)
        y_class = sv.classify(c["y_oracle"]) if kind == "exact" else None
        extra[which] = sv.assert_poisoned(y, y0, c["hit"], reached, f"{what} ({which} poison)", y_class=y_class,
                                          loose=loose, rp=rp, ref=f["ref"])
        if kind == "exact":
            assert np.array_equal(reached, c["hit"]) and extra[which] == 0
    print(f"poisoned-x {what} format={fm} in-reach-not-referenced rows turned non-finite: "
          f"forward {extra['forward']} of {int((_reached(name, 'forward', kind) & ~f['hit']).sum())}, "
          f"inverse {extra['inverse']} of {int((_reached(name, 'inverse', kind) & ~sv.inverse_case(name)['hit']).sum())}")
    plan.destroy()


@pytest.mark.parametrize("name,fmt,kw,family", EXTREME_CASES)
def test_extreme_range(name, fmt, kw, family, request):
    """`tiny` (every product and every sum subnormal: no flush to zero
    anywhere, atomics included) and `huge` (products up to 2^1000): each row
    within its derived bound, bit for bit the sequential sum where the layout
    is sequential, identical over a NaN-filled and a -1.2345e300-filled y."""
    c = sv.extreme_case(name, family)
    m, rp = c["m"], c["rp"]
    lens = np.diff(rp)
    what = request.node.callspec.id
    plan = _build(c, fmt, kw)
    info = plan.info()
    _assert_path(name, fmt, kw, info, lens)
    ya = np.full(m, np.nan)
    plan.execute(c["x"], ya)
    yb = np.full(m, -1.2345e300)
    plan.execute(c["x"], yb)
    worst = sv.assert_extreme(family, ya, rp, c["ref"], what)
    if info["format"] == "coo":
        worst = max(worst, sv.assert_extreme(family, yb, rp, c["ref"], what + " (2nd execute)"))
        inside = ~_coo_split_rows(rp)
        assert np.array_equal(sv.bits(ya[inside]), sv.bits(yb[inside])), f"{what}: rows inside one unit differ run to run"
    else:
        assert np.array_equal(sv.bits(ya), sv.bits(yb)), f"{what}: y depends on what y held before"
    assert (sv.bits(ya[lens == 0]) == 0).all(), f"{what}: an empty row is not +0.0"
    if si.plan_is_sequential(info):
        assert np.array_equal(ya, c["y_oracle"]), f"{what}: {info['format']} is sequential, must be bit-exact"
    print(f"extreme-range {what} format={info['format']} err/tol={worst:.3f}")
    plan.destroy()
