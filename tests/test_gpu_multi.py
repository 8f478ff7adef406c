"""Plan.execute_multi (Y[:, j] = A X[:, j], k interleaved right-hand sides) on
every path: the fused DIA / ELL / JDS kernels, the generic column-by-column
path of every format, the alignment fallback, host and device blocks.

Every column j of Y is judged against independent references
(tests/multi_inputs.py): bit for bit against the oracle's sequential sum where
the plan is sequential, within signed_inputs.row_tol -- (len + 8) 2^-53
sum |a x|, no new tolerance -- for every format, and bit for bit against the
same plan's single-vector execute of that column (COO, whose atomics are
unordered: the bound only).  Y is computed once over a NaN-filled and once
over a -1.2345e300-filled buffer: the used columns must agree and the pad
columns [k, ldy) must keep their fill, bit for bit.
Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest

import guarded_buffers as gb
import multi_inputs as mi
import signed_inputs as si
import singlespmv_amd as sp
import special_values as sv

pytestmark = pytest.mark.gpu


def _plan(c, fmt, **kw):
    return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)


def _run(plan, X, m, k, ldy, fill):
    buf, Y = mi.y_block(m, k, ldy, fill)
    plan.execute_multi(X, Y)
    assert mi.pads_untouched(buf, k, fill), "execute_multi wrote a pad column of Y"
    return np.ascontiguousarray(Y)


def _twice(plan, X, m, k, ldy):
    return _run(plan, X, m, k, ldy, np.nan), _run(plan, X, m, k, ldy, mi.SENTINEL)


def _check_columns(plan, name, family, k, Ya, Yb, what):
    """The checks of the module docstring on every used column; returns the largest err / row_tol."""
    c = mi.case(name, family)
    rp, col, val = c["rp"], c["col"], c["val"]
    info = plan.info()
    coo = info["format"] == "coo"
    worst = 0.0
    for j in range(k):
        cj = mi.column(name, family, j)
        w = f"{what} column {j}"
        worst = max(worst, si.assert_rows(Ya[:, j], rp, col, val, cj["x"], w, ref=cj["ref"]))
        y1 = np.full(c["m"], np.nan)
        plan.execute(np.ascontiguousarray(cj["x"]), y1)
        if coo:
            worst = max(worst, si.assert_rows(Yb[:, j], rp, col, val, cj["x"], w + " (2nd execute)", ref=cj["ref"]))
        else:
            assert np.array_equal(mi.bits(Ya[:, j]), mi.bits(Yb[:, j])), f"{w}: depends on what Y held before"
            assert np.array_equal(mi.bits(Ya[:, j]), mi.bits(y1)), f"{w}: differs from the plan's own execute"
        if si.plan_is_sequential(info):
            assert np.array_equal(Ya[:, j], cj["y_oracle"]), f"{w}: {info['format']} is sequential, must be bit-exact"
    return worst


def _multi(plan, name, family, k, ld, what, fused):
    """One host-block execute_multi of the case at row stride ld, fully checked."""
    c = mi.case(name, family)
    _, X = mi.x_block(name, family, k, ld)
    _, Y = mi.y_block(c["m"], k, ld)
    path = plan.multi_path(X, Y)
    assert sum(path) == k
    if fused is not None:
        assert path == mi.expected_path(k, fused), (what, path)
    Ya, Yb = _twice(plan, X, c["m"], k, ld)
    worst = _check_columns(plan, name, family, k, Ya, Yb, what)
    print(f"multi {what} k={k} path={path} err/row_tol={worst:.3f}")
    return Ya


# ---------------------------------------------------------------- 1. fused DIA
@pytest.mark.parametrize("family", sorted(si.FAMILIES))
@pytest.mark.parametrize("k", [1, 2, 3, 4, 7, 8, 13, 32])
def test_fused_dia(k, family):
    """banded, 20 077 rows (odd), +-40, clipped at both edges."""
    plan = _plan(mi.case("banded", family), "dia")
    assert plan.info()["format"] == "dia"
    _multi(plan, "banded", family, k, mi.ld_for(k), f"dia-banded-{family}", fused=True)
    plan.destroy()


# ---------------------------------------------------------------- 2. DIA window limits
@pytest.mark.parametrize("k", [2, 8, 13])
@pytest.mark.parametrize("name", sorted(mi.TRIDIAGS))
def test_dia_window_limits(name, k):
    """Three diagonals 1500 / 5000 apart: the x window fits the LDS at some
    widths (tri1500) or at none (tri5000).  Whatever path is reported, the
    values must pass."""
    plan = _plan(mi.case(name, "cancel"), "dia")
    info = plan.info()
    assert info["format"] == "dia" and info["n_diags"] == 3
    _multi(plan, name, "cancel", k, mi.ld_for(k), f"dia-{name}", fused=None)
    plan.destroy()


@pytest.mark.parametrize("y_off", [0, 1])
@pytest.mark.parametrize("name", sorted(mi.TRIDIAGS))
def test_dia_single_store_branches(name, y_off):
    """The single-vector DIA kernel with its x window in LDS (tri1500, 3 513
    doubles) and with x from global memory (tri5000, 10 513 > 8 192), each
    storing the row pair as one 16-byte word (y_off 0) and as two scalars
    (y_off 1: y 8 bytes past a 16-byte boundary).  12 001 rows: the last lane
    holds one row.  Bit for bit against the oracle, guards untouched."""
    import torch
    c = mi.case(name, "cancel")
    m = c["m"]
    plan = _plan(c, "dia")
    assert plan.info()["format"] == "dia" and plan.info()["n_diags"] == 3
    x = torch.from_numpy(np.array(c["x"])).cuda()
    ybuf, y = gb.guarded_device(m, y_off, gb.Y_FILL)
    assert y.data_ptr() % 16 == 8 * y_off
    plan.execute(x, y)
    torch.cuda.synchronize()
    got = gb.used(ybuf, m, y_off)
    assert not gb.guard_damage(ybuf, m, y_off, gb.Y_FILL), f"dia-{name} y+{y_off}: a y guard was written"
    assert mi.bits(got)[m - 1] != mi.bits(np.array([gb.Y_FILL]))[0], f"dia-{name} y+{y_off}: last row not written"
    assert np.array_equal(mi.bits(got), mi.bits(c["y_oracle"])), f"dia-{name} y+{y_off}: differs from the oracle"
    plan.destroy()


# ---------------------------------------------------------------- 3. fused ELL
@pytest.mark.parametrize("family", sorted(si.FAMILIES))
@pytest.mark.parametrize("k", [2, 4, 8, 13])
@pytest.mark.parametrize("name", ["uniform16", "short"])
def test_fused_ell(name, k, family):
    """uniform16: 20 011 rows, no multiple of 64; short: 0-3 entries, empty rows, slices of width 0."""
    plan = _plan(mi.case(name, family), "ell")
    assert plan.info()["format"] == "ell"
    _multi(plan, name, family, k, mi.ld_for(k), f"ell-{name}-{family}", fused=True)
    plan.destroy()


# ---------------------------------------------------------------- 4. fused JDS
@pytest.mark.parametrize("k", [2, 8, 13])
@pytest.mark.parametrize("name,kw,fused", [("uniform16", {}, True), ("staircase", {"ell_width": 9000}, True),
                                           ("staircase", {}, False)])
def test_fused_jds(name, kw, fused, k):
    """JDS writes through its permutation; with overflow rows (staircase at
    the default width) it reports width-1 blocks and takes the generic path."""
    plan = _plan(mi.case(name, "cancel"), "jds", **kw)
    info = plan.info()
    assert info["format"] == "jds" and (info["overflow_nnz"] == 0) == fused
    _multi(plan, name, "cancel", k, mi.ld_for(k), f"jds-{name}-{'fused' if fused else 'overflow'}", fused=fused)
    plan.destroy()


# ---------------------------------------------------------------- 5. generic path
GENERIC = [("csr-auto", "csr", {"csr_lanes": 0}), ("csr-lanes1", "csr", {"csr_lanes": 1}), ("ss", "ss", {}),
           ("hyb", "hyb", {}), ("coo", "coo", {}), ("css", "css", {}), ("bin", "bin", {}),
           ("bin-nolong", "bin", {"bin_long_len": -1})]


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("name", ["staircase", "rect7x1000"])
@pytest.mark.parametrize("cid,fmt,kw", GENERIC, ids=[g[0] for g in GENERIC])
def test_generic_path(cid, fmt, kw, name, k):
    plan = _plan(mi.case(name, "cancel"), fmt, **kw)
    assert plan.info()["format"] == fmt
    _multi(plan, name, "cancel", k, mi.ld_for(k), f"{cid}-{name}", fused=False)
    plan.destroy()


@pytest.mark.parametrize("k", [1, 3, 8])
def test_generic_path_auto_powerlaw(k):
    plan = _plan(mi.case("powerlaw", "cancel"), "auto")
    fused = plan.info()["format"] in ("ell", "dia") or (plan.info()["format"] == "jds"
                                                         and plan.info()["overflow_nnz"] == 0)
    _multi(plan, "powerlaw", "cancel", k, mi.ld_for(k), f"auto-powerlaw({plan.info()['format']})", fused=fused)
    plan.destroy()


# ---------------------------------------------------------------- 6. alignment fallback
@pytest.mark.parametrize("fmt,name", [("ell", "uniform16"), ("dia", "banded")])
def test_alignment_fallback(fmt, name):
    """Device blocks starting at an odd column of a wider tensor with an odd
    row stride: all-1 widths.  The same data in aligned blocks: fused widths,
    bit-identical values."""
    import torch
    k = 8
    c = mi.case(name, "cancel")
    plan = _plan(c, fmt)
    _, X = mi.x_block(name, "cancel", k, k)
    Xw = torch.full((c["n"], k + 3), float("nan"), dtype=torch.float64, device="cuda")
    Yw = torch.full((c["m"], k + 3), mi.SENTINEL, dtype=torch.float64, device="cuda")
    assert Xw.data_ptr() % 16 == 0 and Yw.data_ptr() % 16 == 0
    Xo, Yo = Xw[:, 1:1 + k], Yw[:, 1:1 + k]  # odd start column, ld = 11
    Xo.copy_(torch.from_numpy(np.ascontiguousarray(X)))
    assert plan.multi_path(Xo, Yo) == [1] * k
    plan.execute_multi(Xo, Yo)
    torch.cuda.synchronize()
    Yu = Yw.cpu().numpy()
    sent = mi.bits(np.array([mi.SENTINEL]))[0]
    assert (mi.bits(Yu[:, :1]) == sent).all() and (mi.bits(Yu[:, 1 + k:]) == sent).all()
    Xa = torch.from_numpy(np.ascontiguousarray(X)).cuda()
    Ya = torch.full((c["m"], k), float("nan"), dtype=torch.float64, device="cuda")
    assert plan.multi_path(Xa, Ya) == mi.expected_path(k, True)
    plan.execute_multi(Xa, Ya)
    torch.cuda.synchronize()
    Yf = Ya.cpu().numpy()
    assert np.array_equal(mi.bits(Yf), mi.bits(Yu[:, 1:1 + k])), "aligned (fused) and unaligned (generic) runs differ"
    _check_columns(plan, name, "cancel", k, Yf, np.ascontiguousarray(Yu[:, 1:1 + k]), f"{fmt}-unaligned")
    # an even row stride but an odd start column: the block addresses are not 16-byte aligned
    Xe = torch.full((c["n"], k + 2), float("nan"), dtype=torch.float64, device="cuda")
    assert plan.multi_path(Xe[:, 1:1 + k], Ya) == [1] * k
    plan.destroy()


# ---------------------------------------------------------------- 7. device pointers and async
@pytest.mark.parametrize("fmt,name", [("ell", "uniform16"), ("dia", "banded")])
def test_device_blocks_async_stream(fmt, name):
    import torch
    k = 8
    c = mi.case(name, "spread")
    plan = _plan(c, fmt)
    _, X = mi.x_block(name, "spread", k, k + 2)
    Yh = _run(plan, X, c["m"], k, k + 2, np.nan)
    s = torch.cuda.Stream()
    plan.set_stream(s)
    with torch.cuda.stream(s):
        Xd = torch.from_numpy(np.ascontiguousarray(X)).cuda()
        Yd = torch.full((c["m"], k), float("nan"), dtype=torch.float64, device="cuda")
        plan.execute_multi(Xd, Yd, async_=True)
    s.synchronize()
    assert np.array_equal(mi.bits(Yd.cpu().numpy()), mi.bits(Yh)), "device / async result differs from the host call"
    assert plan.time_multi(Xd, Yd, 2) > 0
    plan.set_stream(None)
    plan.destroy()


# ---------------------------------------------------------------- 8. column isolation
@pytest.mark.parametrize("fmt,name", [("dia", "banded"), ("ell", "short"), ("csr", "staircase")])
def test_column_isolation(fmt, name):
    """X[:, j0] NaN in every row, j0 inside a fused block of k = 8: Y[:, j0]
    is non-finite on every row whose reach is non-empty, every other column is
    bit-identical to the clean run."""
    k, j0 = 8, 5
    c = mi.case(name, "cancel")
    plan = _plan(c, fmt)
    info = plan.info()
    buf, X = mi.x_block(name, "cancel", k, k + 2)
    clean = _run(plan, X, c["m"], k, k + 2, np.nan)
    buf[:, j0] = np.nan
    dirty = _run(plan, X, c["m"], k, k + 2, np.nan)
    others = [j for j in range(k) if j != j0]
    assert np.array_equal(mi.bits(dirty[:, others]), mi.bits(clean[:, others])), "a NaN column reached another column"
    rrp, _ = sv.reach(info, c["rp"], c["col"], c["m"], c["n"])
    own = np.diff(c["rp"]) > 0
    reached = np.diff(rrp) > 0
    assert own.any() and (reached | ~own).all()
    assert np.isnan(dirty[own, j0]).all(), "a non-empty row of the NaN column stayed finite"
    assert (mi.bits(dirty[~reached, j0]) == 0).all(), "a row out of the layout's reach is not +0.0"
    plan.destroy()


# ---------------------------------------------------------------- 9. degenerate shapes
def _small(m, n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, size=m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rp, rng.integers(0, max(n, 1), size=rp[-1]).astype(np.int32), rng.uniform(0.5, 2.0, rp[-1])


@pytest.mark.parametrize("fmt", ["csr", "ell", "dia", "coo", "jds", "bin"])
@pytest.mark.parametrize("m,n,empty", [(0, 5, False), (5, 0, True), (4, 4, True)])
def test_degenerate_shapes(m, n, empty, fmt):
    """m = 0, n = 0, nnz = 0 (k = 3, ldy = 5): the used columns are zero, the pad columns keep the sentinel."""
    rp, col, val = (np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)) if empty else _small(m, n, 5)
    try:
        plan = sp.Plan.from_csr(m, n, rp, col, val, fmt)
    except sp.SpmvError as e:
        assert "not supported" in str(e), e
        return
    k = 3
    X = np.full((n, 4), np.nan)
    X[:, :k] = 1.5
    for fill in (np.nan, mi.SENTINEL):
        buf, Y = mi.y_block(m, k, 5, fill)
        plan.execute_multi(X[:, :k], Y)
        assert mi.pads_untouched(buf, k, fill)
        assert (mi.bits(Y) == 0).all(), f"{fmt} {m}x{n}: used columns not +0.0"
    assert sum(plan.multi_path(X[:, :k], Y)) == k
    plan.destroy()


def test_all_empty_dia_plan():
    """A DIA plan with no stored diagonal: a strided Y must be zeroed column
    by column (a memset of 8 m bytes would hit the pads and miss the rows)."""
    m = 1000
    plan = sp.Plan.from_csr(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), "dia")
    assert plan.info()["format"] == "dia" and plan.info()["n_diags"] == 0
    k = 3
    X = np.ones((m, 4))
    for fill in (np.nan, mi.SENTINEL):
        buf, Y = mi.y_block(m, k, 5, fill)
        plan.execute_multi(X[:, :k], Y)
        assert mi.pads_untouched(buf, k, fill) and (mi.bits(Y) == 0).all()
    import torch
    Yd = torch.full((m, 6), mi.SENTINEL, dtype=torch.float64, device="cuda")
    Xd = torch.ones((m, 6), dtype=torch.float64, device="cuda")
    assert plan.multi_path(Xd[:, :4], Yd[:, :4]) == [4]
    plan.execute_multi(Xd[:, :4], Yd[:, :4])
    Yh = Yd.cpu().numpy()
    assert (mi.bits(Yh[:, :4]) == 0).all() and mi.pads_untouched(Yh, 4)
    plan.destroy()


@pytest.mark.parametrize("fmt", ["ell", "dia"])
@pytest.mark.parametrize("name", ["rect513x40", "rect7x1000"])
def test_small_rectangles(name, fmt):
    """513 x 40 and 7 x 1000: fewer columns than a workgroup has rows (DIA
    clamps almost every x row), fewer rows than a wave has lanes.  DIA takes
    them once its fill limit is lifted."""
    c = mi.case(name, "cancel")
    plan = _plan(c, fmt, **({"dia_max_fill": 1000.0} if fmt == "dia" else {}))
    assert plan.info()["format"] == fmt
    for k in (2, 13):
        _multi(plan, name, "cancel", k, mi.ld_for(k), f"{fmt}-{name}", fused=True)
    plan.destroy()


# ---------------------------------------------------------------- 10. / 11. plan state
def test_null_blocks_and_fetch_y_after_multi():
    c = mi.case("rect513x40", "cancel")
    plan = _plan(c, "ell")
    L = sp.lib()
    X = np.ones((c["n"], 2))
    Y = np.zeros((c["m"], 2))
    for xp, yp in ((None, Y.ctypes.data), (X.ctypes.data, None)):
        assert L.spmv_execute_multi(plan._h, 2, xp, 2, yp, 2, 0) == 1
        assert "NULL" in L.spmv_last_error().decode()
    # a Y_STAGED execute marks y for spmv_fetch_y; a multi execute clears the mark
    assert L.spmv_execute(plan._h, c["x"].ctypes.data, None, sp.Y_STAGED) == 0
    y = np.zeros(c["m"])
    assert L.spmv_fetch_y(plan._h, y.ctypes.data) == 0
    assert L.spmv_execute(plan._h, c["x"].ctypes.data, None, sp.Y_STAGED) == 0
    plan.execute_multi(X, Y)
    assert L.spmv_fetch_y(plan._h, y.ctypes.data) == 1
    plan.destroy()


@pytest.mark.parametrize("fmt,name", [("dia", "banded"), ("ell", "uniform16"), ("coo", "rect513x40"), ("bin", "staircase")])
def test_multi_between_single_executes(fmt, name):
    """A multi execute between two spmv_execute calls on one plan leaves both single results those of a fresh plan."""
    c = mi.case(name, "cancel")
    fresh = _plan(c, fmt)
    yf = np.full(c["m"], np.nan)
    fresh.execute(c["x"], yf)
    fresh.destroy()
    plan = _plan(c, fmt)
    y1 = np.full(c["m"], np.nan)
    plan.execute(c["x"], y1)
    _, X = mi.x_block(name, "cancel", 3, 4)
    _run(plan, X, c["m"], 3, 4, np.nan)
    y2 = np.full(c["m"], np.nan)
    plan.execute(c["x"], y2)
    if fmt == "coo":  # unordered atomics: rows inside one 128-entry unit get exactly one add
        inside = (c["rp"][:-1] // 128 == (c["rp"][1:] - 1) // 128) | (np.diff(c["rp"]) == 0)
        assert np.array_equal(y1[inside], yf[inside]) and np.array_equal(y2[inside], yf[inside])
        si.assert_rows(y2, c["rp"], c["col"], c["val"], c["x"], "coo after multi", ref=c["ref"])
    else:
        assert np.array_equal(mi.bits(y1), mi.bits(yf)) and np.array_equal(mi.bits(y2), mi.bits(yf))
    plan.destroy()
