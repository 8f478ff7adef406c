"""CPU checks of tests/guarded_buffers.py: the stair_tail structure, the
guarded buffers' alignment and the route checker itself -- what keeps
tests/test_gpu_routes.py honest.
"""
import numpy as np
import pytest

import guarded_buffers as gb
import multi_inputs as mi
import signed_inputs as si

CSR = {"format": "csr"}
COO = {"format": "coo"}


def _case():
    return gb.case(gb.STAIR_TAIL)


def test_stair_tail_is_what_the_gpu_tests_rely_on():
    m, n, rp, col = gb.structure(gb.STAIR_TAIL)
    c = _case()
    lens = np.diff(rp)
    assert (m, n) == (2041, 2048) and m == 13 * 157 and all(m % k for k in (2, 64, 256, 512))
    assert len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(col) and (col >= 0).all() and (col < n).all()
    assert lens[1022] == 4097 and lens[m - 1] == 9000 and sorted(np.flatnonzero(lens > 700).tolist()) == [1022, m - 1]
    assert set(si.STAIR_LENS) | {4097, 9000} == set(lens.tolist())  # every staircase length, empty rows included
    assert (lens == 0).sum() > 100
    # the staircase's rows 7.., columns unchanged
    ms, ns, rps, cols = si.structure("staircase")
    assert np.array_equal(lens, np.diff(rps)[7:]) and np.array_equal(col, cols[rps[7]:])
    assert set(c) == set(si.case("rect7x1000", "cancel")) and c["m"] == m and c["n"] == n
    assert np.array_equal(c["row"], np.repeat(np.arange(m), lens))
    # the rows cancel (as signed_inputs' cancel family promises) and the sequential sum is within the bound
    rows = (lens >= 2) & (lens % 2 == 0)
    y_hi, mag = c["ref"]
    ok = np.abs(y_hi[rows]) <= 1e-12 * mag[rows]
    assert rows.sum() > 0 and ok.sum() >= 0.95 * rows.sum()
    assert (mag[lens > 0] >= 0.5 * lens[lens > 0] * (1 - 1e-12)).all()
    worst = si.assert_rows(c["y_oracle"], rp, col, c["val"], c["x"], "oracle stair_tail", ref=c["ref"])
    print(f"oracle err/row_tol stair_tail/cancel: {worst:.3f}")
    assert worst <= 1.0
    # COO: both kinds of row exist, among the split ones rows that do not cancel
    inside = gb.coo_inside(rp)
    assert inside[lens == 0].all() and (inside & (lens > 0)).any() and (~inside & (lens % 2 == 1)).any()
    # other names are signed_inputs' cases themselves
    assert gb.case("rect513x40") is si.case("rect513x40", "cancel")


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 40, 513, 2041])
def test_guarded_view_alignment(n, off):
    buf, view = gb.guarded(n, off, gb.Y_FILL)
    assert buf.ctypes.data % 16 == 0 and view.ctypes.data % 16 == 8 * off
    assert view.ctypes.data - buf.ctypes.data == 8 * (gb.GUARD + off)
    assert len(view) == n and len(buf) == 2 * gb.GUARD + off + n
    assert gb.guards_intact(buf, n, off, gb.Y_FILL)
    view[:] = 1.0
    assert gb.guards_intact(buf, n, off, gb.Y_FILL) and (gb.used(buf, n, off) == 1.0).all()
    assert (mi.bits(buf) == mi.bits(np.array([gb.Y_FILL]))[0]).sum() == 2 * gb.GUARD + off


def _correct(off=1, fill=gb.Y_FILL):
    """A guarded y buffer holding the oracle's y of stair_tail."""
    c = _case()
    buf, view = gb.guarded(c["m"], off, fill)
    view[:] = c["y_oracle"]
    return c, buf, view


def _check(c, buf, view, off=1, info=CSR, alpha=1.0, y_base=None, **kw):
    gb.check_route(np.array(view), c["y_oracle"] if y_base is None else y_base, c, info, "cpu", alpha=alpha,
                   guards=[("y", buf, c["m"], off, gb.Y_FILL)], **kw)


@pytest.mark.parametrize("off", [0, 1])
def test_checker_passes_a_correct_y(off):
    c, buf, view = _correct(off)
    _check(c, buf, view, off)
    _check(c, buf, view, off, info=COO)


@pytest.mark.parametrize("at,where", [(lambda m: m, "y[m]"), (lambda m: -1, "y[-1]"),
                                      (lambda m: m + gb.GUARD - 1, "the last guard word"),
                                      (lambda m: -gb.GUARD - 1, "the first guard word")], ids=["m", "-1", "last", "first"])
def test_checker_catches_a_write_to_a_guard(at, where):
    c, buf, view = _correct()
    lo = gb.GUARD + 1
    buf[lo + at(c["m"])] = 0.0
    assert not gb.guards_intact(buf, c["m"], 1, gb.Y_FILL), where
    with pytest.raises(AssertionError, match="guards were written"):
        _check(c, buf, view)


def test_checker_catches_a_used_entry_left_at_the_fill():
    for fill in (np.nan, gb.Y_FILL):
        for r in (0, 1022, 2040):
            c, buf, view = _correct()
            view[r] = fill
            with pytest.raises(AssertionError, match="rows differ"):
                _check(c, buf, view)


def test_checker_compares_nan_guards_by_bits():
    n = 40
    buf, view = gb.guarded(n, 1, gb.X_FILL)
    view[:] = 1.0
    assert gb.guards_intact(buf, n, 1, gb.X_FILL)
    other = np.array([mi.bits(np.array([gb.X_FILL]))[0] ^ 1], np.int64).view(np.float64)[0]
    assert np.isnan(other)
    buf[gb.GUARD + 1 + n] = other  # still a NaN, another payload
    assert not gb.guards_intact(buf, n, 1, gb.X_FILL)
    assert gb.guard_damage(buf, n, 1, gb.X_FILL) == [n]


@pytest.mark.parametrize("alpha", [-2.0, 0.75])
@pytest.mark.parametrize("times", [0, 2], ids=["not-scaled", "scaled-twice"])
def test_checker_catches_a_row_scaled_wrongly(times, alpha):
    c, buf, view = _correct()
    view[:] = alpha * c["y_oracle"]
    _check(c, buf, view, alpha=alpha)
    r = 1022  # 4097 entries: an odd row, |y| >= 0.5
    view[r] = c["y_oracle"][r] * alpha ** times
    with pytest.raises(AssertionError, match="rows differ"):
        _check(c, buf, view, alpha=alpha)


def test_checker_alpha_zero_keeps_signed_zeros():
    c, buf, view = _correct()
    view[:] = 0.0 * c["y_oracle"]
    assert (mi.bits(np.array(view)) != 0).any()  # -0.0 where y is negative
    _check(c, buf, view, alpha=0.0)
    view[:] = 0.0
    with pytest.raises(AssertionError, match="rows differ"):
        _check(c, buf, view, alpha=0.0)


def test_checker_coo_rules():
    """COO: a row inside one unit is held bit for bit, a split row to row_tol;
    a tripled row (a zero_y that ran once for three executes) is caught in both."""
    c, buf, view = _correct()
    rp, lens = c["rp"], np.diff(c["rp"])
    inside = gb.coo_inside(rp)
    odd = lens % 2 == 1
    ri = int(np.flatnonzero(inside & odd)[0])
    rs = int(np.flatnonzero(~inside & odd & (lens >= 129))[-1])
    # one ulp on a split row is run-to-run noise, on an inside row a failure
    view[rs] = np.nextafter(view[rs], np.inf)
    _check(c, buf, view, info=COO)
    with pytest.raises(AssertionError, match="rows differ"):
        _check(c, buf, view, info=CSR)
    view[ri] = np.nextafter(view[ri], np.inf)
    with pytest.raises(AssertionError, match="inside one unit"):
        _check(c, buf, view, info=COO)
    for r, msg in ((ri, "inside one unit"), (rs, "beyond .alpha. row_tol")):
        c, buf, view = _correct()
        view[r] = 3.0 * c["y_oracle"][r]
        with pytest.raises(AssertionError, match=msg):
            _check(c, buf, view, info=COO)
    # alpha = -2: exact scaling, the split rows keep their (scaled) bound; alpha = 0.75: inside rows only
    c, buf, view = _correct()
    view[:] = -2.0 * c["y_oracle"]
    view[rs] = np.nextafter(view[rs], np.inf)
    _check(c, buf, view, info=COO, alpha=-2.0)
    view[rs] = c["y_oracle"][rs]  # not scaled
    with pytest.raises(AssertionError, match="beyond .alpha. row_tol"):
        _check(c, buf, view, info=COO, alpha=-2.0)
    view[:] = 0.75 * c["y_oracle"]
    view[rs] = np.nextafter(view[rs], np.inf)
    _check(c, buf, view, info=COO, alpha=0.75)
    view[ri] = c["y_oracle"][ri]
    with pytest.raises(AssertionError, match="inside one unit"):
        _check(c, buf, view, info=COO, alpha=0.75)


def test_expected_of_a_scaled_x_keeps_positive_zeros():
    """A x with x scaled by -2 is -2 (A x) bit for bit, except that a sum of
    nothing stays +0.0 (alpha * y would make it -0.0)."""
    import oracle
    c = _case()
    y2 = oracle.csr_spmv(c["rp"], c["col"], np.ascontiguousarray(c["val"]), -2.0 * c["x"])
    want = gb.expected(c["y_oracle"], -2.0, scaled_x=True)
    assert np.array_equal(mi.bits(y2), mi.bits(want))
    assert not np.array_equal(mi.bits(y2), mi.bits(gb.expected(c["y_oracle"], -2.0)))
    buf, view = gb.guarded(c["m"], 1, gb.Y_FILL)
    view[:] = y2
    _check(c, buf, view, alpha=-2.0, scaled_x=True)
    with pytest.raises(AssertionError, match="rows differ"):
        _check(c, buf, view, alpha=-2.0)


def test_a_pad_column_read_from_the_guard_poisons_the_row():
    """The CPU model of a kernel that multiplies a zero pad value by x[n] or
    x[-1]: one extra 0.0 * guard term makes the row NaN, which the bit-for-bit
    comparison (and row_tol) rejects."""
    c = _case()
    xbuf, xview = gb.guarded(c["n"], 1, gb.X_FILL)
    xview[:] = c["x"]
    lo = gb.GUARD + 1
    for r, at in ((0, -1), (c["m"] - 1, c["n"])):
        js = slice(int(c["rp"][r]), int(c["rp"][r + 1]))
        acc = 0.0
        for a, j in zip(c["val"][js], c["col"][js]):
            acc += a * xbuf[lo + j]
        assert acc == c["y_oracle"][r]
        acc += 0.0 * xbuf[lo + at]
        assert np.isnan(acc)
        y = np.array(c["y_oracle"])
        y[r] = acc
        with pytest.raises(AssertionError, match="rows differ"):
            gb.check_route(y, c["y_oracle"], c, CSR, "cpu")
        assert si.failing_rows(y, c["rp"], c["ref"])[0].tolist() == [r]
