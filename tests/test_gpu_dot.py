"""Plan.execute_dot (y = A x, dots[0] = w . y, dots[1] = y . y from the same
pass) on every format and kernel path: y bit for bit what plan.execute gives,
both dots within the bound of tests/dot_inputs.py against the exact rational
sums over the y the call returned, the integer family's dots exact, and the
same 16 bytes whatever y held before.  Then the path each plan takes, stale
partials, guarded offset buffers, w = x and w = None, non-finite x and w, the
host / device / stream / staged routes, and degenerate shapes.
Needs an MI355X: `pytest -m gpu`.
"""
import ctypes as C

import numpy as np
import pytest

import dot_inputs as di
import guarded_buffers as gb
import multi_inputs as mi
import signed_inputs as si
import singlespmv_amd as sp

pytestmark = pytest.mark.gpu

ADAPTIVE = ("csr-lanes0", "csr", {"csr_lanes": 0})
SKEWED = [ADAPTIVE, ("hyb", "hyb", {}), ("ss", "ss", {}), ("coo", "coo", {}), ("css", "css", {}), ("bin", "bin", {}),
          ("bin-nolong", "bin", {"bin_long_len": -1}), ("jds", "jds", {})]
DIA_FILL = ("dia", "dia", {"dia_max_fill": 1000})
CONFIGS = {
    "staircase": SKEWED,
    "powerlaw": SKEWED,
    "uniform16": [ADAPTIVE] + [(f"csr-lanes{k}", "csr", {"csr_lanes": k}) for k in (1, 2, 4, 8, 16, 32, 64)]
                 + [("csr-lanes4-rp64", "csr", {"csr_lanes": 4, "csr_row_ptr64": True}),
                    ("csr-lanes16-rp64", "csr", {"csr_lanes": 16, "csr_row_ptr64": True}),
                    ("ell", "ell", {}), ("jds", "jds", {}), ("bin", "bin", {})],
    "banded": [("dia", "dia", {}), ("csr", "csr", {}), ("ell", "ell", {})]
              + [(f"csr-lanes{k}", "csr", {"csr_lanes": k}) for k in (1, 4, 16, 64)],
    "short": [("ell", "ell", {}), ("ss", "ss", {})],
    "rect513x40": [("csr", "csr", {}), ("ell", "ell", {}), DIA_FILL],
    "rect7x1000": [("csr", "csr", {}), ("ell", "ell", {}), DIA_FILL],
    "tri1500": [("dia", "dia", {})],
    "tri5000": [("dia", "dia", {})],
}
SPREAD_TOO = ("csr-lanes0", "ell", "dia", "bin")  # as tests/test_gpu_axpby.py
CASES = [pytest.param(name, family, fmt, kw, id=f"{name}-{family}-{cid}")
         for name, cfgs in CONFIGS.items() for cid, fmt, kw in cfgs
         for family in (("cancel", "spread", "integer") if cid in SPREAD_TOO else ("cancel", "integer"))]


def _case(name, family):
    """The case and its w: the integer family brings its own."""
    if family == "integer":
        c = di.int_case(name)
        return c, c["w"]
    c = di.case(name, family)
    return c, di.w(c["m"])


def _plan(c, fmt, **kw):
    return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)


def _execute(plan, x, m):
    s = np.full(m, np.nan)
    plan.execute(np.ascontiguousarray(x), s)
    return s


def _dot(plan, x, w, m, fill=np.nan):
    """(y, (wy, yy)) through host buffers."""
    y = np.full(m, fill)
    d = plan.execute_dot(np.ascontiguousarray(x), y, None if w is None else np.ascontiguousarray(w))
    return y, d


def _dot_dev(plan, xd, wd, m, fill):
    """(y, (wy, yy)) on a device y that held `fill`, host dots."""
    import torch
    yd = torch.full((m,), fill, dtype=torch.float64, device="cuda")
    d = plan.execute_dot(xd, yd, wd)
    return yd.cpu().numpy(), d


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, np.float64)).cuda()


def _assert_bits(y, want, what):
    rows = np.flatnonzero(di.bits(y) != di.bits(want))
    assert not len(rows), (f"{what}: {len(rows)} entries differ, first {rows[:5].tolist()}: "
                           f"{np.asarray(y)[rows[:3]].tolist()} vs {np.asarray(want)[rows[:3]].tolist()}")


def _same16(d, want, what):
    assert di.bits(d).tolist() == di.bits(want).tolist(), f"{what}: dots {d!r} vs {want!r}"


# ---------------------------------------------------------------- 1. parity on every path
@pytest.mark.parametrize("name,family,fmt,kw", CASES)
def test_dot_parity(name, family, fmt, kw, request):
    c, w = _case(name, family)
    what = request.node.callspec.id
    m = c["m"]
    plan = _plan(c, fmt, **kw)
    try:
        info = plan.info()
        assert info["format"] == fmt
        coo = fmt == "coo"
        s = _execute(plan, c["x"], m)
        y, d = _dot(plan, c["x"], w, m)
        if family == "integer":
            _assert_bits(y, c["y"], f"{what}: y vs the exact integers")
            _same16(d, (float(c["wy"]), float(c["yy"])), f"{what}: the integer dots are exact in every order")
        elif coo:
            si.assert_rows(y, c["rp"], c["col"], c["val"], c["x"], what, ref=c["ref"])
        if not coo:
            _assert_bits(y, s, f"{what}: y vs plan.execute")
        worst = di.assert_dots(d, y, w, what)
        assert d[1] >= 0.0
        if not coo:  # whatever y held before: the same 16 bytes, the same y
            xd, wd = _dev(c["x"]), _dev(w)
            for fill in (np.nan, mi.SENTINEL):
                y2, d2 = _dot_dev(plan, xd, wd, m, fill)
                _assert_bits(y2, s, f"{what}: y over a y of {fill}")
                _same16(d2, d, f"{what}: over a y of {fill}")
        print(f"dot-parity {what} path={plan.dot_path()} err/bound={worst:.3g}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 2. the path each plan takes
FUSED = ([("banded", "dia", {}), ("uniform16", "ell", {}), ("short", "ell", {}), ("uniform16", "jds", {}),
          ("staircase", "jds", {"ell_width": 9000}), ("staircase", "csr", {"csr_lanes": 0}),
          ("powerlaw", "csr", {"csr_lanes": 0})]
         + [(name, "csr", {"csr_lanes": k, "csr_row_ptr64": bool(rp64)}) for name in ("uniform16", "banded")
            for k in (4, 16) for rp64 in (0, 1)]
         # the other lane counts have their twins too (the issue leaves their path open)
         + [(name, "csr", {"csr_lanes": k}) for name in ("uniform16", "banded") for k in (1, 2, 8, 32, 64)])
GENERIC = [("powerlaw", "ss", {}), ("powerlaw", "coo", {}), ("powerlaw", "css", {}), ("powerlaw", "bin", {}),
           ("uniform16", "bin", {}), ("staircase", "hyb", {}), ("uniform16", "hyb", {}), ("staircase", "jds", {})]
PATHS = [pytest.param(n, f, kw, path, id=f"{n}-{f}-" + "-".join(f"{k}{int(v)}" for k, v in kw.items()) + f"-{path}")
         for group, path in ((FUSED, "fused"), (GENERIC, "generic")) for n, f, kw in group]


@pytest.mark.parametrize("name,fmt,kw,path", PATHS)
def test_dot_path(name, fmt, kw, path):
    c, w = _case(name, "cancel")
    plan = _plan(c, fmt, **kw)
    try:
        info = plan.info()
        assert info["format"] == fmt
        got = plan.dot_path()
        assert got == path, got
        if fmt == "jds":
            assert (info["overflow_nnz"] == 0) == (path == "fused"), info["overflow_nnz"]
        if fmt == "csr" and kw.get("csr_lanes") == 0:
            assert info["kernel"] == "csr_adaptive_kernel", info["kernel"]
        y, d = _dot(plan, c["x"], w, c["m"])
        if fmt != "coo":
            _assert_bits(y, _execute(plan, c["x"], c["m"]), f"{name}-{fmt}-{kw}")
        di.assert_dots(d, y, w, f"{name}-{fmt}-{kw}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 3. stale partials
STALE = {"csr-adaptive": ("csr", {"csr_lanes": 0}, "uniform16", "staircase"), "ell": ("ell", {}, "uniform16", "staircase"),
         "dia": ("dia", {}, "banded", "tri1500"), "bin": ("bin", {}, "uniform16", "staircase")}


@pytest.mark.parametrize("cfg", sorted(STALE))
def test_no_slot_carries_an_earlier_call(cfg):
    """A call whose dots are 1e150 times larger, then the ordinary call on the
    same plan; then a plan of another structure right after the first was
    destroyed (the allocator may hand it the same memory): every slot of the
    second call is its own.  uniform16 then staircase, except for DIA, whose
    layout suits neither (nearly all fill): banded then tri1500."""
    fmt, kw, first, second = STALE[cfg]
    c, w = _case(first, "cancel")
    plan = _plan(c, fmt, **kw)
    try:
        y, big = _dot(plan, c["x"], w * 1e150, c["m"])
        di.assert_dots(big, y, w * 1e150, f"{cfg} {first}: w scaled by 1e150")
        assert abs(big[0]) > 1e100  # (a cancelling y is rounding noise: 1e-13 * 1e150)
        y, d = _dot(plan, c["x"], w, c["m"])
        di.assert_dots(d, y, w, f"{cfg} {first}: the ordinary call after the scaled one")
        y, d = _dot(plan, c["x"], None, c["m"])
        di.assert_dots(d, y, None, f"{cfg} {first}: no w after a w")
    finally:
        plan.destroy()
    c, w = _case(second, "cancel")
    plan = _plan(c, fmt, **kw)
    try:
        y, d = _dot(plan, c["x"], w, c["m"])
        di.assert_dots(d, y, w, f"{cfg} {second}: a new plan after {first}'s was destroyed")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 4. guarded, offset device buffers
GUARDED = [("tri1500", "dia", {}), ("tri5000", "dia", {}), ("uniform16", "csr", {}), ("banded", "csr", {}),
           ("short", "ell", {}), ("uniform16", "bin", {})]


@pytest.mark.parametrize("name,fmt,kw", [pytest.param(*g, id=f"{g[0]}-{g[1]}") for g in GUARDED])
def test_guarded_offset_buffers(name, fmt, kw):
    """x, y and w in guarded device buffers, y and w each at the allocation's
    16-byte-aligned base or one double into it (their alignments are
    independent); w's guards hold NaN, so one read past either end of w makes
    dots[0] NaN."""
    import torch
    c, w = _case(name, "cancel")
    m, n = c["m"], c["n"]
    plan = _plan(c, fmt, **kw)
    try:
        assert plan.info()["format"] == fmt
        s = _execute(plan, c["x"], m)
        assert di.bits(s)[-1] != di.bits([gb.Y_FILL])[0]
        xbuf, xv = gb.guarded_device(n, 0, gb.X_FILL)
        xv.copy_(torch.from_numpy(np.array(c["x"])))
        seen = set()
        for y_off in (0, 1):
            for w_off in (0, 1):
                what = f"{name}-{fmt} y+{y_off} w+{w_off}"
                ybuf, yv = gb.guarded_device(m, y_off, gb.Y_FILL)
                wbuf, wv = gb.guarded_device(m, w_off, float("nan"))
                wv.copy_(torch.from_numpy(np.array(w)))
                assert yv.data_ptr() % 16 == 8 * y_off and wv.data_ptr() % 16 == 8 * w_off
                d = plan.execute_dot(xv, yv, wv)
                torch.cuda.synchronize()
                for label, buf, k, off, fill in (("y", ybuf, m, y_off, gb.Y_FILL), ("x", xbuf, n, 0, gb.X_FILL),
                                                 ("w", wbuf, m, w_off, float("nan"))):
                    bad = gb.guard_damage(buf, k, off, fill)
                    assert not bad, f"{what}: the {label} guards were written at {bad[:8]}"
                y = gb.used(ybuf, m, y_off)
                _assert_bits(y, s, what)
                assert di.bits(y)[-1] == di.bits(s)[-1], f"{what}: the last row was not written"
                assert np.isfinite(d).all(), f"{what}: dots {d!r}"
                di.assert_dots(d, y, w, what)
                seen.add(tuple(di.bits(d).tolist()))
        # the order of the adds is a function of the plan and the path, not of the alignments
        assert len(seen) == 1, f"{name}-{fmt}: the dots depend on the alignment of y or w: {seen}"
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 5. aliasing and NULL
@pytest.mark.parametrize("name,fmt,kw", [("uniform16", "csr", {"csr_lanes": 4}), ("banded", "dia", {}),
                                         ("uniform16", "ell", {}), ("powerlaw", "csr", {"csr_lanes": 0}),
                                         ("powerlaw", "bin", {})], ids=lambda v: v if isinstance(v, str) else None)
def test_w_is_x_and_w_is_null(name, fmt, kw):
    c, w = _case(name, "cancel")
    m = c["m"]
    assert m == c["n"]
    plan = _plan(c, fmt, **kw)
    try:
        s = _execute(plan, c["x"], m)
        xd = _dev(c["x"])
        y, d = _dot_dev(plan, xd, xd, m, np.nan)  # CG's p . Ap
        _assert_bits(y, s, f"{name}-{fmt} w = x")
        di.assert_dots(d, y, c["x"], f"{name}-{fmt} w = x")
        _assert_bits(xd.cpu().numpy(), c["x"], f"{name}-{fmt}: x after w = x")
        for route in ("host", "device"):
            y0, d0 = _dot(plan, c["x"], None, m) if route == "host" else _dot_dev(plan, xd, None, m, np.nan)
            _assert_bits(y0, s, f"{name}-{fmt} w = None ({route})")
            assert di.bits([d0[0]])[0] == 0, f"{name}-{fmt} w = None ({route}): dots[0] = {d0[0]!r}, not +0.0"
            di.assert_dots(d0, y0, None, f"{name}-{fmt} w = None ({route})")
            _same16([d0[1]], [d[1]], f"{name}-{fmt} ({route}): y . y with and without a w")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 6. non-finite x and w
FAMILIES = [("banded", "dia", {}), ("uniform16", "ell", {}), ("uniform16", "jds", {}), ("uniform16", "csr", {"csr_lanes": 4}),
            ("banded", "csr", {"csr_lanes": 16}), ("powerlaw", "csr", {"csr_lanes": 0}), ("powerlaw", "bin", {})]
FAMILY_IDS = [f"{n}-{f}" + ("-adaptive" if kw.get("csr_lanes") == 0 else "") for n, f, kw in FAMILIES]


@pytest.mark.parametrize("name,fmt,kw", FAMILIES, ids=FAMILY_IDS)
def test_nan_in_x_reaches_both_dots(name, fmt, kw):
    c, w = _case(name, "cancel")
    m = c["m"]
    plan = _plan(c, fmt, **kw)
    try:
        x = np.array(c["x"])
        x[int(c["col"][len(c["col"]) // 2])] = np.nan
        with np.errstate(invalid="ignore"):
            s = _execute(plan, x, m)
            y, d = _dot(plan, x, w, m)
        assert np.isnan(s).any() and np.isfinite(s).any()
        _assert_bits(y, s, f"{name}-{fmt}: y with a NaN in x")
        assert np.isnan(d[0]) and np.isnan(d[1]), d
    finally:
        plan.destroy()


@pytest.mark.parametrize("name,fmt,kw", FAMILIES, ids=FAMILY_IDS)
def test_nan_in_w_reaches_dots0_only(name, fmt, kw):
    c, w = _case(name, "cancel")
    m = c["m"]
    plan = _plan(c, fmt, **kw)
    try:
        y, d = _dot(plan, c["x"], w, m)
        r = int(np.flatnonzero(np.diff(c["rp"]) > 0)[-1])  # the last non-empty row
        w2 = np.array(w)
        w2[r] = np.nan
        y2, d2 = _dot(plan, c["x"], w2, m)
        assert np.isnan(d2[0]), d2
        _same16([d2[1]], [d[1]], f"{name}-{fmt}: y . y with a NaN in w")
        _assert_bits(y2, y, f"{name}-{fmt}: y with a NaN in w")
    finally:
        plan.destroy()


EMPTY_ROWS = [("staircase", "csr", {"csr_lanes": 0}), ("short", "csr", {"csr_lanes": 4}), ("short", "ell", {}),
              ("staircase", "jds", {"ell_width": 9000}), ("rect513x40", "dia", {"dia_max_fill": 1000}),
              ("powerlaw", "bin", {}), ("short", "ss", {})]


@pytest.mark.parametrize("name,fmt,kw", EMPTY_ROWS, ids=[f"{n}-{f}" for n, f, _ in EMPTY_ROWS])
def test_inf_in_w_on_an_empty_row(name, fmt, kw):
    """No shortcut for zeros: an empty row contributes w[r] * (+0.0), NaN for w[r] = Inf."""
    c, w = _case(name, "cancel")
    m = c["m"]
    plan = _plan(c, fmt, **kw)
    try:
        y, d = _dot(plan, c["x"], w, m)
        empty = np.flatnonzero(np.diff(c["rp"]) == 0)
        assert len(empty)
        for r in (int(empty[0]), int(empty[-1])):
            w2 = np.array(w)
            w2[r] = np.inf
            y2, d2 = _dot(plan, c["x"], w2, m)
            assert di.bits(y2)[r] == 0, f"{name}-{fmt}: y[{r}] of an empty row is {y2[r]!r}"
            assert np.isnan(d2[0]), f"{name}-{fmt}: w[{r}] = Inf on an empty row gave dots[0] = {d2[0]!r}"
            _same16([d2[1]], [d[1]], f"{name}-{fmt}: y . y with an Inf in w")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 7. routes
@pytest.mark.parametrize("name,fmt", [("uniform16", "csr"), ("short", "ss")])
def test_routes(name, fmt):
    import torch
    c, w = _case(name, "cancel")
    m, n = c["m"], c["n"]
    L = sp.lib()
    fresh = _plan(c, fmt)
    try:
        s = _execute(fresh, c["x"], m)
    finally:
        fresh.destroy()
    plan = _plan(c, fmt)
    try:
        h = plan._h
        x = np.ascontiguousarray(c["x"])
        wh = np.ascontiguousarray(w)
        dots = np.full(2, -3.0)
        y = np.full(m, 7.0)

        def call(xp, yp, wp, dp, flags):
            return L.spmv_execute_dot(h, xp, yp, wp, dp, flags)

        # SPMV_X_STAGED before any host x was staged: refused, y and dots untouched
        assert call(None, y.ctypes.data, wh.ctypes.data, dots.ctypes.data, sp.X_STAGED) == 1
        assert "X_STAGED" in L.spmv_last_error().decode() and (y == 7.0).all() and (dots == -3.0).all()
        _assert_bits(_execute(plan, x, m), s, f"{fmt}: execute before any dot execute")
        bytes0 = plan.info()["device_bytes"]
        # host x, y, w, dots
        yh, d = _dot(plan, x, w, m)
        _assert_bits(yh, s, f"{fmt} host")
        di.assert_dots(d, yh, w, f"{fmt} host")
        # the partials and the w staging are counted
        assert plan.info()["device_bytes"] >= bytes0 + 8 * m + 16
        # SPMV_X_STAGED after a host call (x may be NULL)
        assert call(None, y.ctypes.data, wh.ctypes.data, dots.ctypes.data, sp.X_STAGED) == 0, L.spmv_last_error()
        _assert_bits(y, s, f"{fmt} staged x")
        _same16(dots, d, f"{fmt} staged x")
        # device x, y, w with host dots
        xd, wd = _dev(x), _dev(w)
        yd, dd = _dot_dev(plan, xd, wd, m, np.nan)
        _assert_bits(yd, s, f"{fmt} device")
        _same16(dd, d, f"{fmt} device x, y, w, host dots")
        # everything on the device, on a side stream, async
        ya = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        da = torch.full((2,), -3.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        plan.set_stream(side)
        try:
            assert plan.execute_dot(xd, ya, wd, dots=da, async_=True) is None
            side.synchronize()
        finally:
            plan.set_stream(None)
        _assert_bits(ya.cpu().numpy(), s, f"{fmt} device async")
        _same16(da.cpu().numpy(), d, f"{fmt} all device, async")
        # time_dot: the dots of the last iteration are the same again
        da.fill_(-3.0)
        assert plan.time_dot(xd, ya, wd, da, 3) > 0
        torch.cuda.synchronize()
        _same16(da.cpu().numpy(), d, f"{fmt} time_dot")
        assert plan.time_dot(xd, ya, None, da, 2) > 0
        # refusals before any device work: y and dots keep their bits
        y[:] = 7.0
        dots[:] = -3.0
        xp, yp, wp, dp = x.ctypes.data, y.ctypes.data, wh.ctypes.data, dots.ctypes.data
        dev = sp.X_DEVICE | sp.Y_DEVICE | sp.DOTS_DEVICE
        for args, text in (((xp, yp, wp, None, 0), "dots is NULL"), ((None, yp, wp, dp, 0), "NULL"),
                           ((xp, None, wp, dp, 0), "NULL"), ((xp, yp, wp, dp, 0x200), "flag"),
                           ((xp, yp, wp, dp, 0x20), "flag"), ((xp, yp, wp, dp, 0x40), "flag"),
                           ((xp, yp, wp, dp, sp.Y_STAGED), "Y_STAGED"), ((xp, yp, wp, dp, sp.ASYNC), "ASYNC"),
                           ((xp, yp, wp, dp, sp.ASYNC | sp.X_DEVICE | sp.Y_DEVICE), "ASYNC"),
                           ((xp, yp, wp, dp, sp.ASYNC | dev), "ASYNC"),
                           ((xp, yp, wp, dp, sp.ASYNC | sp.X_DEVICE | sp.Y_DEVICE | sp.W_DEVICE), "ASYNC")):
            assert call(*args) == 1, args
            assert text in L.spmv_last_error().decode(), (args, L.spmv_last_error())
        assert (y == 7.0).all() and (dots == -3.0).all()
        ms = C.c_double(-1.0)
        assert L.spmv_time_dot(h, sp._ptr(xd), sp._ptr(ya), sp._ptr(wd), sp._ptr(da), 0, C.byref(ms)) == 1
        assert L.spmv_time_dot(h, sp._ptr(xd), sp._ptr(ya), sp._ptr(wd), sp._ptr(da), 1, None) == 1
        assert ms.value == -1.0
        # a dot execute clears the mark spmv_fetch_y needs
        yf = np.zeros(m)
        assert L.spmv_execute(h, xp, None, sp.Y_STAGED) == 0
        assert L.spmv_fetch_y(h, yf.ctypes.data) == 0
        _dot(plan, x, w, m)
        assert L.spmv_fetch_y(h, yf.ctypes.data) == 1
        # and leaves the plan what it was
        _assert_bits(_execute(plan, x, m), s, f"{fmt}: execute after the dot executes")
        print(f"dot-routes {name}-{fmt} path={plan.dot_path()}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 8. degenerate shapes
def _small(m, n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, size=m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rp, rng.integers(0, max(n, 1), size=rp[-1]).astype(np.int32), rng.uniform(0.5, 2.0, rp[-1])


@pytest.mark.parametrize("fmt", ["csr", "ell", "dia", "coo", "jds", "bin"])
@pytest.mark.parametrize("m,n,empty", [(0, 5, False), (5, 0, True), (4, 4, True)])
def test_degenerate_shapes(m, n, empty, fmt):
    """m = 0, n = 0, nnz = 0: y = +0.0 and both dots the bits of +0.0 for a finite w."""
    rp, col, val = (np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)) if empty else _small(m, n, 5)
    try:
        plan = sp.Plan.from_csr(m, n, rp, col, val, fmt)
    except sp.SpmvError as e:
        assert "not supported" in str(e), e
        return
    try:
        x = np.full(n, 1.5)
        w = np.array(di.w(8)[:m])
        for wv in (w, None):
            y, d = _dot(plan, x, wv, m, fill=mi.SENTINEL)
            assert di.bits(y).tolist() == [0] * m, y
            assert di.bits(d).tolist() == [0, 0], f"{fmt} {m}x{n}: dots {d!r}"
            if m and n:
                y, d = _dot_dev(plan, _dev(x), None if wv is None else _dev(wv), m, mi.SENTINEL)
                assert di.bits(y).tolist() == [0] * m and di.bits(d).tolist() == [0, 0], (y, d)
        if m:  # no shortcut: w[r] * (+0.0) is computed
            w2 = np.array(w)
            w2[m - 1] = np.inf
            assert np.isnan(_dot(plan, x, w2, m)[1][0])
        assert plan.dot_path() in ("fused", "generic")
    finally:
        plan.destroy()


def test_all_empty_dia_plan():
    """A DIA plan with no stored diagonal: y = +0.0 at both alignments of y,
    the terms computed all the same."""
    import torch
    m = 1000
    plan = sp.Plan.from_csr(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), "dia")
    try:
        assert plan.info()["format"] == "dia" and plan.info()["n_diags"] == 0 and plan.dot_path() == "generic"
        w = np.array(di.w(m))
        xd, wd = torch.ones(m, dtype=torch.float64, device="cuda"), _dev(w)
        y, d = _dot(plan, np.ones(m), w, m, fill=mi.SENTINEL)
        assert di.bits(y).tolist() == [0] * m and di.bits(d).tolist() == [0, 0], d
        for off in (0, 1):
            ybuf, yv = gb.guarded_device(m, off, gb.Y_FILL)
            d = plan.execute_dot(xd, yv, wd)
            torch.cuda.synchronize()
            assert gb.guards_intact(ybuf, m, off, gb.Y_FILL)
            assert di.bits(gb.used(ybuf, m, off)).tolist() == [0] * m and di.bits(d).tolist() == [0, 0], d
        w[m // 2] = -np.inf
        assert np.isnan(_dot(plan, np.ones(m), w, m)[1][0])
    finally:
        plan.destroy()
