"""Plan.execute_axpby (y = alpha * A x + beta * y) on every format and kernel
path: bit for bit expected(plan.execute(x), y0, alpha, beta) -- two rounded
multiplies and one rounded add on the plan's own row sums -- and, whatever
the plan's own execute gives, within the derived bound of
tests/axpby_inputs.py against the extended-precision reference (the only
bound COO is held to).  Then the path each plan takes, beta = 0 never reading
y, guarded offset device buffers, non-finite y0 and x, the host / device /
stream / staged routes, and degenerate shapes.
Needs an MI355X: `pytest -m gpu`.
"""
import ctypes as C

import numpy as np
import pytest

import axpby_inputs as ai
import guarded_buffers as gb
import multi_inputs as mi
import signed_inputs as si
import singlespmv_amd as sp
import special_values as sv

pytestmark = pytest.mark.gpu

# the CONFIGS of tests/test_gpu_signed.py, restated
CONFIGS = (
    [(f"csr-lanes{k}", "csr", {"csr_lanes": k}) for k in (0, 1, 2, 4, 8, 16, 32, 64)]
    + [(f"ss-sigma{k}", "ss", {"ss_sigma": k}) for k in (4, 16, 32, 64)]
    + [("ss", "ss", {}), ("ell", "ell", {}), ("hyb", "hyb", {}), ("hyb-width4", "hyb", {"ell_width": 4}),
       ("jds", "jds", {}), ("jds-width9000", "jds", {"ell_width": 9000}), ("coo", "coo", {}),
       ("css", "css", {}), ("css-shift8", "css", {"css_slab_shift": 8}),
       ("bin", "bin", {}), ("bin-long40", "bin", {"bin_long_len": 40}), ("bin-nolong", "bin", {"bin_long_len": -1}),
       ("bin-order1", "bin", {"bin_product_order": 1}), ("bin-order2", "bin", {"bin_product_order": 2}),
       ("bin-strip1000", "bin", {"bin_strip_cols": 1000}), ("dia", "dia", {}), ("auto", "auto", {})])
SPREAD_TOO = ("csr-lanes0", "ell", "dia", "bin")

CASES = [pytest.param(name, family, fmt, kw, id=f"{name}-{family}-{cid}")
         for name in si.STRUCTURES for cid, fmt, kw in CONFIGS if fmt != "dia" or name == "banded"
         for family in (("cancel", "spread") if cid in SPREAD_TOO else ("cancel",))]

# (structure, configuration) pairs whose builder refuses ("not supported"):
# the refusal is asserted, so no case skips; a pair outside this set that
# refuses fails, and so does a pair inside it that builds
EXPECTED_REFUSALS = set()

AB = (-2.5, 0.75)  # the scalars of the tests that are not about the scalars


def _plan(c, fmt, **kw):
    return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)


def _execute(plan, x, m, alpha=1.0):
    s = np.full(m, np.nan)
    plan.execute(np.ascontiguousarray(x), s, alpha=alpha)
    return s


def _axpby(plan, x, y0, alpha, beta):
    y = np.array(y0, np.float64)
    plan.execute_axpby(np.ascontiguousarray(x), y, alpha, beta)
    return y


def _assert_bits(y, want, what):
    rows = np.flatnonzero(ai.bits(y) != ai.bits(want))
    assert not len(rows), (f"{what}: {len(rows)} rows differ, first {rows[:5].tolist()}: "
                           f"{np.asarray(y)[rows[:3]].tolist()} vs {np.asarray(want)[rows[:3]].tolist()}")


# ---------------------------------------------------------------- 1. every configuration x structure
@pytest.mark.parametrize("name,family,fmt,kw", CASES)
def test_axpby_parity(name, family, fmt, kw, request):
    c = si.case(name, family)
    what = request.node.callspec.id
    cid = what[len(f"{name}-{family}-"):]
    if (name, cid) in EXPECTED_REFUSALS:
        with pytest.raises(sp.SpmvError, match="not supported"):
            _plan(c, fmt, **kw).destroy()
        return
    plan = _plan(c, fmt, **kw)  # any refusal here fails
    try:
        info = plan.info()
        coo = info["format"] == "coo"
        m, rp, ref = c["m"], c["rp"], c["ref"]
        s = _execute(plan, c["x"], m)
        y0 = ai.y0(m)
        worst = 0.0
        for alpha, beta in ai.ALPHA_BETA:
            tag = f"{what} alpha={alpha} beta={beta}"
            y = _axpby(plan, c["x"], y0, alpha, beta)
            y2 = _axpby(plan, c["x"], y0, alpha, beta)
            if not coo:
                _assert_bits(y, ai.expected(s, y0, alpha, beta), f"{tag} vs expected(execute)")
                _assert_bits(y2, y, f"{tag} 2nd call")
            else:
                worst = max(worst, ai.assert_bound(y2, rp, ref, y0, alpha, beta, what + " (2nd call)"))
            if si.plan_is_sequential(info):
                _assert_bits(y, ai.expected(c["y_oracle"], y0, alpha, beta), f"{tag} vs expected(sequential sum)")
            worst = max(worst, ai.assert_bound(y, rp, ref, y0, alpha, beta, what))
        print(f"axpby-parity {what} format={info['format']} path={plan.axpby_path()} err/bound={worst:.3f}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 2. the path reaches what it is here for
CSR_KERNEL = {"staircase": "csr_adaptive_kernel", "powerlaw": "csr_adaptive_kernel", "banded": "csr_slabx_kernel",
              "uniform16": "csr_slab2_kernel"}
FUSED = ([("banded", "dia", {}), ("uniform16", "ell", {}), ("short", "ell", {}), ("uniform16", "jds", {}),
          ("staircase", "jds", {"ell_width": 9000})]
         + [(name, "csr", {"csr_lanes": k, "csr_row_ptr64": bool(rp64)}) for name in CSR_KERNEL
            for k in (0, 1, 2, 4, 8, 16, 32, 64) for rp64 in (0, 1)])
GENERIC = [("powerlaw", "ss", {}), ("staircase", "hyb", {}), ("uniform16", "hyb", {}), ("powerlaw", "coo", {}),
           ("powerlaw", "css", {}), ("powerlaw", "bin", {}), ("uniform16", "bin", {}), ("staircase", "jds", {})]
PATHS = [pytest.param(n, f, kw, "fused", id=f"{n}-{f}-" + "-".join(f"{k}{int(v)}" for k, v in kw.items()))
         for n, f, kw in FUSED] + \
        [pytest.param(n, f, kw, "generic", id=f"{n}-{f}-generic") for n, f, kw in GENERIC]


@pytest.mark.parametrize("name,fmt,kw,path", PATHS)
def test_axpby_path(name, fmt, kw, path):
    c = si.case(name, "cancel")
    plan = _plan(c, fmt, **kw)
    try:
        info = plan.info()
        assert info["format"] == fmt and plan.axpby_path() == path, (info["format"], plan.axpby_path())
        if fmt == "csr":
            if CSR_KERNEL[name] == "csr_adaptive_kernel":  # at lanes 0; a lane count takes the row-group kernels
                assert (info["kernel"] == "csr_adaptive_kernel") == (kw["csr_lanes"] == 0), info["kernel"]
            else:
                assert info["kernel"].startswith(CSR_KERNEL[name]), info["kernel"]
            assert info["row_ptr_bytes"] == (8 if kw["csr_row_ptr64"] else 4)
        if fmt == "jds":
            assert (info["overflow_nnz"] == 0) == (path == "fused"), info["overflow_nnz"]
        s = _execute(plan, c["x"], c["m"])
        y0 = ai.y0(c["m"])
        y = _axpby(plan, c["x"], y0, *AB)
        if fmt != "coo":
            _assert_bits(y, ai.expected(s, y0, *AB), f"{name}-{fmt}-{kw}")
        ai.assert_bound(y, c["rp"], c["ref"], y0, *AB, f"{name}-{fmt}-{kw}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 3. beta = 0 never reads y
@pytest.mark.parametrize("name,fmt", [("banded", "dia"), ("uniform16", "bin")])
def test_beta_zero_never_reads_y(name, fmt):
    import torch
    c = si.case(name, "cancel")
    plan = _plan(c, fmt)
    try:
        assert plan.axpby_path() == ("fused" if fmt == "dia" else "generic")
        xd = torch.from_numpy(np.array(c["x"])).cuda()
        for alpha in (1.0, -2.5):
            want = _execute(plan, c["x"], c["m"], alpha=alpha)
            for beta in (0.0, -0.0):
                for fill in (np.nan, mi.SENTINEL):
                    y = _axpby(plan, c["x"], np.full(c["m"], fill), alpha, beta)
                    _assert_bits(y, want, f"{fmt} host alpha={alpha} beta={beta} fill={fill}")
                    yd = torch.full((c["m"],), fill, dtype=torch.float64, device="cuda")
                    plan.execute_axpby(xd, yd, alpha, beta)
                    _assert_bits(yd.cpu().numpy(), want, f"{fmt} device alpha={alpha} beta={beta} fill={fill}")
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 4. guarded, offset device buffers
GUARDED = [("tri1500", "dia", {}), ("tri5000", "dia", {}), ("uniform16", "csr", {}), ("banded", "csr", {}),
           (gb.STAIR_TAIL, "csr", {"csr_lanes": 0}), ("short", "ell", {}), ("uniform16", "jds", {}),
           ("uniform16", "bin", {}), ("short", "ss", {}), (gb.STAIR_TAIL, "coo", {})]


def _guarded_case(name):
    return mi.case(name, "cancel") if name in mi.TRIDIAGS else gb.case(name)


@pytest.mark.parametrize("name,fmt,kw", [pytest.param(*g, id=f"{g[0]}-{g[1]}") for g in GUARDED])
def test_guarded_offset_buffers(name, fmt, kw):
    """x and y one double into a 16-byte-aligned allocation or at its base:
    both DIA store branches (and both axpby_kernel alignments of the generic
    path), m odd so the last lane / the tail holds one row."""
    import torch
    c = _guarded_case(name)
    m, n = c["m"], c["n"]
    plan = _plan(c, fmt, **kw)
    try:
        info = plan.info()
        assert info["format"] == fmt
        if name in mi.TRIDIAGS:  # LDSX on (window 3513 doubles) and off (10513 > 8192)
            assert m == 12001 and info["n_diags"] == 3
        s = _execute(plan, c["x"], m)
        y0 = ai.y0(m)
        want = ai.expected(s, y0, *AB)
        assert ai.bits(want)[-1] != ai.bits(y0)[-1]
        xh, yh = torch.from_numpy(np.array(c["x"])), torch.from_numpy(np.array(y0))
        for x_off in (0, 1):
            xbuf, xv = gb.guarded_device(n, x_off, gb.X_FILL)
            xv.copy_(xh)
            for y_off in (0, 1):
                what = f"{name}-{fmt} x+{x_off} y+{y_off}"
                ybuf, yv = gb.guarded_device(m, y_off, gb.Y_FILL)
                yv.copy_(yh)
                assert xv.data_ptr() % 16 == 8 * x_off and yv.data_ptr() % 16 == 8 * y_off
                plan.execute_axpby(xv, yv, *AB)
                torch.cuda.synchronize()
                for label, buf, k, off, fill in (("y", ybuf, m, y_off, gb.Y_FILL), ("x", xbuf, n, x_off, gb.X_FILL)):
                    bad = gb.guard_damage(buf, k, off, fill)
                    assert not bad, f"{what}: the {label} guards were written at {bad[:8]}"
                y = gb.used(ybuf, m, y_off)
                if fmt != "coo":
                    _assert_bits(y, want, what)
                else:
                    inside = gb.coo_inside(c["rp"])
                    _assert_bits(y[inside], want[inside], what + " (rows of one unit)")
                assert ai.bits(y)[-1] == ai.bits(want)[-1] or fmt == "coo", f"{what}: the last row was not written"
                ai.assert_bound(y, c["rp"], c["ref"], y0, *AB, what)
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 5. non-finite y0 and x
# one fused plan per kernel family (DIA, sliced ELL, ELL through perm, the
# three CSR kernels), plus BIN
FAMILIES = [("banded", "dia", {}), ("uniform16", "ell", {}), ("uniform16", "jds", {}), ("uniform16", "csr", {}),
            ("banded", "csr", {}), ("powerlaw", "csr", {"csr_lanes": 0}), ("powerlaw", "bin", {})]
FAMILY_IDS = [f"{n}-{f}" + ("-adaptive" if kw else "") for n, f, kw in FAMILIES]


@pytest.mark.parametrize("name,fmt,kw", FAMILIES, ids=FAMILY_IDS)
def test_nonfinite_y0_reaches_its_row_only(name, fmt, kw):
    c = si.case(name, "cancel")
    m = c["m"]
    plan = _plan(c, fmt, **kw)
    try:
        rng = np.random.default_rng(77)
        rows = np.sort(rng.choice(m, 40, replace=False))
        rows[0], rows[-1] = 0, m - 1
        rows = np.unique(rows)
        y0 = np.array(ai.y0(m))
        clean = {ab: _axpby(plan, c["x"], y0, *ab) for ab in ((-2.5, 0.75), (1.0, -1.0))}
        y0[rows] = [sv.POISON[i % 3] for i in range(len(rows))]
        s = _execute(plan, c["x"], m)
        for (alpha, beta), yc in clean.items():
            y = _axpby(plan, c["x"], y0, alpha, beta)
            with np.errstate(invalid="ignore"):
                want = ai.expected(s, y0, alpha, beta)
            assert (sv.classify(want[rows]) != 0).all()
            assert np.array_equal(sv.classify(y), sv.classify(want)), \
                f"{fmt} alpha={alpha} beta={beta}: classes differ on rows {np.flatnonzero(sv.classify(y) != sv.classify(want))[:5]}"
            other = np.ones(m, bool)
            other[rows] = False
            _assert_bits(y[other], yc[other], f"{fmt} alpha={alpha} beta={beta}: rows with a finite y0")
    finally:
        plan.destroy()


@pytest.mark.parametrize("name,fmt,kw", FAMILIES, ids=FAMILY_IDS)
def test_poisoned_x_stays_in_the_layouts_reach(name, fmt, kw):
    c = sv.forward_case(name)
    m, n = c["m"], c["n"]
    plan = _plan(c, fmt, **kw)
    try:
        info = plan.info()
        reached = sv.rows_touching(*sv.reach(info, c["rp"], c["col"], m, n), c["poisoned"]) | c["hit"]
        assert c["hit"].any() and (~reached).any()
        y0 = ai.y0(m)
        y_clean = _axpby(plan, c["x_clean"], y0, 1.0, 0.75)
        y = _axpby(plan, c["x"], y0, 1.0, 0.75)
        assert not np.isfinite(y[c["hit"]]).any(), f"{fmt}: a row that references a poisoned column stayed finite"
        _assert_bits(y[~reached], y_clean[~reached], f"{fmt}: rows out of the poison's reach")
        assert np.isfinite(y_clean).all()
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 6. routes
@pytest.mark.parametrize("name,fmt", [("uniform16", "csr"), ("short", "ss")])
def test_routes(name, fmt):
    import torch
    c = si.case(name, "cancel")
    m, n = c["m"], c["n"]
    L = sp.lib()
    plan = _plan(c, fmt)
    try:
        h = plan._h
        assert plan.axpby_path() == ("fused" if fmt == "csr" else "generic")
        x = np.ascontiguousarray(c["x"])
        y0 = ai.y0(m)
        # SPMV_X_STAGED before any host x was staged: refused, y untouched
        y = np.array(y0)
        assert L.spmv_execute_axpby(h, AB[0], None, AB[1], y.ctypes.data, sp.X_STAGED) == 1
        assert "X_STAGED" in L.spmv_last_error().decode() and np.array_equal(ai.bits(y), ai.bits(y0))
        s = _execute(plan, x, m)
        want = ai.expected(s, y0, *AB)
        # host x and y
        _assert_bits(_axpby(plan, x, y0, *AB), want, f"{fmt} host")
        # SPMV_X_STAGED after a host call (x may be NULL)
        y = np.array(y0)
        assert L.spmv_execute_axpby(h, AB[0], None, AB[1], y.ctypes.data, sp.X_STAGED) == 0, L.spmv_last_error()
        _assert_bits(y, want, f"{fmt} staged x")
        # device x and y on a side stream, async
        xd = torch.from_numpy(x).cuda()
        ya, yb = torch.from_numpy(np.array(y0)).cuda(), torch.from_numpy(np.array(y0)).cuda()
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        plan.set_stream(side)
        try:
            plan.execute_axpby(xd, ya, *AB, async_=True)
            plan.execute_axpby(xd, yb, *AB, async_=True)
            plan.execute_axpby(xd, yb, 1.0, 1.0, async_=True)  # in place on the first call's result
            side.synchronize()
        finally:
            plan.set_stream(None)
        _assert_bits(ya.cpu().numpy(), want, f"{fmt} device async")
        _assert_bits(yb.cpu().numpy(), ai.expected(s, want, 1.0, 1.0), f"{fmt} device async, second update in place")
        # refusals before any device work: y keeps its bits
        y = np.array(y0)
        for args, text in (((AB[0], x.ctypes.data, AB[1], y.ctypes.data, sp.Y_STAGED), "Y_STAGED"),
                           ((AB[0], x.ctypes.data, AB[1], y.ctypes.data, 0x100), "flag"),
                           ((AB[0], None, AB[1], y.ctypes.data, 0), "NULL"),
                           ((AB[0], x.ctypes.data, AB[1], None, 0), "NULL"),
                           ((AB[0], x.ctypes.data, 0.0, y.ctypes.data, sp.Y_STAGED), "Y_STAGED")):
            assert L.spmv_execute_axpby(h, *args) == 1, args
            assert text in L.spmv_last_error().decode(), L.spmv_last_error()
        assert np.array_equal(ai.bits(y), ai.bits(y0))
        # time_axpby: y is updated iters times
        yt = torch.from_numpy(np.array(y0)).cuda()
        assert plan.time_axpby(xd, yt, 1.0, 1.0, 2) > 0
        _assert_bits(yt.cpu().numpy(), ai.expected(s, ai.expected(s, y0, 1.0, 1.0), 1.0, 1.0), f"{fmt} time 2 iterations")
        assert plan.time_axpby(xd, yt, -2.5, 0.0, 2) > 0
        _assert_bits(yt.cpu().numpy(), _execute(plan, x, m, alpha=-2.5), f"{fmt} time, beta = 0")
        # an axpby call clears the mark spmv_fetch_y needs (beta != 0 and beta = 0)
        yf = np.zeros(m)
        for beta in (AB[1], 0.0):
            assert L.spmv_execute(h, x.ctypes.data, None, sp.Y_STAGED) == 0
            assert L.spmv_fetch_y(h, yf.ctypes.data) == 0
            _axpby(plan, x, y0, AB[0], beta)
            assert L.spmv_fetch_y(h, yf.ctypes.data) == 1
        # the scratch of the generic path is counted in device_bytes
        if fmt != "csr":
            assert plan.info()["device_bytes"] >= 8 * m
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 7. degenerate shapes
def _small(m, n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, size=m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rp, rng.integers(0, max(n, 1), size=rp[-1]).astype(np.int32), rng.uniform(0.5, 2.0, rp[-1])


@pytest.mark.parametrize("fmt", ["csr", "ell", "dia", "coo", "jds", "bin"])
@pytest.mark.parametrize("m,n,empty", [(0, 5, False), (5, 0, True), (4, 4, True)])
def test_degenerate_shapes(m, n, empty, fmt):
    """m = 0, n = 0, nnz = 0: y = alpha * (+0.0) + beta * y0, nothing else."""
    import torch
    rp, col, val = (np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0)) if empty else _small(m, n, 5)
    try:
        plan = sp.Plan.from_csr(m, n, rp, col, val, fmt)
    except sp.SpmvError as e:
        assert "not supported" in str(e), e
        return
    try:
        x = np.full(n, 1.5)
        y0 = ai.y0(8)[:m]
        for alpha, beta in ai.ALPHA_BETA:
            want = ai.expected(np.zeros(m), y0, alpha, beta)
            _assert_bits(_axpby(plan, x, y0, alpha, beta), want, f"{fmt} {m}x{n} host alpha={alpha} beta={beta}")
            if m and n:
                yd = torch.from_numpy(np.array(y0)).cuda()
                plan.execute_axpby(torch.from_numpy(x).cuda(), yd, alpha, beta)
                _assert_bits(yd.cpu().numpy(), want, f"{fmt} {m}x{n} device alpha={alpha} beta={beta}")
        assert plan.axpby_path() in ("fused", "generic")
    finally:
        plan.destroy()


def test_all_empty_dia_plan():
    """A DIA plan with no stored diagonal: alpha * (+0.0) + beta * y0 on every
    row, at both alignments of y -- not a memset."""
    import torch
    m = 1000
    plan = sp.Plan.from_csr(m, m, np.zeros(m + 1, np.int64), np.zeros(0, np.int32), np.zeros(0), "dia")
    try:
        assert plan.info()["format"] == "dia" and plan.info()["n_diags"] == 0 and plan.axpby_path() == "fused"
        y0 = ai.y0(m)
        xd = torch.ones(m, dtype=torch.float64, device="cuda")
        for alpha, beta in ai.ALPHA_BETA:
            want = ai.expected(np.zeros(m), y0, alpha, beta)
            _assert_bits(_axpby(plan, np.ones(m), y0, alpha, beta), want, f"host alpha={alpha} beta={beta}")
            for off in (0, 1):
                ybuf, yv = gb.guarded_device(m, off, gb.Y_FILL)
                yv.copy_(torch.from_numpy(np.array(y0)))
                plan.execute_axpby(xd, yv, alpha, beta)
                torch.cuda.synchronize()
                assert gb.guards_intact(ybuf, m, off, gb.Y_FILL)
                _assert_bits(gb.used(ybuf, m, off), want, f"device y+{off} alpha={alpha} beta={beta}")
    finally:
        plan.destroy()
