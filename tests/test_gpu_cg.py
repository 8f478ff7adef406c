"""Plan.cg (spmv_cg_solve: conjugate gradients on a plan, scalars on the
device) on every format: convergence and five fixed iterations against the
NumPy reference of tests/cg_inputs.py, the same bytes whatever check_every,
graph replay and host or device buffers are, p . Ap with the bits of
plan.execute_dot, breakdown, trivial solves, guarded offset buffers, refusals,
a cached graph after a value refresh, and the other entry points around a
solve.  Needs an MI355X: `pytest -m gpu`.
"""
import ctypes as C

import numpy as np
import pytest

import cg_inputs as ci
import guarded_buffers as gb
import singlespmv_amd as sp

pytestmark = pytest.mark.gpu

RTOL = ci.RTOL
SPARSE = [("csr-lanes0", "csr", {"csr_lanes": 0}), ("csr-lanes1", "csr", {"csr_lanes": 1}), ("ell", "ell", {}),
          ("jds", "jds", {}), ("hyb", "hyb", {}), ("ss", "ss", {}), ("coo", "coo", {}), ("css", "css", {}),
          ("bin", "bin", {})]
BANDED = [("dia", "dia", {}), ("csr", "csr", {}), ("ell", "ell", {})]
CONFIGS = {"rand8": SPARSE, "skew": SPARSE, "lap2d": BANDED, "lap1d": BANDED}
CASES = [pytest.param(name, cid, fmt, kw, use_dinv, id=f"{name}-{cid}-{'dinv' if use_dinv else 'plain'}")
         for name, cfgs in CONFIGS.items() for cid, fmt, kw in cfgs for use_dinv in (False, True)]
NOT_COO = [c for c in CASES if c.values[2] != "coo"]

_PLANS = {}


def _plan(name, fmt, kw, scale=1.0):
    """The plan of a case, built once per module (a solve changes nothing a
    later solve can see); scale != 1: a plan of scale * A, the caller's to destroy."""
    c = ci.case(name)
    if scale != 1.0:
        return sp.Plan.from_csr(c["m"], c["m"], c["rp"], c["col"], scale * c["val"], fmt, **kw)
    key = (name, fmt, tuple(sorted(kw.items())))
    if key not in _PLANS:
        _PLANS[key] = sp.Plan.from_csr(c["m"], c["m"], c["rp"], c["col"], c["val"], fmt, **kw)
        assert _PLANS[key].info()["format"] == fmt
    return _PLANS[key]


@pytest.fixture(scope="module", autouse=True)
def _destroy_plans():
    yield
    for plan in _PLANS.values():
        plan.destroy()
    _PLANS.clear()


def _dinv(c, use_dinv):
    return np.array(c["dinv"]) if use_dinv else None


def _solve(plan, c, use_dinv, x0=None, b=None, **kw):
    """(x, info) through host buffers from the case's x0."""
    x = np.array(c["x0"] if x0 is None else x0)
    info = plan.cg(np.array(c["b"] if b is None else b), x, _dinv(c, use_dinv), **kw)
    return x, info


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, np.float64)).cuda()


def _solve_dev(plan, c, use_dinv, **kw):
    xd = _dev(c["x0"])
    info = plan.cg(_dev(c["b"]), xd, _dev(_dinv(c, use_dinv)), **kw)
    return xd.cpu().numpy(), info


def _key(x, info):
    """x and info as bit patterns."""
    return (ci.bits(x).tobytes(), info["status"], info["iterations"],
            tuple(ci.bits([info[k] for k in ("rr", "bb", "rz", "pq")]).tolist()))


def _assert_same(got, want, what):
    (x, info), (x_w, info_w) = got, want
    assert _key(x, info)[1:] == _key(x_w, info_w)[1:], f"{what}: info {info} vs {info_w}"
    rows = np.flatnonzero(ci.bits(x) != ci.bits(x_w))
    assert not len(rows), f"{what}: {len(rows)} entries of x differ, first {rows[:5].tolist()}"


# ---------------------------------------------------------------- 1. convergence
@pytest.mark.parametrize("name,cid,fmt,kw,use_dinv", CASES)
def test_convergence(name, cid, fmt, kw, use_dinv):
    c, ref = ci.case(name), ci.reference(name, use_dinv)
    x, info = _solve(_plan(name, fmt, kw), c, use_dinv, rtol=RTOL, max_iters=2 * ref["ref_iters"])
    relres = ci.true_relres(c, x, c["b"])
    print(f"cg-conv {name} {cid} dinv={int(use_dinv)} iters={info['iterations']} ref_iters={ref['ref_iters']} "
          f"recurred={np.sqrt(info['rr'] / info['bb']):.3e} true={relres:.3e}")
    assert info["status"] == "converged", info
    assert 0 < info["iterations"] <= 2 * ref["ref_iters"]
    assert np.sqrt(info["rr"] / info["bb"]) <= RTOL
    assert relres <= 2 * RTOL
    if not use_dinv:
        assert ci.bits([info["rz"]])[0] == ci.bits([info["rr"]])[0], "without dinv rz is rr"


# ---------------------------------------------------------------- 2. five fixed iterations
@pytest.mark.parametrize("name,cid,fmt,kw,use_dinv", CASES)
def test_five_iterations(name, cid, fmt, kw, use_dinv):
    """The distance from the longdouble iterate, measured by the float64
    reference's own (d_ref): a plan's row sums and dots add in another order
    than NumPy's, and five steps compound it -- at most 16 d_ref.

    Measured on the MI355X (worst ratio per format over the cases and both
    dinv settings) -- see DESIGN.md §3.12."""
    c, ref = ci.case(name), ci.reference(name, use_dinv)
    x, info = _solve(_plan(name, fmt, kw), c, use_dinv, rtol=0.0, max_iters=ci.FIXED)
    dist = ci.rel_distance(x, ref["x5"])
    print(f"cg-five {name} {cid} dinv={int(use_dinv)} dist={dist:.3e} d_ref={ref['d_ref']:.3e} "
          f"ratio={dist / ref['d_ref']:.3g}")
    assert info["status"] == "max_iters" and info["iterations"] == ci.FIXED, info
    assert dist <= 16 * ref["d_ref"]


# ---------------------------------------------------------------- 3. same bytes
@pytest.mark.parametrize("name,cid,fmt,kw,use_dinv", NOT_COO)
def test_same_bytes(name, cid, fmt, kw, use_dinv):
    """x and info are a function of the plan, b, x0, dinv, rtol and max_iters:
    not of the call, of check_every, of graph replay, of host or device
    buffers.  Once to convergence (done falls inside a check interval) and once
    with a max_iters that is no multiple of any check_every."""
    c, ref = ci.case(name), ci.reference(name, use_dinv)
    plan = _plan(name, fmt, kw)
    for rtol, max_iters in ((RTOL, 2 * ref["ref_iters"]), (0.0, 7)):
        what = f"{name}-{cid} dinv={int(use_dinv)} max_iters={max_iters}"
        base = _solve(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=8)
        assert base[1]["status"] == ("converged" if rtol else "max_iters") and base[1]["iterations"] > 0
        _assert_same(_solve(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=8), base, f"{what}: again")
        for every in (1, 3, 64):
            _assert_same(_solve(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=every), base,
                         f"{what}: check_every={every}")
        _assert_same(_solve_dev(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=8), base,
                     f"{what}: device buffers")
        if fmt == "css":
            continue
        for every in (8, 3):
            _assert_same(_solve(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=every, graph=True),
                         base, f"{what}: graph, check_every={every}")
        _assert_same(_solve_dev(plan, c, use_dinv, rtol=rtol, max_iters=max_iters, check_every=3, graph=True), base,
                     f"{what}: graph, device buffers")


# ---------------------------------------------------------------- 4. built from the plan's own kernels
@pytest.mark.parametrize("name,cid,fmt,kw", [pytest.param(n, cid, f, kw, id=f"{n}-{cid}")
                                             for n, cfgs in CONFIGS.items() for cid, f, kw in cfgs])
def test_pq_has_the_bits_of_execute_dot(name, cid, fmt, kw):
    """x0 = 0, no dinv: r = b - A 0 = b, p = b, so the first p . Ap is
    plan.execute_dot(b, q, w=b)'s dots[0], bit for bit.  COO (unordered
    atomics in q): within the bound of a row's sum (len + 8 roundings of its
    magnitude, signed_inputs.row_tol's shape) carried through the dot
    (m + 8 more), for both q."""
    c = ci.case(name)
    plan = _plan(name, fmt, kw)
    m, b = c["m"], np.array(c["b"])
    x, info = _solve(plan, c, False, x0=np.zeros(m), rtol=0.0, max_iters=1)
    assert info["status"] == "max_iters" and info["iterations"] == 1
    q = np.full(m, np.nan)
    wy, _ = plan.execute_dot(b, q, b)
    assert plan.cg_path() == (5 if plan.dot_path() == "fused" else plan.info()["n_kernels"] + 5)
    if fmt != "coo":
        assert ci.bits([info["pq"]])[0] == ci.bits([wy])[0], f"pq {info['pq']!r} vs execute_dot's {wy!r}"
        # ... and the x of one step is alpha * b with alpha = (b . b) / pq
        alpha = info["bb"] / info["pq"]
        assert np.array_equal(ci.bits(x), ci.bits(0.0 + alpha * b))
        return
    mag = np.zeros(m)
    np.add.at(mag, c["row"], np.abs(c["val"] * b[c["col"]]))
    u = 2.0 ** -53
    bound = 2 * u * (np.diff(c["rp"]).max() + 8 + m + 8) * float(np.sum(np.abs(b) * mag))
    assert abs(info["pq"] - wy) <= bound, (info["pq"], wy, bound)


# ---------------------------------------------------------------- 5. breakdown
@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("ell", {}), ("bin", {}), ("coo", {})], ids=lambda v: v if isinstance(v, str) else "")
def test_breakdown(fmt, kw):
    c = ci.case("rand8")
    neg = _plan("rand8", fmt, kw, scale=-1.0)
    try:
        for every in (1, 64):
            x, info = _solve(neg, c, False, rtol=RTOL, max_iters=50, check_every=every)
            assert info["status"] == "breakdown" and info["iterations"] == 0 and info["pq"] < 0, info
            assert np.array_equal(ci.bits(x), ci.bits(c["x0"])), "x moved in an iteration that broke down"
    finally:
        neg.destroy()
    b = np.array(c["b"])
    b[1234] = np.nan
    plan = _plan("rand8", fmt, kw)
    for graph in (False, True):
        x, info = _solve(plan, c, True, b=b, rtol=RTOL, max_iters=50, check_every=64, graph=graph)
        assert info["status"] == "breakdown" and info["iterations"] == 0 and np.isnan(info["pq"]), info
        assert np.array_equal(ci.bits(x), ci.bits(c["x0"]))


# ---------------------------------------------------------------- 6. trivial solves
@pytest.mark.parametrize("fmt", ["csr", "ell", "dia", "bin"])
def test_zero_rhs_and_init_only(fmt):
    c = ci.case("lap1d")
    plan = _plan("lap1d", fmt, {})
    m = c["m"]
    x, info = _solve(plan, c, False, x0=np.zeros(m), b=np.zeros(m), rtol=RTOL, max_iters=10)
    assert info["status"] == "converged" and info["iterations"] == 0, info
    assert not ci.bits(x).any(), "x is not all +0.0"
    assert ci.bits([info["rr"], info["bb"], info["rz"], info["pq"]]).tolist() == [0, 0, 0, 0]
    # max_iters = 0: the init only -- rr of b - A x0, x as it was
    for use_dinv in (False, True):
        x, info = _solve(plan, c, use_dinv, rtol=RTOL, max_iters=0)
        _, want = ci.ref_cg(c, c["b"], c["x0"], _dinv(c, use_dinv), RTOL, 0)
        assert info["status"] == "max_iters" and info["iterations"] == 0 and ci.bits([info["pq"]])[0] == 0, info
        assert np.array_equal(ci.bits(x), ci.bits(c["x0"]))
        for k in ("rr", "bb", "rz"):  # m roundings of positive terms, either order
            assert abs(info[k] - want[k]) <= 2 * (m + 8) * 2.0 ** -53 * want[k], (k, info[k], want[k])
    # ... and converged at entry: x0 = the solution
    xs, _ = ci.ref_cg(c, c["b"], c["x0"], None, 1e-13, 1000)
    x, info = _solve(plan, c, False, x0=xs, rtol=1e-6, max_iters=10)
    assert info["status"] == "converged" and info["iterations"] == 0 and np.array_equal(ci.bits(x), ci.bits(xs))


@pytest.mark.parametrize("name", ["tiny1", "tiny65", "tiny130"])
@pytest.mark.parametrize("fmt", ["csr", "ell", "dia", "coo", "bin", "css"])
def test_tiny(name, fmt):
    c = ci.case(name)
    plan = _plan(name, fmt, {})
    for use_dinv in (False, True):
        ref = ci.reference(name, use_dinv)
        for dev in (False, True):
            x, info = (_solve_dev if dev else _solve)(plan, c, use_dinv, rtol=RTOL, max_iters=2 * ref["ref_iters"] + 1)
            assert info["status"] == "converged" and info["iterations"] >= 1, info
            assert ci.true_relres(c, x, c["b"]) <= 2 * RTOL


def test_empty_plan():
    plan = sp.Plan.from_csr(0, 0, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0), "csr")
    try:
        info = plan.cg(np.zeros(0), np.zeros(0), None)
        assert info == {"status": "converged", "iterations": 0, "rr": 0.0, "bb": 0.0, "rz": 0.0, "pq": 0.0}
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 7. buffer contract
@pytest.mark.parametrize("name,fmt", [("rand8", "csr"), ("lap1d", "dia"), ("skew", "bin"), ("tiny130", "ell")])
def test_guarded_offset_buffers(name, fmt):
    """b, x and dinv in guarded device buffers, x at a 16-byte boundary or 8
    bytes past one, b and dinv likewise: the guards of x are untouched, b and
    dinv unchanged (their guards hold NaN: one read past either end reaches a
    dot product), and x and info do not depend on the alignment."""
    import torch
    c = ci.case(name)
    m = c["m"]
    plan = _plan(name, fmt, {})
    base = _solve(plan, c, True, rtol=0.0, max_iters=6, check_every=4)
    for x_off in (0, 1):
        for bd_off in (0, 1):
            what = f"{name}-{fmt} x+{x_off} b,dinv+{bd_off}"
            xbuf, xv = gb.guarded_device(m, x_off, gb.Y_FILL)
            bbuf, bv = gb.guarded_device(m, bd_off, float("nan"))
            dbuf, dv = gb.guarded_device(m, bd_off, float("nan"))
            xv.copy_(torch.from_numpy(np.array(c["x0"])))
            bv.copy_(torch.from_numpy(np.array(c["b"])))
            dv.copy_(torch.from_numpy(np.array(c["dinv"])))
            assert xv.data_ptr() % 16 == 8 * x_off and bv.data_ptr() % 16 == 8 * bd_off == dv.data_ptr() % 16
            for graph in (False, True):
                xv.copy_(torch.from_numpy(np.array(c["x0"])))
                info = plan.cg(bv, xv, dv, rtol=0.0, max_iters=6, check_every=4, graph=graph)
                torch.cuda.synchronize()
                for label, buf, off, fill in (("x", xbuf, x_off, gb.Y_FILL), ("b", bbuf, bd_off, float("nan")),
                                              ("dinv", dbuf, bd_off, float("nan"))):
                    bad = gb.guard_damage(buf, m, off, fill)
                    assert not bad, f"{what}: the {label} guards were written at {bad[:8]}"
                assert np.array_equal(ci.bits(gb.used(bbuf, m, bd_off)), ci.bits(c["b"])), f"{what}: b changed"
                assert np.array_equal(ci.bits(gb.used(dbuf, m, bd_off)), ci.bits(c["dinv"])), f"{what}: dinv changed"
                _assert_same((gb.used(xbuf, m, x_off), info), base, f"{what} graph={graph}")


# ---------------------------------------------------------------- 8. refusals
def _raw(plan, b, x, dinv, rtol, max_iters, every, flags, info):
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    st = sp.lib().spmv_cg_solve(plan._h, ptr(b), ptr(x), ptr(dinv), rtol, max_iters, every, flags,
                                None if info is None else C.byref(info))
    return st, sp.lib().spmv_last_error().decode()


def test_refusals():
    import torch
    c = ci.case("tiny65")
    m = c["m"]
    plan = _plan("tiny65", "csr", {})
    b, x = np.array(c["b"]), np.full(m, 7.0)
    info = sp.CgInfo(-5, -6, -1.0, -2.0, -3.0, -4.0)
    bytes0 = plan.info()["device_bytes"]
    for args, word in (((b, x, None, 1e-8, 10, 1, 0, None), "info is NULL"),
                       ((None, x, None, 1e-8, 10, 1, 0, info), "b or x is NULL"),
                       ((b, None, None, 1e-8, 10, 1, 0, info), "b or x is NULL"),
                       ((b, x, None, 1e-8, -1, 1, 0, info), "max_iters < 0"),
                       ((b, x, None, 1e-8, 10, 0, 0, info), "check_every < 1"),
                       ((b, x, None, -1e-8, 10, 1, 0, info), "rtol is negative or NaN"),
                       ((b, x, None, float("nan"), 10, 1, 0, info), "rtol is negative or NaN")) + tuple(
            ((b, x, None, 1e-8, 10, 1, f, info), "unknown flag bits")
            for f in (sp.X_DEVICE, sp.Y_DEVICE, sp.ASYNC, sp.X_STAGED, sp.Y_STAGED, sp.W_DEVICE, sp.DOTS_DEVICE,
                      sp.CSR_DEVICE, sp.VAL_DEVICE, 0x800, sp.CG_GRAPH | 0x80000000)):
        st, err = _raw(plan, *args)
        assert st == 1 and word in err, (args[3:], st, err)
    assert (x == 7.0).all() and info.status == -5 and info.pq == -4.0
    assert plan.info()["device_bytes"] == bytes0, "a refused solve allocated"
    # host pointers under SPMV_CG_DEVICE are refused before any device work
    st, err = _raw(plan, b, x, None, 1e-8, 10, 1, sp.CG_DEVICE, info)
    assert st == 1 and "SPMV_CG_DEVICE needs device memory" in err and (x == 7.0).all()
    # host and device buffers mixed: refused in Python
    with pytest.raises(ValueError, match="must all be numpy arrays"):
        plan.cg(b, torch.zeros(m, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="must all be numpy arrays"):
        plan.cg(b, x, torch.ones(m, dtype=torch.float64, device="cuda"))
    assert (x == 7.0).all()


def test_a_plan_that_is_not_square():
    rp = np.arange(8, dtype=np.int64) * 2
    col = np.tile(np.array([3, 900], np.int32), 7)
    plan = sp.Plan.from_csr(7, 1000, rp, col, np.ones(14), "csr")
    try:
        x = np.full(1000, 7.0)
        with pytest.raises(sp.SpmvError, match="invalid value.*not square"):
            plan.cg(np.ones(1000), x)
        assert (x == 7.0).all()
    finally:
        plan.destroy()


def test_css_refuses_the_graph():
    c = ci.case("rand8")
    plan = _plan("rand8", "css", {})
    x = np.array(c["x0"])
    for buffers in (lambda a: a, _dev):
        xb = buffers(x)
        with pytest.raises(sp.SpmvError, match="not supported.*CSS"):
            plan.cg(buffers(np.array(c["b"])), xb, graph=True)
        assert np.array_equal(ci.bits(gb.to_host(xb)), ci.bits(c["x0"]))


# ---------------------------------------------------------------- 9. value refresh with a cached graph
@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("bin", {})], ids=["csr", "bin"])
def test_cached_graph_replays_refreshed_values(fmt, kw):
    """2 A x = b from x0 = 0 is half the solution of A x = b, step for step
    (every product with the doubled values is exact), with the same dinv
    tensor: a graph that replayed the old values would miss it by a factor 2."""
    c = ci.case("rand8")
    plan = sp.Plan.from_csr(c["m"], c["m"], c["rp"], c["col"], c["val"], fmt, **kw)
    try:
        bd, xd, dd = _dev(c["b"]), _dev(np.zeros(c["m"])), _dev(c["dinv"])
        first = plan.cg(bd, xd, dd, rtol=RTOL, max_iters=100, check_every=4, graph=True)
        x1 = xd.cpu().numpy()
        assert first["status"] == "converged"
        plan.prepare_update(c["rp"], c["col"])
        plan.update_values(2.0 * c["val"])
        xd.zero_()
        second = plan.cg(bd, xd, dd, rtol=RTOL, max_iters=100, check_every=4, graph=True)
        x2 = xd.cpu().numpy()
        bytes2 = plan.info()["device_bytes"]
        assert second["status"] == "converged" and second["iterations"] == first["iterations"]
        assert (np.abs(x2 - 0.5 * x1) <= 4 * 2.0 ** -53 * np.abs(0.5 * x1)).all()
        xd.zero_()
        third = plan.cg(bd, xd, dd, rtol=RTOL, max_iters=100, check_every=4, graph=True)
        _assert_same((xd.cpu().numpy(), third), (x2, second), "the third solve")
        assert plan.info()["device_bytes"] == bytes2, "the cached graph's solve allocated again"
    finally:
        plan.destroy()


# ---------------------------------------------------------------- 10. the other entry points
@pytest.mark.parametrize("name,fmt,kw", [("rand8", "csr", {}), ("skew", "hyb", {}), ("skew", "bin", {}),
                                         ("lap2d", "dia", {}), ("rand8", "ss", {})],
                         ids=lambda v: v if isinstance(v, str) else "")
def test_other_entry_points_around_a_solve(name, fmt, kw):
    c = ci.case(name)
    m = c["m"]
    plan = sp.Plan.from_csr(m, m, c["rp"], c["col"], c["val"], fmt, **kw)
    try:
        v, w = np.array(c["x0"]), np.array(c["b"])

        def others():
            y = np.full(m, np.nan)
            plan.execute(v, y)
            y2 = np.full(m, np.nan)
            d = plan.execute_dot(v, y2, w)
            y3 = np.array(w)
            plan.execute_axpby(v, y3, alpha=-1.0, beta=0.5)
            return np.concatenate([y, y2, y3, d])

        before = others()
        x1, info1 = _solve(plan, c, True, rtol=RTOL, max_iters=200)
        between = others()
        x2, info2 = _solve(plan, c, True, rtol=RTOL, max_iters=200, graph=True, check_every=5)
        after = others()
        assert np.array_equal(ci.bits(before), ci.bits(between)) and np.array_equal(ci.bits(before), ci.bits(after))
        _assert_same((x2, info2), (x1, info1), f"{name}-{fmt}: the solve after the other entry points")
        # the solve clears the mark spmv_fetch_y needs, like any non-staged execute
        st = sp.lib().spmv_fetch_y(plan._h, np.zeros(m).ctypes.data)
        assert st == 1 and "spmv_fetch_y without a previous SPMV_Y_STAGED execute" in sp.lib().spmv_last_error().decode()
    finally:
        plan.destroy()
