"""The transpose on the GPU: spmv_csr_transpose_device against the host
function byte for byte, and plans of the transpose (Plan.from_device_csr /
Plan.from_csr with transpose=True) against the plan of the host-transposed
CSR, array by array (spmv_plan_digest) and y bit for bit, on every route a
plan has: execute, axpby, multi, graph, value refresh.  No tolerance of its
own: bytes against bytes, or signed_inputs' row_tol.
Needs an MI355X: `pytest -m gpu`.
"""
import ctypes as C

import numpy as np
import pytest

import signed_inputs as si
import singlespmv_amd as sp
import transpose_inputs as ti
from test_gpu_signed import CASES, CONFIGS, _check_y, _execute_twice

pytestmark = pytest.mark.gpu

INVALID = 1
ONE_PER_FORMAT = [("csr", {}), ("ss", {}), ("ell", {}), ("hyb", {}), ("jds", {}), ("coo", {}), ("css", {}),
                  ("bin", {}), ("auto", {})]
# (structure, format): one config per format on staircase, DIA (and the rest again) on banded
PER_FORMAT_CASES = ([pytest.param("staircase", f, kw, id=f"staircase-{f}") for f, kw in ONE_PER_FORMAT]
                    + [pytest.param("banded", f, kw, id=f"banded-{f}") for f, kw in ONE_PER_FORMAT + [("dia", {})]])
REFRESH_CASES = ([pytest.param("staircase", f, kw, id=f"staircase-{f}") for f, kw in ONE_PER_FORMAT]
                 + [pytest.param("banded", "dia", {}, id="banded-dia")])


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().tensor(np.asarray(a)).cuda()  # a copy: the shared fixtures are read-only


def _host(t):
    return None if t is None else t.cpu().numpy()


def _same_layout(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, f"{what}: arrays {bad} differ from the plan of the host-transposed CSR"


def _same_info(a, b, what, keys=("format", "kernel", "m", "n", "nnz", "device_bytes")):
    for k in keys:
        assert a[k] == b[k], f"{what}: info[{k}] {a[k]} vs {b[k]}"


def _companion(m, n, rp, col, val, fmt, kw):
    """The ordinary plan of an (already transposed) CSR, built on the device;
    skips where the builder itself refuses the configuration."""
    try:
        return sp.Plan.from_device_csr(m, n, _dev(rp), _dev(col), _dev(val), fmt, **kw)
    except sp.SpmvError as e:
        if "not supported" in str(e):
            pytest.skip(f"the builder refuses this configuration: {e}")
        raise


def _transposed(t, fmt, kw, val=None):
    return sp.Plan.from_device_csr(t["m"], t["n"], _dev(t["rp"]), _dev(t["col"]),
                                   _dev(t["val"] if val is None else val), fmt, transpose=True, **kw)


# ---- 1. the device transposition ----------------------------------------------
def _inputs():
    for name in si.STRUCTURES:
        yield pytest.param(("structure", name), id=name)
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
def test_device_transposition_equals_host(key):
    m, n, rp, col, val = _load(key)
    want = sp.csr_transpose(m, n, rp, col, val, perm=True)
    d = (_dev(rp), _dev(col), _dev(val))
    got = sp.csr_transpose(m, n, *d, perm=True)
    assert all(t.is_cuda for t in got)
    ti.assert_same_csr([_host(t) for t in got], want, f"{key}")
    again = sp.csr_transpose(m, n, *d, perm=True)
    ti.assert_same_csr([_host(t) for t in again], want, f"{key} (second call)")
    for t, h, name in zip(d, (rp, col, val), ("row_ptr", "col", "val")):
        same = np.array_equal(ti.bits(_host(t)), ti.bits(h)) if name == "val" else np.array_equal(_host(t), h)
        assert same, f"{key}: the input {name} was written"
    # the pattern alone, and without perm
    pat = sp.csr_transpose(m, n, d[0], d[1])
    ti.assert_same_csr([_host(t) for t in pat], (want[0], want[1], None), f"{key} pattern only")
    ti.assert_same_csr([_host(t) for t in sp.csr_transpose(m, n, *d)], want[:3], f"{key} without perm")


@pytest.mark.parametrize("name", ["col-eq-n", "col-negative", "row_ptr-decreasing"])
def test_device_transposition_refusals(name):
    """validate_csr_device's refusal, before any kernel indexes by a column: outputs untouched."""
    torch = _torch()
    m, n, nnz, rp, col = ti.refused()[name]
    d_rp, d_col, d_val = _dev(rp), _dev(col), _dev(np.arange(1.0, nnz + 1))
    t_rp = torch.full((n + 1,), -77, dtype=torch.int64, device="cuda")
    t_col = torch.full((nnz,), -77, dtype=torch.int32, device="cuda")
    t_val = torch.full((nnz,), -77.0, dtype=torch.float64, device="cuda")
    perm = torch.full((nnz,), -77, dtype=torch.int64, device="cuda")
    st = sp.lib().spmv_csr_transpose_device(0, m, n, nnz, d_rp.data_ptr(), d_col.data_ptr(), d_val.data_ptr(),
                                            t_rp.data_ptr(), t_col.data_ptr(), t_val.data_ptr(), perm.data_ptr())
    torch.cuda.synchronize()
    assert st == INVALID, (name, st, sp.lib().spmv_last_error().decode())
    for t in (t_rp, t_col, t_val, perm):
        assert bool((t == -77).all()), f"{name}: an output was written"
    with pytest.raises(sp.SpmvError, match="invalid value"):
        sp.Plan.from_device_csr(m, n, d_rp, d_col, d_val, "csr", transpose=True)


# ---- 2. plans of the transpose: A := the twin, so A^T is the case itself ------------------
@pytest.mark.parametrize("name,family,fmt,kw", CASES)
def test_transposed_plan_is_the_companion(name, family, fmt, kw, request):
    t = ti.twin(name, family)
    c = t["case"]
    what = request.node.callspec.id
    comp = _companion(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, kw)
    plan = _transposed(t, fmt, kw)
    assert plan.transposed and not comp.transposed
    assert (plan.m, plan.n) == (c["m"], c["n"]) == (t["n"], t["m"])
    _same_layout(plan.digest(), comp.digest(), what)
    _same_info(plan.info(), comp.info(), what)
    assert plan.built_on_device() == comp.built_on_device()
    ya, yb = _execute_twice(plan, c)
    worst = _check_y(plan, c, ya, yb, what)
    yc, _ = _execute_twice(comp, c)
    if plan.info()["format"] != "coo":  # (COO's unordered atomics: _check_y's rule)
        assert np.array_equal(ya, yc), f"{what}: y differs from the companion's"
    print(f"transposed-parity {what} format={plan.info()['format']} err/row_tol={worst:.3f}")
    plan.destroy()
    comp.destroy()


# ---- 3. the other direction: A := the structure, A^T is new ground ----------------------
@pytest.mark.parametrize("fmt", ["csr", "ell", "bin", "coo", "ss", "auto"])
@pytest.mark.parametrize("family", sorted(si.FAMILIES))
@pytest.mark.parametrize("name", si.STRUCTURES)
def test_transposed_structures(name, family, fmt):
    m, n, rp, col = si.structure(name)
    t_rp, t_col, _, perm = ti.np_transpose(m, n, rp, col)
    # values drawn on the transposed pattern, carried back into A's entry order
    t_val, x = si.FAMILIES[family](t_rp, t_col, m, seed=100 + si.STRUCTURES.index(name))
    val = np.empty(len(col))
    val[perm] = t_val
    what = f"{name}^T-{family}-{fmt}"
    comp = _companion(n, m, t_rp, t_col, t_val, fmt, {})
    plan = sp.Plan.from_device_csr(m, n, _dev(rp), _dev(col), _dev(val), fmt, transpose=True)
    assert (plan.m, plan.n) == (n, m) and plan.transposed
    _same_layout(plan.digest(), comp.digest(), what)
    _same_info(plan.info(), comp.info(), what)
    ya, yb = np.full(n, np.nan), np.full(n, -1.2345e300)
    plan.execute(x, ya)
    plan.execute(x, yb)
    ref = si.ref_rows(t_rp, t_col, t_val, x)
    si.assert_rows(ya, t_rp, t_col, t_val, x, what, ref=ref)
    si.assert_rows(yb, t_rp, t_col, t_val, x, what + " (2nd execute)", ref=ref)
    if plan.info()["format"] != "coo":
        yc = np.full(n, np.nan)
        comp.execute(x, yc)
        assert np.array_equal(ya, yb) and np.array_equal(ya, yc), f"{what}: y differs from the companion's"
    plan.destroy()
    comp.destroy()


# ---- 4. host arrays, both build routes ------------------------------------------------
@pytest.mark.parametrize("name,fmt,kw", PER_FORMAT_CASES)
def test_host_arrays_both_routes(name, fmt, kw):
    t = ti.twin(name, "cancel")
    c = t["case"]
    comp = _companion(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, kw)
    for build in ("host", "device"):
        plan = sp.Plan.from_csr(t["m"], t["n"], t["rp"], t["col"], t["val"], fmt, transpose=True, build=build, **kw)
        what = f"{name}-{fmt} build={build}"
        assert plan.transposed and plan.built_on_device() == (build == "device"), what
        _same_layout(plan.digest(), comp.digest(), what)
        _same_info(plan.info(), comp.info(), what, keys=("format", "kernel", "m", "n", "nnz"))
        ya, yb = _execute_twice(plan, c)
        _check_y(plan, c, ya, yb, what)
        plan.destroy()
    comp.destroy()


# ---- 5. every route on a transposed plan ----------------------------------------------
@pytest.mark.parametrize("name,fmt", [("staircase", "csr"), ("banded", "dia"), ("staircase", "bin")])
def test_routes_equal_the_companion(name, fmt):
    torch = _torch()
    t = ti.twin(name, "spread")
    c = t["case"]
    m, n = c["m"], c["n"]
    comp = _companion(m, n, c["rp"], c["col"], c["val"], fmt, {})
    plan = _transposed(t, fmt, {})
    rng = np.random.default_rng(31)
    y0 = rng.standard_normal(m)
    X = np.ascontiguousarray(rng.standard_normal((n, 3)))
    out = {}
    for key, p in (("plan", plan), ("comp", comp)):
        y = y0.copy()
        p.execute_axpby(c["x"], y, alpha=-2.5, beta=0.75)
        Y = np.full((m, 3), np.nan)
        p.execute_multi(X, Y)
        xd = _dev(c["x"])
        yd = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
        g = p.graph(xd, yd)
        g.launch()
        torch.cuda.synchronize()
        yg = yd.cpu().numpy()
        g.destroy()
        out[key] = (y, Y, yg, p.axpby_path(), p.multi_path(X, Y))
    a, b = out["plan"], out["comp"]
    assert a[3] == b[3] and a[4] == b[4], (a[3:], b[3:])
    for k, route in enumerate(("execute_axpby", "execute_multi", "graph")):
        assert np.array_equal(a[k], b[k]), f"{name}-{fmt}: {route} differs from the companion's"
    ye, _ = _execute_twice(plan, c)
    assert np.array_equal(a[2], ye), "the graph replay differs from execute"
    si.assert_rows(ye, c["rp"], c["col"], c["val"], c["x"], f"{name}-{fmt}", ref=c["ref"])
    plan.destroy()
    comp.destroy()


# ---- 6. value refresh: the CSR the plan was created from is A's ---------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,fmt,kw", REFRESH_CASES)
def test_refresh_in_source_order(name, fmt, kw, device):
    t0, t1 = ti.twin(name, "spread"), ti.twin(name, "cancel")
    c1 = t1["case"]
    assert np.array_equal(t0["rp"], t1["rp"]) and np.array_equal(t0["col"], t1["col"])
    what = f"{name}-{fmt} {'device' if device else 'host'} arrays"
    plan = _transposed(t0, fmt, kw)
    fresh = _transposed(t1, fmt, kw)
    # A^T's pattern in place of A's: refused, and the plan stays usable (a
    # symmetric pattern, the full band, is its own transpose: nothing to refuse)
    symmetric = np.array_equal(c1["rp"], t0["rp"]) and np.array_equal(c1["col"], t0["col"])
    assert symmetric == (name == "banded")
    if not symmetric:
        with pytest.raises(sp.SpmvError, match="invalid value"):
            if device:
                plan.prepare_update(_dev(c1["rp"]), _dev(c1["col"]))
            else:
                plan.prepare_update(c1["rp"], c1["col"])
    y0, _ = _execute_twice(plan, t0["case"])
    si.assert_rows(y0, c1["rp"], c1["col"], t0["case"]["val"], t0["case"]["x"], what + " after the refusal",
                   ref=t0["case"]["ref"])
    if device:
        plan.prepare_update(_dev(t0["rp"]), _dev(t0["col"]))
        plan.update_values(_dev(t1["val"]))
    else:
        plan.prepare_update(t0["rp"], t0["col"])
        plan.update_values(np.ascontiguousarray(t1["val"]))
    _same_layout(plan.digest(), fresh.digest(), what + " after update_values")
    ya, yb = _execute_twice(plan, c1)
    _check_y(plan, c1, ya, yb, what)
    yf, _ = _execute_twice(fresh, c1)
    if plan.info()["format"] != "coo":
        assert np.array_equal(ya, yf), f"{what}: y differs from the fresh build's"
    plan.destroy()
    fresh.destroy()


# ---- 7. shapes --------------------------------------------------------------------------
def test_shape_checks_use_the_swapped_shape():
    t = ti.twin("rect513x40", "spread")  # A is 40 x 513
    c = t["case"]
    plan = _transposed(t, "csr", {})
    comp = _companion(c["m"], c["n"], c["rp"], c["col"], c["val"], "csr", {})
    assert plan.transposed is True and comp.transposed is False
    assert (plan.m, plan.n) == (513, 40) and (t["m"], t["n"]) == (40, 513)
    with pytest.raises(ValueError, match="y holds 40"):  # y of length m_A
        plan.execute(np.ones(40), np.zeros(40))
    plan.execute(np.ones(40), np.zeros(513))
    # A := the structure itself (513 x 40): x of length n_A is too short
    m, n, rp, col = si.structure("rect513x40")
    wide = sp.Plan.from_device_csr(m, n, _dev(rp), _dev(col), _dev(np.ones(len(col))), "csr", transpose=True)
    assert (wide.m, wide.n) == (40, 513)
    with pytest.raises(ValueError, match="x holds 40"):
        wide.execute(np.ones(40), np.zeros(40))
    y = np.full(40, np.nan)
    wide.execute(np.ones(513), y)
    assert np.array_equal(y, np.bincount(col, minlength=40).astype(np.float64))  # column counts, exact
    # prepare_update checks row_ptr against the source shape (m_A + 1 = 514 entries)
    with pytest.raises(ValueError, match="the plan needs 514"):
        wide.prepare_update(np.zeros(41, np.int64), col)
    st = C.c_int32(-1)
    assert sp.lib().spmv_plan_is_transposed(wide._h, C.byref(st)) == 0 and st.value == 1
    for p in (plan, comp, wide):
        p.destroy()


def test_configs_cover_every_format():
    assert {f for _, f, _ in CONFIGS} >= {"csr", "ss", "ell", "hyb", "jds", "coo", "css", "bin", "dia", "auto"}
