"""Every format on a y of 4 GiB and more: both sides of m = 2^29 (the byte
offset of y[r] and of the 64-bit row pointers passes 2^32), rows beyond 2^30
(the 4-byte per-row arrays -- 32-bit row pointers, perm, rmap, nzrow,
empty_rows, the row lists of adaptive CSR and of the HYB / JDS overflow --
pass 4 GiB) and the API's largest m = 2^31 - 2; for k right-hand sides,
Y[r * ldy + j] beyond 2^32 bytes at m = 2^26, ldy = 8.

The matrices are tiny (4003 live rows, tests/tall_inputs.py); only y and the
per-row arrays are big.  Nothing of size m lives on the host: the row pointers
are a cumsum on the device, the plans are built there (Plan.from_device_csr),
and y is judged there -- the live rows within signed_inputs.row_tol of the
extended-precision reference, bit for bit the oracle's sequential sum where
the plan is sequential, every other row +0.0 exactly.  Every execute case then
runs y = -2.5 A x + 0.75 y once on the same plan and y (tall_inputs.y0_rows,
check_axpby_y): the fused CSR / ELL / JDS / DIA kernels' load of y[row], and
the generic path's scratch of m + 2 doubles with axpby_kernel over all m rows;
test_tall_axpby_zero runs that kernel on plans with nothing stored.  One
row_ptr and one y are alive per size (peak about 38 GiB in the default
selection; m = 2^31 - 2
for every format, and ELL, BIN, AUTO and DIA at 2^30 rows, are opt-in,
SPMV_HUGE_TESTS=1, about 100 GiB; profiles/tall_y/README.md has the measured
lines and why the default selection is cut as it is).  Needs an MI355X:
`pytest -m gpu`.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest

import signed_inputs as si
import singlespmv_amd as sp
import special_values as sv
import tall_inputs as ti
from multi_inputs import SENTINEL
from test_gpu_wide_x import CONFIGS

pytestmark = pytest.mark.gpu

T = ti.TALL
GIB = 1 << 30
HUGE = pytest.mark.skipif(os.environ.get("SPMV_HUGE_TESTS") != "1", reason="opt-in: SPMV_HUGE_TESTS=1")
FILLS = (float("nan"), SENTINEL)


def _mid(m):
    return {T - 1: "T-1", T + 4099: "T+4099", 2 * T + 4099: "2T+4099", 4 * T - 2: "4T-2",
            ti.MULTI_TALL - 1: "T/8-1", ti.MULTI_TALL + 4099: "T/8+4099"}[m]


# ---------------------------------------------------------------- the two big buffers
class _Buffer:
    """The device row pointers (m + 1 int64) and y (m * ld doubles) of one
    size, refilled for every case."""

    def __init__(self, m, ld, rp, y):
        self.m, self.ld, self.rp, self.y = m, ld, rp, y
        self.rp_of = None

    def csr(self, c):
        """(row_ptr, col, val) of the case on the device; the row pointers
        are rebuilt only when the structure changes."""
        import torch
        assert c["m"] == self.m
        if self.rp_of != c["name"]:
            self.rp_of = None
            ti.device_csr(c, self.m, "cuda", out=self.rp)
            self.rp_of = c["name"]
        return self.rp, torch.from_numpy(np.array(c["col"])).cuda(), torch.from_numpy(np.array(c["val"])).cuda()

    def Y(self):
        return self.y.view(self.m, self.ld)


@pytest.fixture(scope="module")
def tall_buf(request):
    """The device buffers of one (m, ld, rp?, extra), module-scoped and
    parametrised as test_gpu_wide_x.wide_buf: each parameter is torn down (its
    memory returned to the device) before the next is set up.  `extra`: what
    the largest plan of the size adds (DIA: x and three diagonals of m; the
    execute cases: the m + 2 doubles a generic plan's execute_axpby
    allocates), so that a device too small for a case skips it at set-up."""
    import torch
    m, ld, with_rp, extra = request.param
    need = 8 * m * ld + (8 * (m + 1) if with_rp else 0) + extra
    free, total = torch.cuda.mem_get_info()
    if free < need + 8 * GIB:
        pytest.skip(f"y, row_ptr and the plans of {need / GIB:.1f} GiB + 8 GiB need more than the {free / GIB:.1f} GiB "
                    f"free of {total / GIB:.1f} GiB")
    b = _Buffer(m, ld, torch.empty(m + 1 if with_rp else 0, dtype=torch.int64, device="cuda"),
                torch.empty(m * ld, dtype=torch.float64, device="cuda"))
    yield b
    torch.cuda.synchronize()
    for t in (b.rp, b.y):
        t.untyped_storage().resize_(0)  # whatever view a failed test's traceback still holds
    b.rp = b.y = None
    torch.cuda.empty_cache()


def _buf(m, ld=1, with_rp=True, extra=0, marks=()):
    return pytest.param((m, ld, with_rp, extra), id=_mid(m) + (f"-ld{ld}" if ld > 1 else ""), marks=marks)


def _used_gib():
    """Device memory in use right now, GiB (a measurement for the printed lines)."""
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / GIB


# ---------------------------------------------------------------- checks
def _execute_twice(plan, x, y, c, what):
    """Two executes into the one y buffer, over a NaN and over a
    -1.2345e300 fill: tall_inputs.check_y on both, the live rows bit for bit
    the same (COO: inside one unit).  Returns (the largest err / row_tol, the
    live rows of the first execute)."""
    info = plan.info()
    worst, first = 0.0, None
    for fill in FILLS:
        y.fill_(fill)
        plan.execute(x, y)
        now = ti.live(y, c)
        worst = max(worst, ti.check_y(y, c, what + ("" if first is None else " (2nd execute)"), info=info, prev=first))
        first = now if first is None else first
    return worst, first


def _axpby_path(info):
    """The path spmv_execute_axpby takes on a plan of this format: CSR, ELL, DIA and JDS without overflow rows
    have one writer per row and take alpha and beta in their store."""
    fused = info["format"] in ("csr", "ell", "dia") or (info["format"] == "jds" and info["overflow_nnz"] == 0)
    return "fused" if fused else "generic"


def _axpby(plan, x, y, c, first, what):
    """One execute_axpby(x, y, -2.5, 0.75) on the m-entry y filled with tall_inputs' y0, `first` the live rows of
    the plain execute: the path the plan must take, the scratch of m + 2 doubles a generic plan allocates for it,
    and tall_inputs.check_axpby_y.  Returns (the path, the largest err / bound)."""
    info = plan.info()
    path = plan.axpby_path()
    assert path == _axpby_path(info), (what, info["format"], path)
    ti.fill_y0(y)
    plan.execute_axpby(x, y, *ti.AXPBY)
    grown = plan.info()["device_bytes"] - info["device_bytes"]
    assert grown >= 8 * c["m"] if path == "generic" else grown == 0, (what, path, grown)
    return path, ti.check_axpby_y(y, c, first, *ti.AXPBY, what, info)


def _only_live(y, c, what):
    """The live rows of y; every other row must be +0.0 (y's live rows are
    zeroed in place on the way)."""
    import torch
    h = ti.live(y, c)
    y[torch.from_numpy(np.array(c["rowmap"])).cuda()] = 0.0
    assert ti.nonzero_bits(y) == 0, f"{what}: a row off the live ones is not +0.0"
    return h


def _device_plan(buf, c, fmt, kw):
    rp, col, val = buf.csr(c)
    return sp.Plan.from_device_csr(c["m"], c["n"], rp, col, val, fmt=fmt, **kw)


def _dia_fill(c):
    """dia_max_fill that accepts three diagonals of m rows for the case's
    entries (the default 3.0 allows 3 m <= 3 nnz)."""
    return 1.01 * 3.0 * c["m"] / len(c["val"])


# ---------------------------------------------------------------- 1. execute
# test_gpu_wide_x.CONFIGS without DIA (tall_band below) and without the second CSS slab width (a column-side option)
TALL_CONFIGS = [(cid, fmt, kw) for cid, fmt, kw in CONFIGS if fmt != "dia" and "css_slab_shift" not in kw]
ROWS4 = ("csr", "ss", "hyb", "jds", "css", "coo")  # the formats with 4-byte per-row arrays: what m = 2^30 is about


def _cases(keep):
    return [pytest.param(name, fmt, kw, id=f"{name}-{cid}")
            for name in ti.STRUCTURES for cid, fmt, kw in TALL_CONFIGS if keep(fmt)]


def _scratch(m):
    """What the first execute_axpby adds to a generic plan: its scratch of m + 2 doubles."""
    return 8 * (m + 2)


SIZES = [_buf(T - 1, extra=_scratch(T - 1)), _buf(T + 4099, extra=_scratch(T + 4099)),
         _buf(4 * T - 2, extra=_scratch(4 * T - 2), marks=HUGE)]
# DIA: x (8 m) and three diagonals of m rows rounded up to 512 (24 m) on top; its axpby is fused, no scratch
DIA_SIZES = [_buf(T - 1, extra=32 * T), _buf(T + 4099, extra=32 * T), _buf(2 * T + 4099, extra=64 * T, marks=HUGE),
             _buf(4 * T - 2, extra=128 * T, marks=HUGE)]


def _assert_path(name, fmt, kw, info, c):
    """The configuration reaches the path it is here for (AUTO: any format)."""
    lens = np.diff(c["rp"])
    assert info["n"] == c["n"] and info["m"] == c["m"] and info["nnz"] == len(c["val"])
    if fmt == "auto":
        return
    assert info["format"] == fmt, info["format"]
    if fmt == "csr":
        lanes = kw["csr_lanes"]
        if lanes == 0 and name == "tall_long":  # rows beyond 4096 entries: the per-bin row lists over all m rows
            assert info["kernel"] == "csr_adaptive_kernel", info["kernel"]
        else:  # lanes 0 on tall_uniform: the empty rows are > 99 % of one bin, one lane serves 16 entries
            lanes = lanes or 1
            assert info["kernel"] == f"csr_slab2_kernel<{lanes}>" and info["csr_lanes"] == lanes, info["kernel"]
    if name == "tall_long":
        if fmt == "hyb":
            assert info["n_kernels"] == 2 and info["overflow_nnz"] > 0
        if fmt == "jds":
            assert info["overflow_nnz"] > 0
        if fmt == "css":
            assert info["css_split_rows"] > 0
        if kw.get("bin_long_len") == 40:
            assert info["bin_long_rows"] > 0 and info["bin_long_len"] == 40
    if kw.get("ell_width") == 4:
        assert info["overflow_nnz"] == int(np.maximum(lens - 4, 0).sum()) > 0
    if kw.get("bin_long_len") == -1:
        assert info["bin_long_len"] == 0 and info["bin_long_rows"] == 0 and si.plan_is_sequential(info)
    if fmt == "jds":
        assert info["kernel"].startswith("ell_slice_kernel<perm>"), info["kernel"]  # perm over all m rows
    if fmt == "dia":
        assert info["n_diags"] == 3 and si.plan_is_sequential(info)
    if fmt == "ell":
        assert info["ell_width"] == -(-int(lens.max()) // 4) * 4  # whole 4-entry chunks


def _line(what, info, worst, t0, axpby=None):
    ab = "" if axpby is None else f"axpby={axpby[0]} err/bound={axpby[1]:.3f} "
    print(f"tall-y {what} format={info['format']} kernel={info['kernel']} err/row_tol={worst:.3f} {ab}"
          f"device-used={_used_gib():.1f}GiB wall={time.perf_counter() - t0:.1f}s")


def _bin_refused(buf, c, fmt, e, what):
    """BIN's documented grid limit (row bins x column strips > 2^28): the
    refusal is the result, and AUTO must not have picked BIN."""
    assert fmt == "bin" and "not supported" in str(e) and "segment table limit" in str(e), (what, str(e))
    auto = _device_plan(buf, c, "auto", {})
    assert auto.info()["format"] != "bin"
    auto.destroy()
    print(f"tall-y {what} refused: {e}")


def _execute_case(buf, name, fmt, kw, what):
    t0 = time.perf_counter()
    c = ti.case(name, buf.m)
    try:
        plan = _device_plan(buf, c, fmt, kw)
    except sp.SpmvError as e:
        return _bin_refused(buf, c, fmt, e, what)
    info = plan.info()
    assert plan.built_on_device()
    _assert_path(name, fmt, kw, info, c)
    x = ti.device_x(c, "cuda")
    worst, first = _execute_twice(plan, x, buf.y, c, what)
    ab = _axpby(plan, x, buf.y, c, first, what)
    _line(what, info, worst, t0, ab)
    plan.destroy()


@pytest.mark.parametrize("name,fmt,kw", _cases(lambda fmt: True))
@pytest.mark.parametrize("tall_buf", SIZES, indirect=True)
def test_tall_execute(tall_buf, name, fmt, kw, request):
    """Device-built plan, device x and y, two executes (NaN- and
    -1.2345e300-filled y): tall_inputs.check_y."""
    _execute_case(tall_buf, name, fmt, kw, request.node.callspec.id)


@pytest.mark.parametrize("name,fmt,kw", _cases(lambda fmt: fmt in ROWS4))
@pytest.mark.parametrize("tall_buf", [_buf(2 * T + 4099, extra=_scratch(2 * T + 4099))], indirect=True)
def test_tall_execute_rows4(tall_buf, name, fmt, kw, request):
    """Rows beyond 2^30 on the formats whose per-row arrays hold 4-byte
    entries (the others at this size: opt-in, below)."""
    _execute_case(tall_buf, name, fmt, kw, request.node.callspec.id)


@pytest.mark.parametrize("name,fmt,kw", _cases(lambda fmt: fmt not in ROWS4))
@pytest.mark.parametrize("tall_buf", [_buf(2 * T + 4099, extra=_scratch(2 * T + 4099), marks=HUGE)], indirect=True)
def test_tall_execute_rows8(tall_buf, name, fmt, kw, request):
    """Rows beyond 2^30 on ELL, BIN and AUTO."""
    _execute_case(tall_buf, name, fmt, kw, request.node.callspec.id)


@pytest.mark.parametrize("tall_buf", DIA_SIZES, indirect=True)
def test_tall_execute_dia(tall_buf, request):
    """DIA on tall_band (n = m): three diagonals over all m rows, accepted
    with dia_max_fill raised."""
    c = ti.case(ti.BAND, tall_buf.m)
    _execute_case(tall_buf, ti.BAND, "dia", {"dia_max_fill": _dia_fill(c)}, request.node.callspec.id + "-tall_band-dia")


# ---------------------------------------------------------------- 2. the other routes
def _csr32_device_plan(c, rp32, col, val, fmt):
    o = sp.make_options(fmt, device=0)
    h = C.c_void_p()
    L = sp.lib()
    st = L.spmv_plan_create_csr32_device(c["m"], c["n"], len(c["val"]), sp._ptr(rp32), sp._ptr(col), sp._ptr(val),
                                         C.byref(o), C.byref(h))
    assert st == 0, L.spmv_last_error().decode()
    return sp.Plan(h.value)


@pytest.mark.parametrize("fmt", ["csr", "ell"])
@pytest.mark.parametrize("tall_buf", [_buf(T + 4099)], indirect=True)
def test_tall_routes(tall_buf, fmt, request):
    """execute(alpha) -- scale_kernel over m --, a graph replay, Plan.time,
    and spmv_plan_create_csr32_device (int32 device row pointers): the y of
    the plain execute, bit for bit."""
    import torch
    t0 = time.perf_counter()
    what = request.node.callspec.id
    c = ti.case("tall_long", tall_buf.m)
    y = tall_buf.y
    plan = _device_plan(tall_buf, c, fmt, {})
    x = ti.device_x(c, "cuda")
    worst, first = _execute_twice(plan, x, y, c, what)
    y.fill_(SENTINEL)
    plan.execute(x, y, alpha=2.5)
    assert np.array_equal(sv.bits(_only_live(y, c, what + " alpha")), sv.bits(2.5 * first)), f"{what}: alpha * y"
    y.fill_(SENTINEL)
    g = plan.graph(x, y, 2)
    g.launch()
    torch.cuda.synchronize()
    assert np.array_equal(sv.bits(_only_live(y, c, what + " graph")), sv.bits(first)), f"{what}: graph replay"
    g.destroy()
    y.fill_(SENTINEL)
    assert plan.time(x, y, 2) > 0
    assert np.array_equal(sv.bits(_only_live(y, c, what + " time")), sv.bits(first)), f"{what}: Plan.time"
    rp, col, val = tall_buf.csr(c)
    p32 = _csr32_device_plan(c, rp.to(torch.int32), col, val, fmt)
    assert p32.built_on_device() and p32.info()["kernel"] == plan.info()["kernel"]
    assert p32.digest() == plan.digest(), f"{what}: the int32 entry point builds another layout"
    y.fill_(SENTINEL)
    p32.execute(x, y)
    assert np.array_equal(sv.bits(_only_live(y, c, what + " csr32_device")), sv.bits(first)), f"{what}: csr32_device"
    _line(what, plan.info(), worst, t0)
    p32.destroy()
    plan.destroy()


# ---------------------------------------------------------------- 3. host builders
@pytest.fixture(scope="module")
def host_rp():
    """The numpy row pointers (4.3 GB) of tall_long at m = T + 4099, copied
    back from the device once for the host-build cases."""
    return {}


@pytest.mark.parametrize("fmt", ["csr", "ell"])
@pytest.mark.parametrize("tall_buf", [_buf(T + 4099)], indirect=True)
def test_tall_host_build(tall_buf, host_rp, fmt, request):
    """Plan.from_csr(build="host") from host row pointers of 4.3 GB -- the
    host builders (formats.cpp) past 2^29 rows: the device build's layout
    array by array (spmv_plan_digest) and its y."""
    t0 = time.perf_counter()
    what = request.node.callspec.id
    c = ti.case("tall_long", tall_buf.m)
    pd = _device_plan(tall_buf, c, fmt, {})
    if "rp" not in host_rp:
        host_rp["rp"] = tall_buf.rp.cpu().numpy()
    ph = sp.Plan.from_csr(c["m"], c["n"], host_rp["rp"], c["col"], c["val"], fmt, build="host")
    assert pd.built_on_device() and not ph.built_on_device()
    ih, idv = ph.info(), pd.info()
    assert ih["format"] == idv["format"] == fmt and ih["kernel"] == idv["kernel"]
    dh, dd = ph.digest(), pd.digest()
    assert list(dd) == list(dh), (what, list(dd), list(dh))
    bad = [a for a in dh if dh[a] != dd[a]]
    assert not bad, f"{what}: host layout differs from the device build in {bad}"
    x = ti.device_x(c, "cuda")
    _, yd = _execute_twice(pd, x, tall_buf.y, c, what + " device build")
    worst, yh = _execute_twice(ph, x, tall_buf.y, c, what + " host build")
    assert np.array_equal(sv.bits(yh), sv.bits(yd)), f"{what}: differs from the device build"
    _line(what, ih, worst, t0)
    ph.destroy()
    pd.destroy()
    if fmt == "ell":  # the last case: give the 4.3 GB back
        host_rp.clear()


@pytest.mark.parametrize("fmt", ["csr", "ss", "ell"])
def test_csr32_host_small(fmt):
    """spmv_plan_create_csr32 (host int32 row pointers) on the staircase:
    the layout and the y of Plan.from_csr."""
    c = si.case("staircase", "cancel")
    ref = sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt)
    rp32, col, val = c["rp"].astype(np.int32), np.ascontiguousarray(c["col"], np.int32), np.ascontiguousarray(c["val"])
    o = sp.make_options(fmt)
    h = C.c_void_p()
    L = sp.lib()
    st = L.spmv_plan_create_csr32(c["m"], c["n"], len(val), rp32.ctypes.data, col.ctypes.data, val.ctypes.data,
                                  C.byref(o), C.byref(h))
    assert st == 0, L.spmv_last_error().decode()
    p32 = sp.Plan(h.value)
    assert p32.info()["kernel"] == ref.info()["kernel"] and p32.digest() == ref.digest()
    x = np.ascontiguousarray(c["x"])
    ya, yb = np.full(c["m"], np.nan), np.full(c["m"], SENTINEL)
    ref.execute(x, ya)
    p32.execute(x, yb)
    assert np.array_equal(sv.bits(ya), sv.bits(yb))
    si.assert_rows(yb, c["rp"], c["col"], c["val"], c["x"], f"csr32 {fmt}", ref=c["ref"])
    p32.destroy()
    ref.destroy()


# ---------------------------------------------------------------- 4. multi-vector
LDY = 8
MULTI = [pytest.param("tall_uniform", "ell", 8, [8], id="tall_uniform-ell-k8"),
         pytest.param("tall_uniform", "jds", 8, [8], id="tall_uniform-jds-k8"),
         pytest.param(ti.BAND, "dia", 8, [8], id="tall_band-dia-k8"),
         pytest.param("tall_uniform", "csr", 3, [1, 1, 1], id="tall_uniform-csr-k3"),
         pytest.param("tall_uniform", "bin", 3, [1, 1, 1], id="tall_uniform-bin-k3")]


# DIA: X (64 m) and three diagonals (24 m) on top of Y and row_ptr
@pytest.mark.parametrize("name,fmt,k,path", MULTI)
@pytest.mark.parametrize("tall_buf", [_buf(m, LDY, extra=88 * m) for m in ti.MULTI_MS], indirect=True)
def test_tall_multi(tall_buf, name, fmt, k, path, request):
    """execute_multi into a Y of row stride 8 and 4 GiB: the fused ELL / JDS
    (no overflow) / DIA kernels at k = 8, the generic path (CSR, BIN) at
    k = 3.  Every column as check_y on the strided view Y[:, j]; the columns
    [k, ldy) keep their fill bit for bit."""
    import torch
    t0 = time.perf_counter()
    what = request.node.callspec.id
    c = ti.case(name, tall_buf.m)
    plan = _device_plan(tall_buf, c, fmt, {"dia_max_fill": _dia_fill(c)} if fmt == "dia" else {})
    info = plan.info()
    assert info["format"] == fmt and info["overflow_nnz"] == 0
    X = ti.device_X(c, LDY, k, "cuda")[:, :k]
    Ybuf = tall_buf.Y()
    Y = Ybuf[:, :k]
    worst, first = 0.0, None
    for fill in FILLS:
        Ybuf.fill_(fill)
        assert plan.multi_path(X, Y) == path, (what, plan.multi_path(X, Y))
        plan.execute_multi(X, Y)
        pad = Ybuf[:, k:].view(torch.int64) != int(sv.bits(np.array([fill]))[0])
        assert int(torch.count_nonzero(pad)) == 0, f"{what}: a pad column of Y was written"
        del pad
        now = [ti.live(Ybuf[:, j], c) for j in range(k)]
        for j in range(k):
            cj = ti.column(name, tall_buf.m, j)
            worst = max(worst, ti.check_y(Ybuf[:, j], c, f"{what} column {j}", info=info, col=cj,
                                          prev=None if first is None else first[j]))
        first = now if first is None else first
    _line(f"multi {what} path={path}", info, worst, t0)
    plan.destroy()


@pytest.mark.parametrize("tall_buf", [_buf(T + 4099, LDY, with_rp=False)], indirect=True)
def test_tall_multi_zero(tall_buf, request):
    """A plan with nothing stored (DIA without a diagonal, nnz = 0) at
    m * k beyond 2^32: execute_multi succeeds and the k = 8 used columns of
    a Y of 34 GiB, the only big buffer alive, are +0.0 everywhere."""
    import torch
    t0 = time.perf_counter()
    m, n, k = tall_buf.m, 8, 8
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    plan = sp.Plan.from_device_csr(m, n, rp, torch.zeros(0, dtype=torch.int32, device="cuda"),
                                   torch.zeros(0, dtype=torch.float64, device="cuda"), fmt="dia")
    rp.untyped_storage().resize_(0)
    del rp
    torch.cuda.empty_cache()
    info = plan.info()
    assert info["format"] == "dia" and info["n_diags"] == 0 and info["nnz"] == 0
    X = torch.full((n, k), float("nan"), dtype=torch.float64, device="cuda")  # never read
    Y = tall_buf.Y()
    for fill in FILLS:
        Y.fill_(fill)
        assert plan.multi_path(X, Y) == [8]
        plan.execute_multi(X, Y)  # raises unless the call returns success
        assert ti.nonzero_bits(tall_buf.y) == 0, "Y is not +0.0 everywhere"
    _line(request.node.callspec.id + " multi-zero", info, 0.0, t0)
    plan.destroy()


@pytest.mark.parametrize("fmt", ["csr", "dia"])
@pytest.mark.parametrize("tall_buf", [_buf(T + 4099, LDY, with_rp=False)], indirect=True)
def test_tall_axpby_zero(tall_buf, fmt, request):
    """execute_axpby on a plan with nothing stored (CSR with nnz = 0, DIA
    without a diagonal), m = 2^29 + 4099: axpby_kernel without row sums over
    all m rows, on the first m entries of multi-zero's buffer.  Every row is
    bit for bit 0.75 * y0[r] = alpha * (+0.0) + beta * y0[r]; the entry after
    the last row keeps its fill."""
    import torch
    t0 = time.perf_counter()
    what = request.node.callspec.id
    m, n = tall_buf.m, 8
    rp = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    plan = sp.Plan.from_device_csr(m, n, rp, torch.zeros(0, dtype=torch.int32, device="cuda"),
                                   torch.zeros(0, dtype=torch.float64, device="cuda"), fmt=fmt)
    rp.untyped_storage().resize_(0)
    del rp
    torch.cuda.empty_cache()
    info = plan.info()
    assert info["format"] == fmt and info["nnz"] == 0 and plan.axpby_path() == "fused"
    x = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")  # never read
    y = tall_buf.y[:m]
    ti.fill_y0(y)
    tall_buf.y[m] = SENTINEL
    plan.execute_axpby(x, y, *ti.AXPBY)
    assert plan.info()["device_bytes"] == info["device_bytes"]  # no scratch
    stray, at = ti.off_pattern(y, ti.AXPBY[1])
    assert stray == 0, (f"{what}: {stray} rows are not 0.75 * y0, first {at}: {[float(y[r]) for r in at]} vs "
                        f"{(ti.AXPBY[1] * ti.y0_rows(at)).tolist()}")
    assert float(tall_buf.y[m]) == SENTINEL, f"{what}: the entry after the last row was written"
    _line(what + " axpby-zero", info, 0.0, t0, ("fused", 0.0))
    plan.destroy()
