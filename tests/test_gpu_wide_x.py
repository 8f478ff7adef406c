"""Every format on an x of 4 GiB and more: both sides of the 32-bit / 64-bit
x addressing switch at n = 2^29 (tests/wide_inputs.py names the three guards),
columns beyond 2^28, 2^29 and 2^30, and the API's largest n = 2^31 - 2.

The matrices are tiny (about 4 000 rows); only x is big.  x is NaN over all n
entries except on the columns a layout may multiply, so a read at a wrapped or
sign-extended offset poisons its row wherever it lands: y must be finite on
every row, within signed_inputs.row_tol of the extended-precision reference on
the compact columns, and bit for bit the oracle's sequential sum where the
plan is sequential.  Every test_wide_execute case then runs
y = -2.5 A x + 0.75 y once on the same plan and x: the fused kernels choose
their x addressing on their own.  One device x is alive at a time (peak about 20 GiB in the
multi-vector case of 16 GiB).  Needs an MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest

import axpby_inputs as ai
import signed_inputs as si
import singlespmv_amd as sp
import special_values as sv
import wide_inputs as wi
from multi_inputs import SENTINEL
from test_gpu_parity import _device_csr, assert_bin_rows

pytestmark = pytest.mark.gpu

W = wi.WIDE
GIB = 1 << 30
AXPBY = (-2.5, 0.75)  # (alpha, beta) of the one execute_axpby of every test_wide_execute case


def _nid(n):
    return {W - 1: "W-1", W: "W", W + 4099: "W+4099", 2 * W + 4099: "2W+4099", 4 * W - 2: "4W-2",
            wi.MULTI_WIDE - 1: "W/8-1", wi.MULTI_WIDE: "W/8", wi.MULTI_WIDE + 4099: "W/8+4099"}[n]


# ---------------------------------------------------------------- the one big buffer
class _Buffer:
    """n * ld doubles of device memory, refilled for every case."""

    def __init__(self, n, ld, t):
        self.n, self.ld, self.t = n, ld, t

    def x(self, c):
        assert self.ld == 1 and c["n"] == self.n
        return wi.device_x(self.n, c["ucol"], c["x_c"], self.t.device, out=self.t)

    def X(self, c, k):
        assert c["n"] == self.n and k <= self.ld
        cols = np.stack([wi.column(c["name"], self.n, j)["x_c"] for j in range(k)], axis=1)
        return wi.device_X(self.n, self.ld, c["ucol"], cols, self.t.device, out=self.t.view(self.n, self.ld))


@pytest.fixture(scope="module")
def wide_buf(request):
    """The device buffer of one (n, ld), module-scoped and parametrised: each
    parameter is torn down (its memory returned to the device) before the
    next is set up, so one buffer is alive at a time."""
    import torch
    n, ld = request.param
    need = 8 * n * ld
    free, total = torch.cuda.mem_get_info()
    if free < need + 8 * GIB:
        pytest.skip(f"x of {need / GIB:.1f} GiB + 8 GiB needs more than the {free / GIB:.1f} GiB free "
                    f"of {total / GIB:.1f} GiB")
    b = _Buffer(n, ld, torch.empty(n * ld, dtype=torch.float64, device="cuda"))
    yield b
    torch.cuda.synchronize()
    b.t.untyped_storage().resize_(0)  # whatever view a failed test's traceback still holds
    b.t = None
    torch.cuda.empty_cache()


def _buf(n, ld=1):
    return pytest.param((n, ld), id=_nid(n) + (f"-ld{ld}" if ld > 1 else ""))


def _used_gib():
    """Device memory in use right now, GiB (a measurement for the printed lines)."""
    import torch
    free, total = torch.cuda.mem_get_info()
    return (total - free) / GIB


# ---------------------------------------------------------------- checks
def _device_y(m, fill):
    import torch
    return torch.full((m,), fill, dtype=torch.float64, device="cuda")


def _execute_twice(plan, x, m):
    """y over a NaN-filled and over a -1.2345e300-filled device buffer."""
    ya, yb = _device_y(m, float("nan")), _device_y(m, SENTINEL)
    plan.execute(x, ya)
    plan.execute(x, yb)
    return ya.cpu().numpy(), yb.cpu().numpy()


def _check_y(plan, c, ya, yb, what, col=None):
    """test_gpu_signed._check_y on the compact arrays (x_c, ccol), plus
    finiteness; returns the largest err / row_tol."""
    rp, info = c["rp"], plan.info()
    x_c = c["x_c"] if col is None else col["x_c"]
    y_oracle = c["y_oracle"] if col is None else col["y_oracle"]
    worst = wi.check_y(ya, c, what, col)
    lens = np.diff(rp)
    if info["format"] == "coo":
        # f64 atomics: a row split across 128-entry units may round differently
        # run to run; a row inside one unit gets exactly one atomic
        worst = max(worst, wi.check_y(yb, c, what + " (2nd execute)", col))
        inside = (rp[:-1] // 128 == (rp[1:] - 1) // 128) & (lens > 0)
        assert np.array_equal(ya[inside], yb[inside]), f"{what}: rows inside one unit differ run to run"
        assert (ya[lens == 0] == 0).all() and (yb[lens == 0] == 0).all()
    else:
        assert np.array_equal(sv.bits(ya), sv.bits(yb)), f"{what}: y depends on what y held before"
    if c["name"] == wi.UNSORTED:  # rows out of column order: no layout owes the CSR-order sum (BIN adds strip by strip)
        return worst
    if info["format"] == "bin":
        assert_bin_rows(plan, ya, rp, c["ccol"], c["val"], x_c, what=what)
    if si.plan_is_sequential(info):  # rows ascend in column order, DIA runs without duplicates
        assert np.array_equal(ya, y_oracle), f"{what}: {info['format']} is sequential, must be bit-exact"
    return worst


def _check_axpby(plan, c, x, ya, what):
    """One execute_axpby(x, y, -2.5, 0.75) on a device copy of
    axpby_inputs.y0(m), ya = the plan's plain execute: the fused twins choose
    their x addressing again (CSR, ELL, DIA; JDS without overflow rows), every
    other plan runs its own kernels into its scratch.  Bit for bit
    expected(ya, y0, ...) (COO: on the rows inside one 128-entry unit), and
    every plan within axpby_inputs.assert_bound on the compact arrays.
    Returns (the path, the largest err / bound)."""
    import torch
    info, m, rp = plan.info(), c["m"], c["rp"]
    fused = info["format"] in ("csr", "ell", "dia") or (info["format"] == "jds" and info["overflow_nnz"] == 0)
    path = plan.axpby_path()
    assert path == ("fused" if fused else "generic"), (what, info["format"], path)
    y0 = ai.y0(m)
    yd = torch.from_numpy(np.array(y0)).cuda()
    plan.execute_axpby(x, yd, *AXPBY)
    y = yd.cpu().numpy()
    assert np.isfinite(y).all(), (f"{what}: axpby: {int((~np.isfinite(y)).sum())} rows read x outside the reach, "
                                  f"first {np.flatnonzero(~np.isfinite(y))[:5].tolist()}")
    rows = np.ones(m, bool)
    if info["format"] == "coo":  # f64 atomics: only a row inside one unit gets its sum in one piece
        rows = (rp[:-1] // 128 == (rp[1:] - 1) // 128) | (np.diff(rp) == 0)
    want = ai.expected(ya, y0, *AXPBY)
    bad = np.flatnonzero((ai.bits(y) != ai.bits(want)) & rows)
    assert not len(bad), (f"{what}: axpby: {len(bad)} rows are not expected(execute), first {bad[:5].tolist()}: "
                          f"{y[bad[:3]].tolist()} vs {want[bad[:3]].tolist()}")
    return path, ai.assert_bound(y, rp, c["ref"], y0, *AXPBY, what + ": axpby")


def _host_plan(c, fmt, kw):
    return sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, build="host", **kw)


# ---------------------------------------------------------------- 1. execute
CONFIGS = ([(f"csr-lanes{k}", "csr", {"csr_lanes": k}) for k in (0, 1, 16)]
           + [("ss", "ss", {}), ("ell", "ell", {}), ("hyb", "hyb", {}), ("hyb-width4", "hyb", {"ell_width": 4}),
              ("jds", "jds", {}), ("coo", "coo", {}), ("css", "css", {}), ("css-shift17", "css", {"css_slab_shift": 17}),
              ("bin", "bin", {}), ("bin-nolong", "bin", {"bin_long_len": -1}), ("bin-order2", "bin", {"bin_product_order": 2}),
              ("bin-long40", "bin", {"bin_long_len": 40}),
              ("dia", "dia", {}), ("auto", "auto", {})])
AUTO_FORMAT = {"far_uniform": "csr", "far_band": "dia", "two_bands": "dia", "far_long": "ss"}

# the buffer is parametrised on its own (stacked below): its parameter index
# then means the same n in every case, which is what pytest groups the cases of
# a module-scoped parameter by
EXECUTE_CASES = [pytest.param(name, fmt, kw, id=f"{name}-{cid}")
                 for name in wi.STRUCTURES for cid, fmt, kw in CONFIGS if fmt != "dia" or name in wi.BANDED]


def _assert_path(name, fmt, kw, info, c):
    """The configuration reaches the path it is here for."""
    n = c["n"]
    assert info["format"] == (AUTO_FORMAT[name] if fmt == "auto" else fmt), info["format"]
    assert info["n"] == n and info["m"] == c["m"] and info["nnz"] == len(c["val"])
    if fmt == "csr":
        lanes = kw["csr_lanes"]
        if lanes == 0:  # the empty rows keep any one lane count below 99 % of the rows
            assert info["kernel"] == "csr_adaptive_kernel", info["kernel"]
        else:
            kernel = "csr_slabx_kernel" if name == "far_band" else "csr_slab2_kernel"  # far_band: windows beyond 2^29
            assert info["kernel"] == f"{kernel}<{lanes}>" and info["csr_lanes"] == lanes, info["kernel"]
    if name == "far_long":
        if fmt == "hyb":
            assert info["n_kernels"] == 2 and info["overflow_nnz"] > 0
        if fmt == "jds":
            assert info["overflow_nnz"] > 0
        if fmt == "css":
            assert info["css_split_rows"] > 0
        if fmt == "bin" and not kw:
            # without options a row is long from max(128, strips) entries on (about one run piece per strip it
            # touches): >= 26 215 at these n, beyond the 9000-entry row -- the run path is bin-long40's here
            long_rows = int((np.diff(c["rp"]) >= max(128, info["bin_strips"])).sum())
            assert info["bin_long_rows"] == long_rows == 0, info
        if kw.get("bin_long_len") == 40:
            assert info["bin_long_rows"] > 0 and info["bin_long_len"] == 40
    if kw.get("bin_long_len") == -1:
        assert info["bin_long_len"] == 0 and info["bin_long_rows"] == 0 and si.plan_is_sequential(info)
    if fmt == "bin":
        assert info["bin_strips"] == -(-n // info["bin_strip_cols"]) and info["bin_strips"] >= 26_000
    if fmt == "css":  # the default slab shift stops at 24: 32 to 128 slabs; shift 17: 4096 to 16 384
        assert info["css_slabs"] == -(-n >> kw.get("css_slab_shift", 24)), info["css_slabs"]
    if info["format"] == "dia":
        assert info["n_diags"] == {"far_band": 17, "two_bands": 34}[name] and si.plan_is_sequential(info)
    if fmt == "ell":
        assert info["ell_width"] == -(-int(np.diff(c["rp"]).max()) // 4) * 4  # whole 4-entry chunks


@pytest.mark.parametrize("name,fmt,kw", EXECUTE_CASES)
@pytest.mark.parametrize("wide_buf", [_buf(n) for n in wi.NS], indirect=True)
def test_wide_execute(wide_buf, name, fmt, kw, request):
    """Host-built plan, device x and y, two executes (NaN- and -1.2345e300-
    filled y): finite, within row_tol, bit for bit the sequential sum where
    the plan is sequential, BIN as assert_bin_rows."""
    c = wi.case(name, wide_buf.n)
    what = request.node.callspec.id
    plan = _host_plan(c, fmt, kw)
    info = plan.info()
    _assert_path(name, fmt, kw, info, c)
    x = wide_buf.x(c)
    ya, yb = _execute_twice(plan, x, c["m"])
    worst = _check_y(plan, c, ya, yb, what)
    assert (sv.bits(ya[np.diff(c["rp"]) == 0]) == 0).all(), f"{what}: an empty row is not +0.0"
    path, worst_ab = _check_axpby(plan, c, x, ya, what)
    print(f"wide-x {what} format={info['format']} kernel={info['kernel']} err/row_tol={worst:.3f} "
          f"axpby={path} err/bound={worst_ab:.3f} device-used={_used_gib():.1f}GiB")
    plan.destroy()


# ---------------------------------------------------------------- 2. device builders
BUILD_FORMATS = ["csr", "ss", "ell", "hyb", "jds", "coo", "css", "bin", "dia", "auto"]
BUILD_CASES = [pytest.param(name, fmt, id=f"{name}-{fmt}@device")
               for name in wi.STRUCTURES + (wi.UNSORTED,) for fmt in BUILD_FORMATS if fmt != "dia" or name in wi.BANDED]
INFO_KEYS = ("format", "kernel", "empty_rows", "stored_slots", "algo_bytes", "n_kernels", "ell_width", "n_diags",
             "overflow_nnz", "csr_lanes", "ss_sigma", "css_slabs", "css_split_rows", "bin_bins", "bin_strips",
             "bin_long_len", "bin_long_rows")


@pytest.mark.parametrize("name,fmt", BUILD_CASES)
@pytest.mark.parametrize("wide_buf", [_buf(n) for n in (W - 1, W + 4099, 4 * W - 2)], indirect=True)
def test_wide_device_build(wide_buf, name, fmt, request):
    """Plan.from_device_csr (the diagonal census over m + n - 1 keys, the
    radix sorts of CSS by column and of BIN by strip, AUTO on device data):
    the host build's layout array by array (spmv_plan_digest), its format and
    kernel, and its y bit for bit (COO: within row_tol)."""
    c = wi.case(name, wide_buf.n)
    what = request.node.callspec.id
    ph = _host_plan(c, fmt, {})
    pd = sp.Plan.from_device_csr(c["m"], c["n"], *_device_csr(c["rp"].copy(), c["col"].copy(), c["val"].copy()), fmt=fmt)
    assert pd.built_on_device() and not ph.built_on_device()
    ih, idv = ph.info(), pd.info()
    if fmt != "auto":
        assert ih["format"] == fmt
    elif name != wi.UNSORTED:
        assert ih["format"] == AUTO_FORMAT[name]
    for k in INFO_KEYS:
        assert idv[k] == ih[k], f"{what}: info {k} {idv[k]} != {ih[k]}"
    dh, dd = ph.digest(), pd.digest()
    assert list(dd) == list(dh), (what, list(dd), list(dh))
    bad = [a for a in dh if dh[a] != dd[a]]
    assert not bad, f"{what}: device layout differs in {bad}"
    x = wide_buf.x(c)
    yh, _ = _execute_twice(ph, x, c["m"])
    ya, yb = _execute_twice(pd, x, c["m"])
    worst = _check_y(pd, c, ya, yb, what)
    if ih["format"] != "coo":
        assert np.array_equal(sv.bits(ya), sv.bits(yh)), f"{what}: differs from the host build"
    print(f"wide-x {what} format={ih['format']} err/row_tol={worst:.3f}")
    ph.destroy()
    pd.destroy()


# ---------------------------------------------------------------- 3. multi-vector
FUSED = [("far_uniform", "ell"), ("far_uniform", "jds"), ("far_band", "ell"), ("far_band", "jds"), ("far_band", "dia")]
GENERIC = [pytest.param((W + 4099, 2), "csr", 2, [1, 1], id="W+4099-ld2-csr-k2"),
           pytest.param((W + 4099, 2), "bin", 2, [1, 1], id="W+4099-ld2-bin-k2"),
           pytest.param((W + 4099, 4), "ell", 3, [2, 1], id="W+4099-ld4-ell-k3")]


def _multi(wide_buf, name, fmt, k, path, what):
    """One execute_multi on device blocks of row stride ld over a NaN- and a
    -1.2345e300-filled Y: the cut, every column as _check_y, the pad columns
    [k, ld) of Y untouched."""
    import torch
    n, ld = wide_buf.n, wide_buf.ld
    c = wi.case(name, n)
    m = c["m"]
    plan = _host_plan(c, fmt, {})
    info = plan.info()
    assert info["format"] == fmt and info["overflow_nnz"] == 0
    X = wide_buf.X(c, k)[:, :k]
    out = []
    for fill in (float("nan"), SENTINEL):
        Ybuf = torch.full((m, ld), fill, dtype=torch.float64, device="cuda")
        Y = Ybuf[:, :k]
        assert plan.multi_path(X, Y) == path, (what, plan.multi_path(X, Y))
        plan.execute_multi(X, Y)
        h = Ybuf.cpu().numpy()
        assert (sv.bits(h[:, k:]) == sv.bits(np.array([fill]))[0]).all(), f"{what}: a pad column of Y was written"
        out.append(np.ascontiguousarray(h[:, :k]))
    Ya, Yb = out
    worst = 0.0
    for j in range(k):
        cj = wi.column(name, n, j)
        worst = max(worst, _check_y(plan, c, np.ascontiguousarray(Ya[:, j]), np.ascontiguousarray(Yb[:, j]),
                                    f"{what} column {j}", col=cj))
    print(f"wide-x multi {what} path={path} err/row_tol={worst:.3f} device-used={_used_gib():.1f}GiB")
    plan.destroy()


@pytest.mark.parametrize("name,fmt", FUSED, ids=[f"{a}-{b}" for a, b in FUSED])
@pytest.mark.parametrize("wide_buf", [_buf(n, 8) for n in wi.MULTI_NS], indirect=True)
def test_wide_multi(wide_buf, name, fmt, request):
    """The fused ELL / JDS (no overflow) and DIA kernels at k = ldx = ldy = 8
    on an X of 4 GiB: both sides of n * ldx = 2^29."""
    _multi(wide_buf, name, fmt, 8, [8], request.node.callspec.id)


@pytest.mark.parametrize("wide_buf,fmt,k,path", GENERIC, indirect=["wide_buf"])
def test_wide_multi_generic(wide_buf, fmt, k, path, request):
    """The generic path's column pack and unpack at i * ldx beyond 2^29
    (n = WIDE + 4099): CSR and BIN at k = ldx = 2 (X of 8 GiB), and ELL at
    k = 3 in ldx = 4 (X of 16 GiB): one fused pair and one packed column."""
    _multi(wide_buf, "far_uniform", fmt, k, path, request.node.callspec.id)


# ---------------------------------------------------------------- 4. host x
def test_wide_host_x():
    """far_uniform, CSR, n = WIDE + 4099 with a host x: the H2D staging
    buffer sized by a wide n, then SPMV_X_STAGED re-use of it."""
    import torch
    n = W + 4099
    c = wi.case("far_uniform", n)
    free, total = torch.cuda.mem_get_info()
    if free < 8 * n + 8 * GIB:
        pytest.skip(f"the staged x of {8 * n / GIB:.1f} GiB + 8 GiB needs more than the {free / GIB:.1f} GiB free")
    plan = _host_plan(c, "csr", {"csr_lanes": 16})
    assert plan.info()["kernel"] == "csr_slab2_kernel<16>"
    x = np.full(n, np.nan)
    x[c["ucol"]] = c["x_c"]
    ya = np.full(c["m"], np.nan)
    plan.execute(x, ya)
    del x
    yb = np.full(c["m"], SENTINEL)
    L = sp.lib()
    assert L.spmv_execute(plan._h, None, yb.ctypes.data, sp.X_STAGED) == 0, L.spmv_last_error()
    worst = _check_y(plan, c, ya, yb, "host x")
    print(f"wide-x host-x err/row_tol={worst:.3f} device-used={_used_gib():.1f}GiB")
    plan.destroy()
