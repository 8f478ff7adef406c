"""Every execute route of every format on guarded, offset device buffers.

The parity tests hand Plan.execute host arrays, so the kernels run on the
plan's own 16-byte-aligned staging buffers, whose slack nobody looks at.  Here
x and y are device vectors inside guarded buffers (tests/guarded_buffers.py:
512 NaN doubles around x, 512 sentinel doubles around y), 16-byte aligned or
at an 8-byte offset, and every entry point that launches the kernels --
device pointers, a side stream, alpha, staged x / y, spmv_time, spmv_profile,
HIP graphs, the k = 1 in-place multi execute -- must give the y of the plan's
host execute bit for bit and leave every guard word alone (COO's split rows:
signed_inputs.row_tol; no tolerance of its own).  The baseline y itself is
held to the extended-precision reference once, and to the sequential sum bit
for bit where the plan is sequential.  One plan per test; every route runs
over a NaN-filled and over a sentinel-filled y.
Needs an MI355X: `pytest -m gpu`.
"""
import ctypes as C

import numpy as np
import pytest

import guarded_buffers as gb
import multi_inputs as mi
import signed_inputs as si
import singlespmv_amd as sp
from test_gpu_signed import CONFIGS as SIGNED_CONFIGS

pytestmark = pytest.mark.gpu

# bin-groups3: the groups' Mul launches share the phase / graph sequence.
# dia-fill1000: rect513x40 (one row past DIA's 512-row block) is beyond DIA's
# default fill limit; with the limit lifted it is a DIA plan.
CONFIGS = list(SIGNED_CONFIGS) + [("bin-groups3", "bin", {"bin_groups": 3})]
DIA_FILL = ("dia-fill1000", "dia", {"dia_max_fill": 1000.0})
STRUCTURES = (gb.STAIR_TAIL, "rect513x40", "uniform16", "banded", "short")


def _configs(name):
    if name == "short":  # every SS tile-end store path
        return [c for c in CONFIGS if c[1] == "ss"]
    out = [c for c in CONFIGS if c[1] != "dia" or name in ("banded", "rect513x40")]
    return out + [DIA_FILL] if name == "rect513x40" else out


CASES = [pytest.param(name, cid, fmt, kw, id=f"{name}-{cid}") for name in STRUCTURES for cid, fmt, kw in _configs(name)]

# The (structure, configuration) pairs whose builder refuses ("not supported"):
# for these the refusal is asserted, so no case skips.  A pair outside this
# set that refuses fails, and so does a pair inside it that builds.  No CSR,
# ELL, COO, SS or plain BIN entry.
EXPECTED_REFUSALS = {
    ("rect513x40", "dia"),  # 474 diagonals for 2 600 entries: beyond DIA's default fill limit (3.0)
}
_FORMAT_OF = {cid: fmt for cid, fmt, _ in CONFIGS + [DIA_FILL]}
assert all(_FORMAT_OF[cid] not in ("csr", "ell", "coo", "ss") and cid != "bin" for _, cid in EXPECTED_REFUSALS)

# the phase names include/spmv_hip.h documents at spmv_profile (JDS and HYB
# report "overflow" even when no row overflows; BIN two phases for any
# bin_groups: the groups' Mul launches are one phase)
PHASES = {"csr": ["csr"], "ell": ["ell"], "jds": ["ell", "overflow"], "hyb": ["ell", "overflow"],
          "ss": ["tile", "fixup"], "dia": ["dia"], "css": ["sweep"], "coo": ["zero_y", "segment"],
          "bin": ["mul", "sum"]}
OFFSETS = ((0, 0), (1, 0), (0, 1), (1, 1))
Y_FILLS = (float("nan"), mi.SENTINEL)


def _assert_path(name, fmt, kw, info, lens):
    """test_gpu_signed's assertions that a configuration reaches the path it is
    named for (stair_tail: what that test asserts for staircase)."""
    stair = name == gb.STAIR_TAIL
    if fmt != "auto":
        assert info["format"] == fmt, info["format"]
    if fmt == "csr":
        lanes = kw["csr_lanes"]
        if lanes == 0 and stair:
            assert info["kernel"] == "csr_adaptive_kernel", info["kernel"]
        elif name == "banded":
            assert info["kernel"].startswith("csr_slabx_kernel"), info["kernel"]
        elif name == "uniform16":
            assert info["kernel"].startswith("csr_slab2_kernel"), info["kernel"]
        if lanes:
            assert info["csr_lanes"] == lanes
    if stair:
        if fmt == "hyb":
            assert info["n_kernels"] == 2 and info["overflow_nnz"] > 0
        if fmt == "jds" and not kw:
            assert info["overflow_nnz"] > 0
        if fmt == "css":
            assert info["css_split_rows"] > 0
    if kw.get("ell_width") == 9000:
        assert info["overflow_nnz"] == 0 and si.plan_is_sequential(info)
    if kw.get("bin_long_len") == 40 and (lens >= 40).any():
        assert info["bin_long_rows"] > 0 and info["bin_long_len"] == 40
    if kw.get("bin_long_len") == -1:
        assert info["bin_long_len"] == 0 and info["bin_long_rows"] == 0 and si.plan_is_sequential(info)
    if kw.get("bin_groups") == 3:
        assert info["bin_groups"] == min(3, info["bin_bins"]), info  # one group per row bin at the most
    if fmt == "dia":
        assert si.plan_is_sequential(info)


class _Routes:
    """One plan, its baseline y and the guarded device buffers of one test."""

    def __init__(self, plan, c, what):
        import torch
        self.torch, self.plan, self.c, self.what = torch, plan, c, what
        self.info = plan.info()
        self.m, self.n = c["m"], c["n"]
        self.keep, self.ran = [], []  # every device tensor stays alive until the test's last synchronize
        self.x = {}
        xh = torch.from_numpy(np.array(c["x"]))  # a writable copy: the case's arrays are read-only
        for off in (0, 1):
            buf, view = gb.guarded_device(self.n, off, gb.X_FILL)
            view.copy_(xh)
            self.x[off] = (buf, view)
        y = np.full(self.m, np.nan)
        plan.execute(c["x"], y)
        self.y_base = y

    def y(self, off, fill):
        """A guarded device y at offset `off`, its used entries prefilled with `fill`."""
        buf, view = gb.guarded_device(self.m, off, gb.Y_FILL)
        view.fill_(fill)
        self.keep.append(buf)
        return buf, view

    def check(self, route, ybuf, x_off, y_off, **kw):
        """check_route on a guarded device y (and the x it was computed from)."""
        self.torch.cuda.synchronize()
        guards = [("y", ybuf, self.m, y_off, gb.Y_FILL)]
        if x_off is not None:
            guards.append(("x", self.x[x_off][0], self.n, x_off, gb.X_FILL))
        y = gb.used(ybuf, self.m, y_off)
        gb.check_route(y, self.y_base, self.c, self.info, f"{self.what} [{route}]", guards=guards, **kw)
        if route.split()[0] not in self.ran:
            self.ran.append(route.split()[0])
        return y

    def check_host(self, route, y, **kw):
        gb.check_route(y, self.y_base, self.c, self.info, f"{self.what} [{route}]", **kw)
        if route.split()[0] not in self.ran:
            self.ran.append(route.split()[0])

    # ---- 1. device pointers at every alignment
    def device(self):
        coo = self.info["format"] == "coo"
        first = None
        for fill in Y_FILLS:
            for x_off, y_off in OFFSETS:
                ybuf, yv = self.y(y_off, fill)
                xv = self.x[x_off][1]
                assert xv.data_ptr() % 16 == 8 * x_off and yv.data_ptr() % 16 == 8 * y_off
                self.plan.execute(xv, yv)
                y = self.check(f"device x+{x_off} y+{y_off} fill {fill}", ybuf, x_off, y_off)
                if first is None:
                    first = y
                # DIA: the scalar store branch (y + 1) gives the vector branch's y;
                # BIN: register staging of x (x + 1) gives LDS-DMA's
                assert coo or np.array_equal(mi.bits(y), mi.bits(first)), \
                    f"{self.what} [device]: offsets ({x_off}, {y_off}) differ from (0, 0)"

    # ---- 2. two async executes on a side stream
    def stream(self):
        torch = self.torch
        side = torch.cuda.Stream()
        ya, yb = self.y(1, Y_FILLS[0]), self.y(1, Y_FILLS[1])
        torch.cuda.synchronize()  # the fills ran on the default stream
        self.plan.set_stream(side)
        try:
            self.plan.execute(self.x[1][1], ya[1], async_=True)
            self.plan.execute(self.x[1][1], yb[1], async_=True)
            side.synchronize()
        finally:
            self.plan.set_stream(None)
        self.check("stream async 1st", ya[0], 1, 1)
        self.check("stream async 2nd", yb[0], 1, 1)

    # ---- 3. alpha
    def alpha(self):
        for alpha in (-2.0, 0.75):
            for fill in Y_FILLS:
                ybuf, yv = self.y(1, fill)
                self.plan.execute(self.x[1][1], yv, alpha=alpha)
                self.check(f"alpha {alpha} fill {fill}", ybuf, 1, 1, alpha=alpha)
        for fill in Y_FILLS:  # host buffers; expected 0.0 * y_base, signed zeros included
            buf, yv = gb.guarded(self.m, 1, gb.Y_FILL)
            yv[:] = fill
            self.plan.execute(self.c["x"], yv, alpha=0.0)
            self.check_host(f"alpha 0.0 host fill {fill}", np.array(yv), alpha=0.0,
                            guards=[("host y", buf, self.m, 1, gb.Y_FILL)])

    # ---- 4. staged x and y through the raw C-ABI
    def staged(self):
        L, h, m = sp.lib(), self.plan._h, self.m
        x = np.ascontiguousarray(self.c["x"])
        x_b = -2.0 * x
        for fill in Y_FILLS:
            def fetch():
                y = np.full(m, fill)
                assert L.spmv_fetch_y(h, y.ctypes.data) == 0, L.spmv_last_error()
                return y
            assert L.spmv_execute(h, x.ctypes.data, None, sp.Y_STAGED) == 0, L.spmv_last_error()
            self.check_host(f"staged y, fetch, fill {fill}", fetch())
            y2 = np.full(m, fill)
            assert L.spmv_execute(h, None, y2.ctypes.data, sp.X_STAGED) == 0, L.spmv_last_error()
            self.check_host(f"staged x, host y, fill {fill}", y2)
            # a second host x: the stage must hold the latest upload, not the first
            assert L.spmv_execute(h, x_b.ctypes.data, None, sp.Y_STAGED) == 0, L.spmv_last_error()
            assert L.spmv_execute(h, None, None, sp.X_STAGED | sp.Y_STAGED) == 0, L.spmv_last_error()
            self.check_host(f"staged x and y after a second upload, fill {fill}", fetch(), alpha=-2.0, scaled_x=True)

    # ---- 5. spmv_time: y is one execute's, not an accumulation
    def time(self):
        for fill in Y_FILLS:
            ybuf, yv = self.y(1, fill)
            assert self.plan.time(self.x[1][1], yv, 3) > 0
            self.check(f"time 3 iterations, fill {fill}", ybuf, 1, 1)

    # ---- 6. spmv_profile: the same y, the documented phase names
    def profile(self):
        L, h = sp.lib(), self.plan._h
        want = PHASES[self.info["format"]]
        ybuf, yv = self.y(1, Y_FILLS[0])
        prof = self.plan.profile(self.x[1][1], yv, 2)
        self.check(f"profile 2 iterations, fill {Y_FILLS[0]}", ybuf, 1, 1)
        assert list(prof) == list(dict.fromkeys(want)) and all(v >= 0 for v in prof.values()), (self.what, prof)
        ybuf, yv = self.y(1, Y_FILLS[1])
        ms, nph = (C.c_double * 8)(), C.c_int32()
        st = L.spmv_profile(h, C.c_void_p(self.x[1][1].data_ptr()), C.c_void_p(yv.data_ptr()), 2, ms, 8, C.byref(nph))
        assert st == 0, L.spmv_last_error()
        self.check(f"profile 2 iterations, fill {Y_FILLS[1]}", ybuf, 1, 1)
        names = [L.spmv_phase_name(h, k).decode() for k in range(nph.value)]
        assert names == want, f"{self.what} [profile]: phases {names}, documented {want}"
        assert L.spmv_phase_name(h, nph.value).decode() == ""

    # ---- 7. HIP graph of two executes, launched twice
    def graph(self):
        ybuf, yv = self.y(1, Y_FILLS[0])
        if self.info["format"] == "css":
            with pytest.raises(sp.SpmvError, match="not supported"):
                self.plan.graph(self.x[1][1], yv, reps=2)
            self.ran.append("graph")  # the documented refusal and nothing else
            return
        g = self.plan.graph(self.x[1][1], yv, reps=2)
        try:
            for k, fill in enumerate(Y_FILLS):
                yv.fill_(fill)
                self.torch.cuda.synchronize()
                g.launch()
                self.check(f"graph launch {k + 1} fill {fill}", ybuf, 1, 1)
        finally:
            g.destroy()

    # ---- 8. the k = 1, ld = 1 multi execute runs the plan's kernels in place
    def multi(self):
        X = self.x[1][1].view(self.n, 1)
        for fill in Y_FILLS:
            ybuf, yv = self.y(1, fill)
            Y = yv.view(self.m, 1)
            assert X.data_ptr() % 16 == 8 and Y.data_ptr() % 16 == 8
            assert self.plan.multi_path(X, Y) == [1]
            self.plan.execute_multi(X, Y)
            self.check(f"multi k=1 in place fill {fill}", ybuf, 1, 1)


@pytest.mark.parametrize("name,cid,fmt,kw", CASES)
def test_routes(name, cid, fmt, kw, request):
    c = gb.case(name)
    what = request.node.callspec.id
    if (name, cid) in EXPECTED_REFUSALS:  # the refusal itself is the test: nothing skips
        with pytest.raises(sp.SpmvError, match="not supported"):
            sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw).destroy()
        print(f"routes {what} refused by the builder, as expected")
        return
    plan = sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], fmt, **kw)  # any refusal here fails
    try:
        info = plan.info()
        _assert_path(name, fmt, kw, info, np.diff(c["rp"]))
        r = _Routes(plan, c, what)
        worst = si.assert_rows(r.y_base, c["rp"], c["col"], c["val"], c["x"], f"{what} [baseline]", ref=c["ref"])
        if si.plan_is_sequential(info):
            assert np.array_equal(mi.bits(r.y_base), mi.bits(c["y_oracle"])), \
                f"{what} [baseline]: {info['format']} is sequential, must equal the sequential sum bit for bit"
        r.device()
        r.stream()
        r.alpha()
        r.staged()
        r.time()
        r.profile()
        r.graph()
        r.multi()
        r.torch.cuda.synchronize()
        assert r.ran == ["device", "stream", "alpha", "staged", "time", "profile", "graph", "multi"], r.ran
        print(f"routes {what} format={info['format']} kernel={info['kernel']} err/row_tol={worst:.3f} "
              f"routes={','.join(r.ran)}")
    finally:
        plan.destroy()
