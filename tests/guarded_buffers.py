"""Guarded, offset x / y buffers and the checker of every execute route.

The parity tests say what the kernels compute; this module is about where
they read and write.  A vector lives inside a wider buffer with GUARD doubles
on each side: the x guards hold NaN (a guard value that reaches any sum, even
with weight 0, makes the row NaN), the y guards hold multi_inputs.SENTINEL and
are compared bit for bit afterwards.  GUARD = 512 is the largest row block one
workgroup of any kernel owns (DIA's kDiaBlockRows): a workgroup that is off by
a whole block still lands inside the guard.  The view starts GUARD + off
doubles into a 16-byte-aligned buffer, so it is 16-byte aligned (off 0) or
sits at an 8-byte offset (off 1), as a torch slice buf[1:] does.

`stair_tail` is rows 7..2047 of signed_inputs' staircase (columns unchanged):
m = 2041 = 13 * 157 rows -- odd, no multiple of 64, 256 or 512 -- with the
9000-entry row as the matrix's last row, where an overrun would happen.

check_route holds what every route (device pointers, streams, alpha, staged
x / y, time, profile, graphs, the k = 1 multi execute) must satisfy: the y of
the plan's host execute bit for bit, untouched guards.  No tolerance of its
own: COO's split rows are held to signed_inputs.row_tol.

Plain helper module (numpy only; torch is imported by guarded_device alone);
tests/test_guarded_buffers.py checks it on the CPU, tests/test_gpu_routes.py
uses it on the GPU.
"""
import functools
import math

import numpy as np

import multi_inputs as mi
import signed_inputs as si

GUARD = 512  # doubles on each side of a vector: DIA's 512-row workgroup block
X_FILL = float("nan")
Y_FILL = mi.SENTINEL

STAIR_TAIL = "stair_tail"
STAIR_TAIL_ROW0 = 7  # the first staircase row kept


# ---------------------------------------------------------------- buffers
def guarded(n, off, fill):
    """(buffer, view), numpy: a buffer of GUARD + off + n + GUARD doubles, all
    `fill`, whose base is 16-byte aligned, and its view of the n doubles that
    start GUARD + off doubles in (off 0: 16-byte aligned, off 1: 8 bytes past)."""
    assert off in (0, 1) and n >= 1
    total = 2 * GUARD + off + n
    raw = np.full(total + 1, fill, np.float64)
    buf = raw[1:] if raw.ctypes.data % 16 else raw[:total]
    view = buf[GUARD + off:GUARD + off + n]
    assert buf.ctypes.data % 16 == 0 and view.ctypes.data % 16 == 8 * off
    return buf, view


def guarded_device(n, off, fill):
    """(buffer, view) as torch CUDA tensors, laid out as guarded()'s."""
    import torch
    assert off in (0, 1) and n >= 1
    buf = torch.full((2 * GUARD + off + n,), fill, dtype=torch.float64, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 8 * off
    return buf, view


def to_host(a):
    """A numpy copy of a numpy array or torch tensor."""
    return np.array(a, np.float64) if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def used(buffer, n, off):
    """The n used doubles of a guarded buffer, on the host."""
    return np.ascontiguousarray(to_host(buffer)[GUARD + off:GUARD + off + n])


def guard_damage(buffer, n, off, fill):
    """Indices, relative to the view's first element (negative: the guard
    before, >= n: the guard after), of the guard words that no longer hold
    `fill` bit for bit."""
    b = mi.bits(to_host(buffer))
    assert len(b) == 2 * GUARD + off + n, "not a guarded() buffer of this n and off"
    want = mi.bits(np.array([fill]))[0]
    lo, hi = GUARD + off, GUARD + off + n
    bad = np.concatenate([np.flatnonzero(b[:lo] != want), hi + np.flatnonzero(b[hi:] != want)])
    return (bad - lo).tolist()


def guards_intact(buffer, n, off, fill):
    """Both guards of a guarded() / guarded_device() buffer still hold `fill`, bit for bit."""
    return not guard_damage(buffer, n, off, fill)


# ---------------------------------------------------------------- stair_tail
@functools.lru_cache(maxsize=None)
def structure(name):
    """(m, n, rp, col): stair_tail, or one of signed_inputs.STRUCTURES."""
    if name != STAIR_TAIL:
        return si.structure(name)
    m, n, rp, col = si.structure("staircase")
    r0 = STAIR_TAIL_ROW0
    rp2 = np.ascontiguousarray(rp[r0:] - rp[r0])
    col2 = np.ascontiguousarray(col[rp[r0]:])
    for a in (rp2, col2):
        a.setflags(write=False)
    return m - r0, n, rp2, col2


@functools.lru_cache(maxsize=None)
def case(name, family="cancel"):
    """signed_inputs.case(name, family), or stair_tail with that family's
    values -- same keys, computed once, read-only."""
    if name != STAIR_TAIL:
        return si.case(name, family)
    import oracle
    m, n, rp, col = structure(name)
    val, x = si.FAMILIES[family](rp, col, n, seed=700 + sorted(si.FAMILIES).index(family))
    c = {"name": name, "family": family, "m": m, "n": n, "rp": rp, "col": col, "val": val, "x": x,
         "row": np.repeat(np.arange(m, dtype=np.int32), np.diff(rp)), "ref": si.ref_rows(rp, col, val, x),
         "y_oracle": oracle.csr_spmv(rp, col, np.ascontiguousarray(val), np.ascontiguousarray(x))}
    for a in (val, x, c["row"], c["y_oracle"]) + c["ref"]:
        a.setflags(write=False)
    return c


# ---------------------------------------------------------------- the checker
def coo_inside(rp):
    """Rows of a COO plan whose y is the same on every run: the empty rows
    (zeroed) and the rows inside one 128-entry unit (exactly one atomic add)."""
    rp = np.asarray(rp, np.int64)
    return (np.diff(rp) == 0) | (rp[:-1] // 128 == (rp[1:] - 1) // 128)


def expected(y_base, alpha=1.0, scaled_x=False):
    """The y a route must give: alpha * y_base as numpy computes it (one
    rounded multiply per row; alpha = 1: y_base itself).  scaled_x: the route
    did not scale y, it ran on alpha * x (alpha a power of two, so every
    product and sum scales exactly) -- a row whose sum is 0 (no entries, or
    exact cancellation) is then +0.0 again, not alpha * 0.0."""
    y_base = np.asarray(y_base, np.float64)
    if alpha == 1.0:
        return y_base
    want = np.float64(alpha) * y_base
    if scaled_x:
        assert _exact_scale(alpha) and alpha != 0.0
        want[y_base == 0] = y_base[y_base == 0]
    return want


def _exact_scale(alpha):
    """alpha * v is exact for every v of the test data: 0 or +-2^k."""
    return alpha == 0.0 or math.frexp(abs(alpha))[0] == 0.5


def check_route(y, y_base, case, info, what, alpha=1.0, scaled_x=False, guards=()):
    """What every execute route must satisfy.

    guards: (label, buffer, n, off, fill) of every guarded buffer the route
    was handed -- both guards of each must hold their fill bit for bit.
    y (the m used entries) must equal expected(y_base, alpha) bit for bit.
    COO plans (unordered f64 atomics): the rows of coo_inside bit for bit; the
    rows split across units within signed_inputs.row_tol of case["ref"] --
    under an alpha whose multiply is exact (0, +-2^k) against alpha * y_hi
    with |alpha| * row_tol, the same derived bound; under any other alpha the
    split rows are not compared."""
    for label, buffer, n, off, fill in guards:
        bad = guard_damage(buffer, n, off, fill)
        assert not bad, (f"{what}: the {label} guards were written at {bad[:8]} relative to the vector "
                         f"({len(bad)} words; {n} used, offset {off})")
    y = np.asarray(y, np.float64)
    m, rp = case["m"], case["rp"]
    assert y.shape == (m,) and np.shape(y_base) == (m,), f"{what}: y has shape {y.shape}, the plan {m} rows"
    want = expected(y_base, alpha, scaled_x)
    differs = mi.bits(y) != mi.bits(want)
    if info["format"] != "coo":
        rows = np.flatnonzero(differs)
        assert not len(rows), (f"{what}: {len(rows)} rows differ from the expected y, first {rows[:5].tolist()}: "
                               f"{y[rows[:3]].tolist()} vs {want[rows[:3]].tolist()}")
        return
    rows = np.flatnonzero(differs & coo_inside(rp))
    assert not len(rows), (f"{what}: {len(rows)} COO rows inside one unit (or empty) differ, first "
                           f"{rows[:5].tolist()}: {y[rows[:3]].tolist()} vs {want[rows[:3]].tolist()}")
    if _exact_scale(alpha):
        y_hi, mag = case["ref"]
        a = np.longdouble(alpha)
        bad, ratio = si.failing_rows(y, rp, (a * y_hi, abs(a) * mag))
        assert not len(bad), (f"{what}: {len(bad)} COO rows beyond |alpha| row_tol, first {bad[:5].tolist()}, "
                              f"worst err/tol {ratio[bad].max():.3g}")
