"""Inputs and references for the multi-vector execute (Plan.execute_multi,
Y[:, j] = A X[:, j]).

The k-column X of a case: column 0 is the family's own x (so the rows of the
`cancel` family cancel in it), column j >= 1 an independent +-U(0.5, 2) draw
seeded by j -- a column read in another column's place moves every row.  X
lives inside a wider buffer whose pad columns are NaN (a kernel reading past
its k columns poisons its sums); Y lives inside a buffer prefilled with a
sentinel (a kernel writing past its k columns, or leaving a used entry
unwritten, shows bit for bit).

Every column is judged on its own: signed_inputs.ref_rows / row_tol (the
derived bound, no new tolerance) and oracle.csr_spmv of that column alone.

Plain helper module (numpy only, besides signed_inputs and the oracle);
tests/test_multi_inputs.py checks it on the CPU, tests/test_gpu_multi.py uses
it on the GPU.
"""
import functools

import numpy as np

import signed_inputs as si

MULTI_MAX = 32
SENTINEL = -1.2345e300
WIDTHS = (8, 4, 2)  # fused block widths, tried greedily, widest first


def bits(a):
    """The int64 patterns of a float64 array (NaN payloads and signed zeros count)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------- the cut
def greedy_cut(k, widths=WIDTHS):
    """k columns cut into blocks of 8, 4 and 2, then single columns: every
    block of width >= 2 starts at an even column."""
    out, j = [], 0
    while j < k:
        w = next((c for c in widths if k - j >= c), 1)
        out.append(w)
        j += w
    return out


def expected_path(k, fused):
    """The width list spmv_multi_path must report: the greedy cut when the
    plan's blocks are fused, else k single columns."""
    return greedy_cut(k) if fused else [1] * k


# ---------------------------------------------------------------- matrices
def _diagonals(m, n, offsets):
    """CSR pattern with entries at (r, r + off) for every off inside the matrix."""
    r = np.repeat(np.arange(m, dtype=np.int64), len(offsets))
    c = r + np.tile(np.asarray(sorted(offsets), np.int64), m)
    keep = (c >= 0) & (c < n)
    lens = np.bincount(r[keep], minlength=m)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return m, n, rp, c[keep].astype(np.int32)


# name -> (m, n, offsets): three diagonals whose x window (512 + span + 1
# doubles per 512-row workgroup) is 3513 doubles (fits the LDS with 2 columns,
# not with 8) or 10513 doubles (two columns of it exceed the LDS)
TRIDIAGS = {"tri1500": (12001, 12001, (-1500, 0, 1500)), "tri5000": (12001, 12001, (-5000, 0, 5000))}


@functools.lru_cache(maxsize=None)
def case(name, family):
    """signed_inputs.case(name, family), or one of TRIDIAGS with that family's
    values -- same keys, computed once, read-only."""
    if name not in TRIDIAGS:
        return si.case(name, family)
    import oracle
    m, n, rp, col = _diagonals(*TRIDIAGS[name])
    val, x = si.FAMILIES[family](rp, col, n, seed=500 + sorted(TRIDIAGS).index(name))
    c = {"name": name, "family": family, "m": m, "n": n, "rp": rp, "col": col, "val": val, "x": x,
         "row": np.repeat(np.arange(m, dtype=np.int32), np.diff(rp)), "ref": si.ref_rows(rp, col, val, x),
         "y_oracle": oracle.csr_spmv(rp, col, np.ascontiguousarray(val), np.ascontiguousarray(x))}
    for a in (rp, col, val, x, c["row"], c["y_oracle"]) + c["ref"]:
        a.setflags(write=False)
    return c


# ---------------------------------------------------------------- columns
@functools.lru_cache(maxsize=None)
def column(name, family, j):
    """Column j of the case's X with its references: {"x", "ref" (ref_rows),
    "y_oracle" (the sequential sum)} -- computed once, read-only."""
    import oracle
    c = case(name, family)
    if j == 0:
        return {"x": c["x"], "ref": c["ref"], "y_oracle": c["y_oracle"]}
    rng = np.random.default_rng(j)
    x = rng.choice([-1.0, 1.0], c["n"]) * rng.uniform(0.5, 2.0, c["n"])
    ref = si.ref_rows(c["rp"], c["col"], c["val"], x)
    yo = oracle.csr_spmv(c["rp"], c["col"], np.ascontiguousarray(c["val"]), x) if c["m"] else np.zeros(0)
    for a in (x, yo) + ref:
        a.setflags(write=False)
    return {"x": x, "ref": ref, "y_oracle": yo}


def x_block(name, family, k, ldx):
    """(buffer, X): an (n, ldx) buffer, NaN in its pad columns [k, ldx), and
    its view X = buffer[:, :k] holding columns 0..k-1."""
    n = case(name, family)["n"]
    assert ldx >= k
    buf = np.full((n, ldx), np.nan)
    for j in range(k):
        buf[:, j] = column(name, family, j)["x"]
    return buf, buf[:, :k]


def y_block(m, k, ldy, fill=SENTINEL):
    """(buffer, Y): an (m, ldy) buffer filled with `fill` and its view Y = buffer[:, :k]."""
    assert ldy >= k
    buf = np.full((m, ldy), fill)
    return buf, buf[:, :k]


def pads_untouched(buf, k, fill=SENTINEL):
    """The pad columns [k, ld) of a y_block buffer still hold `fill`, bit for bit."""
    return bool((bits(buf[:, k:]) == bits(np.array([fill]))[0]).all())


def ld_for(k):
    """The row stride the fused DIA cases use: k + 2 for even k, k + 1 for odd k (even, > k)."""
    return k + 2 if k % 2 == 0 else k + 1
