"""Signed, cancelling test data and a per-row error bound that holds for it.

The parity tests on U(0,1] data measure error against |y_ref|; once a row
cancels that is meaningless (|y_ref| can be 1e-16 of sum |a x|).  Here the
reference is the row sum in extended precision and the bound is relative to
sum |a x|:

    row_tol_i = (len_i + 8) * 2^-53 * sum_j |a_ij x_j|

Derivation: any order of len rounded products and adds (fused or not) errs by
at most gamma_len * sum |a x|, gamma_n = n u / (1 - n u), u = 2^-53; the
extended-precision reference errs by at most (len + 1) * 2^-64 * sum |a x|.
(len + 8) u covers both for rows far longer than the 9000 entries used here,
so the bound holds for every summation order a format may take -- butterflies,
run pieces, atomics -- and for none that drops, doubles or mis-gathers an
entry of the `cancel` family.

Plain helper module (numpy only, besides the project's generators for three
of the structures); tests/test_signed_inputs.py checks it on the CPU,
tests/test_gpu_signed.py uses it on the GPU.
"""
import functools
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LONGDOUBLE_OK = np.finfo(np.longdouble).nmant >= 63  # x87 extended: 63, eps 1.08e-19


# ---------------------------------------------------------------- reference
def _segment_sums(p, rp):
    """Per-row sums of p; np.add.reduceat returns a wrong element for an
    empty segment, so only the non-empty rows' starts are handed to it."""
    lens = np.diff(rp)
    out = np.zeros(len(lens), p.dtype)
    ne = lens > 0
    if ne.any():
        out[ne] = np.add.reduceat(p, rp[:-1][ne])
    return out


def _ref_rows_longdouble(rp, col, val, x):
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than double here"
    p = val.astype(np.longdouble) * x[col].astype(np.longdouble)
    return _segment_sums(p, rp), _segment_sums(np.abs(p), rp)


def _to_longdouble(f):
    hi = float(f)
    return np.longdouble(hi) + np.longdouble(float(f - Fraction(hi)))


def _ref_rows_fraction(rp, col, val, x):
    """Exact row sums (where np.longdouble is only a double)."""
    m = len(rp) - 1
    y, mag = np.zeros(m, np.longdouble), np.zeros(m, np.longdouble)
    xf = [Fraction(float(v)) for v in x]
    for r in range(m):
        s = a = Fraction(0)
        for j in range(int(rp[r]), int(rp[r + 1])):
            t = Fraction(float(val[j])) * xf[int(col[j])]
            s += t
            a += abs(t)
        y[r], mag[r] = _to_longdouble(s), _to_longdouble(a)
    return y, mag


def ref_rows(rp, col, val, x):
    """(y_hi, mag): per-row sum a x and sum |a x| in extended precision."""
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val, np.float64)
    x = np.asarray(x, np.float64)
    if LONGDOUBLE_OK:
        return _ref_rows_longdouble(rp, col, val, x)
    return _ref_rows_fraction(rp, col, val, x)


def row_tol(rp, mag):
    """(len + 8) * 2^-53 * mag per row (derived in the module docstring)."""
    lens = np.diff(np.asarray(rp, np.int64))
    return (lens + 8).astype(np.longdouble) * np.longdouble(U) * mag


def failing_rows(y, rp, ref):
    """(rows with |y - y_hi| > row_tol or a non-finite y, err / tol per row);
    ref = ref_rows(...).  A row with mag == 0 passes only with y == 0."""
    y_hi, mag = ref
    tol = row_tol(rp, mag)
    err = np.abs(np.asarray(y, np.float64).astype(np.longdouble) - y_hi)
    ok = err <= tol  # False for NaN
    ratio = np.full(len(err), np.inf)
    pos = tol > 0
    ratio[pos] = (err[pos] / tol[pos]).astype(np.float64)
    ratio[~pos & ok] = 0.0
    ratio[np.isnan(ratio)] = np.inf
    return np.flatnonzero(~ok), ratio


def assert_rows(y, rp, col, val, x, what, ref=None):
    """|y - y_hi| <= row_tol on every row; reports the worst row, its length
    and its err / tol.  Returns the largest err / tol (a measurement)."""
    if ref is None:
        ref = ref_rows(rp, col, val, x)
    bad, ratio = failing_rows(y, rp, ref)
    if len(bad):
        w = int(bad[np.argmax(ratio[bad])])
        lens = np.diff(np.asarray(rp, np.int64))
        raise AssertionError(f"{what}: {len(bad)} rows beyond row_tol, first {bad[:5].tolist()}; worst row {w} "
                             f"(len {int(lens[w])}): y {y[w]!r} vs {float(ref[0][w])!r}, err/tol {ratio[w]:.3g}")
    return float(ratio.max()) if len(ratio) else 0.0


# ---------------------------------------------------------------- value families
def spread(rp, col, n, seed):
    """val = +-U(0.5,1) 10^k, k in [-8, 8]; x = +-U(0.5,1) 10^j, j in [-4, 4]:
    a wide dynamic range (almost any change of add order changes bits), no
    underflow (the smallest product is about 1e-13)."""
    rng = np.random.default_rng(seed)
    nnz = int(rp[-1])
    val = rng.choice([-1.0, 1.0], nnz) * rng.uniform(0.5, 1.0, nnz) * 10.0 ** rng.integers(-8, 9, nnz)
    x = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * 10.0 ** rng.integers(-4, 5, n)
    return val, x


def cancel(rp, col, n, seed):
    """x = +-U(0.5,2); per row, targets t in +- pairs from U(0.5,2), shuffled
    within the row, val_j = t_j / x[col_j]: an even-length row sums to
    rounding noise while sum |a x| ~ len, and every entry has comparable size
    (one dropped, doubled or mis-gathered entry moves y by >= 0.5)."""
    rng = np.random.default_rng(seed)
    rp = np.asarray(rp, np.int64)
    nnz = int(rp[-1])
    x = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)
    lens = np.diff(rp)
    row = np.repeat(np.arange(len(lens)), lens)
    pos = np.arange(nnz) - np.repeat(rp[:-1], lens)
    u = rng.uniform(0.5, 2.0, nnz)
    t = u[np.arange(nnz) - (pos & 1)] * np.where(pos & 1, -1.0, 1.0)  # (t, -t) pairs; an odd row keeps one single
    t = t[np.argsort(row + rng.random(nnz))]  # shuffled within each row (row + U[0,1) keeps rows apart)
    val = t / x[np.asarray(col, np.int64)]
    return val, x


FAMILIES = {"spread": spread, "cancel": cancel}


# ---------------------------------------------------------------- structures
STAIR_LENS = (0, 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 700)
STAIR_LONG = {3: 4096, 1029: 4097, 2047: 9000}  # row: entries (columns with duplicates)


def with_empty_rows(rp, col, val, frac, seed):
    """The CSR with about frac of its rows (the first 3 and last 5 among
    them) emptied."""
    m = len(rp) - 1
    rng = np.random.default_rng(seed)
    lens = np.diff(rp)
    zero = rng.random(m) < frac
    zero[:3] = True
    zero[-5:] = True
    keep = np.repeat(~zero, lens)
    rp2 = np.concatenate([[0], np.cumsum(np.where(zero, 0, lens))]).astype(np.int64)
    return rp2, np.ascontiguousarray(col[keep]), np.ascontiguousarray(val[keep])


def _staircase():
    # the edges of csr_adaptive's eight length bins (<= 4 L for L = 1..32
    # lanes, <= 4096 for 64 lanes, a workgroup per row beyond); the 9000-entry
    # row spans > 35 SS tiles at sigma 4, ~70 COO units, the HYB / JDS
    # overflow, BIN's run path and CSS's split path
    m = n = 2048
    rng = np.random.default_rng(2048)
    lens = np.array([STAIR_LENS[r % len(STAIR_LENS)] for r in range(m)], np.int64)
    for r, k in STAIR_LONG.items():
        lens[r] = k
    cols = [np.sort(rng.integers(0, n, k)) if r in STAIR_LONG else np.sort(rng.choice(n, int(k), replace=False))
            for r, k in enumerate(lens)]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return m, n, rp, np.concatenate(cols).astype(np.int32)


def _generated(kind, m, **kw):
    import singlespmv_amd as sp
    rp, col, val = sp.generate_csr(sp.gen_spec(kind, m, **kw))
    return rp, col, val


def _short():
    # rows of 0-3 entries: an SS tile finishes 64-4096 rows (every tile-end
    # store path)
    m = 30011
    rng = np.random.default_rng(30011)
    lens = rng.integers(0, 4, m)
    cols = np.sort(rng.integers(0, m - 2, (m, 3)), axis=1) + np.arange(3)  # ascending, distinct, < m
    keep = np.arange(3)[None, :] < lens[:, None]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return m, m, rp, cols[keep].astype(np.int32)


def _rect(m, n):
    # the matrices of the csr_slabx small-shapes test: a few entries around
    # the (scaled) diagonal, every 11th row empty
    rng = np.random.default_rng(m * 7 + n)
    lens, cols = [], []
    for r in range(m):
        c = r * n // m
        cs = sorted({min(n - 1, max(0, c + d)) for d in range(-3, 4) if rng.random() < 0.8})
        if r % 11 == 5:
            cs = []
        lens.append(len(cs))
        cols += cs
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return m, n, rp, np.asarray(cols, np.int32)


STRUCTURES = ("staircase", "powerlaw", "uniform16", "banded", "short", "rect513x40", "rect7x1000")


@functools.lru_cache(maxsize=None)
def structure(name):
    """(m, n, rp, col) of one named structure (arrays shared: do not write)."""
    if name == "staircase":
        out = _staircase()
    elif name == "powerlaw":
        rp, col, val = with_empty_rows(*_generated("powerlaw", 20000, max_len=3000, seed=11), 0.1, 12)
        out = 20000, 20000, rp, col
    elif name == "uniform16":  # m no multiple of 64, 256 or 512
        rp, col, _ = _generated("uniform", 20011, per_row=16)
        out = 20011, 20011, rp, col
    elif name == "banded":  # rows clipped at both matrix edges
        rp, col, _ = _generated("banded", 20077, band_lo=-40, band_hi=40)
        out = 20077, 20077, rp, col
    elif name == "short":
        out = _short()
    elif name == "rect513x40":
        out = _rect(513, 40)
    elif name == "rect7x1000":
        out = _rect(7, 1000)
    else:
        raise KeyError(name)
    for a in out[2:]:
        a.setflags(write=False)
    return out


def structures():
    for name in STRUCTURES:
        yield (name,) + structure(name)


@functools.lru_cache(maxsize=None)
def case(name, family):
    """One structure with one family's values, its extended-precision
    reference and the oracle's sequential sums -- computed once, shared by
    every test that needs them, read-only."""
    import oracle
    m, n, rp, col = structure(name)
    val, x = FAMILIES[family](rp, col, n, seed=STRUCTURES.index(name) * 2 + sorted(FAMILIES).index(family) + 1)
    ref = ref_rows(rp, col, val, x)
    yo = oracle.csr_spmv(rp, col, np.ascontiguousarray(val), np.ascontiguousarray(x)) if m else np.zeros(0)
    row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))  # the sorted COO's row indices
    for a in (val, x, yo, row) + ref:
        a.setflags(write=False)
    return {"name": name, "family": family, "m": m, "n": n, "rp": rp, "row": row, "col": col, "val": val, "x": x,
            "ref": ref, "y_oracle": yo}


# ---------------------------------------------------------------- plans
def plan_is_sequential(info, dia_duplicates=False):
    """True when the plan (Plan.info()) sums every row in CSR order with one
    accumulator, i.e. must equal opt_crs bit for bit on rows in ascending
    column order: ELL, DIA (unless duplicate entries were added into one slot
    first), one-lane CSR, JDS without overflow, CSS without split rows, BIN
    without the long rows' run path."""
    f = info["format"]
    return (f == "ell" or (f == "dia" and not dia_duplicates) or (f == "csr" and info["csr_lanes"] == 1)
            or (f == "jds" and info["overflow_nnz"] == 0)
            or (f == "css" and info["css_split_rows"] == 0)
            or (f == "bin" and info["bin_long_len"] == 0))
