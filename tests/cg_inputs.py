"""Inputs and the reference for Plan.cg (spmv_cg_solve: conjugate gradients
on a plan, the scalars on the device).

Seeded symmetric positive definite cases, none a multiple of 64 rows:

    rand8    m = 3001, 8 symmetric random off-diagonals per row (4 drawn per
             row, mirrored), diagonal = 1.25 * sum |off| + 0.5
    skew     m = 4099, 4 per row (2 drawn, mirrored) plus one hub row and
             column of about 3000 entries, same diagonal rule: adaptive CSR
             bins, HYB / JDS overflow rows, BIN's long rows
    lap2d    the 61 x 53 five-point grid, diagonal 4.05
    lap1d    m = 5003 tridiagonal, diagonal 4.01
    tiny1    m = 1;  tiny65: m = 65, tridiagonal;  tiny130: m = 130, tridiagonal
             (the one even m: the vector kernels have no odd last row)

The diagonal rule makes every matrix strictly diagonally dominant with a
positive diagonal, hence positive definite.

ref_cg is the library's iteration in NumPy, recurrence for recurrence
(include/spmv_hip.h): alpha = rz / pq, x += alpha p, r -= alpha q, z = dinv r,
beta = rz_new / rz, p = z + beta p, the stop rr <= rtol^2 bb tested before the
first iteration too, breakdown unless pq is a finite number > 0 -- in float64
or in longdouble.  What a plan does differently is the order of the adds in
its row sums and dot products.

reference(name, use_dinv) records, at RTOL = 1e-10 from the case's x0:
ref_iters (float64 iterations to converge), true_relres of that solve
(|b - A x| / |b| with a longdouble matvec), x5 (the longdouble iterate after
exactly FIXED = 5 iterations) and d_ref, the relative distance of the float64
iterate after 5 iterations from x5: the reference's own rounding error, the
yardstick of tests/test_gpu_cg.py.

Plain helper module (numpy only); tests/test_cg_inputs.py checks it on the
CPU, tests/test_gpu_cg.py uses it on the GPU.
"""
import functools

import numpy as np

RTOL = 1e-10
FIXED = 5
CONVERGED, MAX_ITERS, BREAKDOWN = "converged", "max_iters", "breakdown"
NAMES = ("rand8", "skew", "lap2d", "lap1d", "tiny1", "tiny65", "tiny130")


def bits(a):
    """The int64 patterns of a float64 array (NaN payloads and signed zeros count)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---------------------------------------------------------------- matrices
def _csr(m, rows, cols, vals):
    """CSR (int64 rp, int32 col ascending within a row, float64 val) of COO
    entries; duplicates are added."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    vals = np.asarray(vals, np.float64)
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    first = np.ones(len(rows), bool)
    first[1:] = (rows[1:] != rows[:-1]) | (cols[1:] != cols[:-1])
    start = np.flatnonzero(first)
    vals = np.add.reduceat(vals, start) if len(start) else vals
    rows, cols = rows[start], cols[start]
    rp = np.zeros(m + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), cols.astype(np.int32), np.ascontiguousarray(vals)


def _dominant(m, r, c, v):
    """The symmetric matrix with off-diagonals (r, c, v) and (c, r, v), and the
    diagonal 1.25 * sum |off| + 0.5 of the merged rows."""
    keep = r != c
    r, c, v = r[keep], c[keep], v[keep]
    rp, col, val = _csr(m, np.concatenate([r, c]), np.concatenate([c, r]), np.concatenate([v, v]))
    row = np.repeat(np.arange(m), np.diff(rp))
    off = np.zeros(m)
    np.add.at(off, row, np.abs(val))
    d = np.arange(m)
    return _csr(m, np.concatenate([row, d]), np.concatenate([col.astype(np.int64), d]),
                np.concatenate([val, 1.25 * off + 0.5]))


def _random_sym(m, per_row, seed, hub=0):
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(m), per_row)
    c = rng.integers(0, m, len(r))
    v = rng.uniform(-1.0, 1.0, len(r))
    if hub:
        hc = rng.choice(np.arange(1, m), hub, replace=False)  # mirrored: row 0 and column 0
        r = np.concatenate([r, np.zeros(len(hc), np.int64)])
        c = np.concatenate([c, hc])
        v = np.concatenate([v, rng.uniform(-1.0, 1.0, len(hc))])
    return _dominant(m, r, c, v)


def _stencil(m, offsets, diag):
    """-1 at the given (row, col) pairs both ways, `diag` on the diagonal."""
    r = np.concatenate([o[0] for o in offsets])
    c = np.concatenate([o[1] for o in offsets])
    d = np.arange(m)
    return _csr(m, np.concatenate([r, c, d]), np.concatenate([c, r, d]),
                np.concatenate([-np.ones(2 * len(r)), np.full(m, diag)]))


def _tridiagonal(m, diag):
    i = np.arange(m - 1)
    return _stencil(m, [(i, i + 1)], diag)


def _lap2d(nx, ny, diag):
    idx = np.arange(nx * ny).reshape(ny, nx)
    return _stencil(nx * ny, [(idx[:, :-1].ravel(), idx[:, 1:].ravel()), (idx[:-1, :].ravel(), idx[1:, :].ravel())],
                    diag)


_BUILD = {
    "rand8": lambda: (3001,) + _random_sym(3001, 4, 11),
    "skew": lambda: (4099,) + _random_sym(4099, 2, 12, hub=3000),
    "lap2d": lambda: (61 * 53,) + _lap2d(61, 53, 4.05),
    "lap1d": lambda: (5003,) + _tridiagonal(5003, 4.01),
    "tiny1": lambda: (1,) + _csr(1, [0], [0], [2.5]),
    "tiny65": lambda: (65,) + _tridiagonal(65, 4.01),
    "tiny130": lambda: (130,) + _tridiagonal(130, 4.01),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """m, rp, col, val, row (of every entry), diag, dinv = 1 / diag, b and x0
    (seeded, U(-1, 1)).  Computed once, shared, read-only."""
    m, rp, col, val = _BUILD[name]()
    row = np.repeat(np.arange(m, dtype=np.int64), np.diff(rp))
    diag = np.zeros(m)
    on = row == col
    diag[row[on]] = val[on]
    rng = np.random.default_rng(500 + NAMES.index(name))
    c = {"name": name, "m": m, "n": m, "rp": rp, "col": col, "val": val, "row": row, "diag": diag,
         "dinv": 1.0 / diag, "b": rng.uniform(-1.0, 1.0, m), "x0": rng.uniform(-1.0, 1.0, m)}
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def is_symmetric(c):
    """Pattern and values: the transposed entry list is the entry list."""
    a = np.lexsort((c["col"], c["row"]))
    t = np.lexsort((c["row"], c["col"]))
    return (np.array_equal(c["row"][a], c["col"][t]) and np.array_equal(c["col"][a], c["row"][t])
            and np.array_equal(bits(c["val"][a]), bits(c["val"][t])))


# ---------------------------------------------------------------- the reference
def matvec(c, x, dtype=np.float64, scale=1.0):
    """(scale * A) x with every product and sum in `dtype`, rows added in column order."""
    x = np.asarray(x, dtype)
    prod = (c["val"].astype(dtype) * dtype(scale)) * x[c["col"]]
    return np.add.reduceat(prod, c["rp"][:-1])  # every row holds its diagonal: none is empty


def ref_cg(c, b, x0, dinv, rtol, max_iters, dtype=np.float64, scale=1.0):
    """The iteration of spmv_cg_solve on (scale * A) in `dtype`: (x, info) with
    info = status, iterations, rr, bb, rz, pq as Plan.cg reports them."""
    T = dtype
    b, x = np.asarray(b, T), np.array(x0, T)
    d = None if dinv is None else np.asarray(dinv, T)
    rtol2 = T(rtol) * T(rtol)
    r = b - matvec(c, x, T, scale)
    z = r if d is None else d * r
    p = z.copy()
    rz, rr, bb, pq = np.sum(r * z), np.sum(r * r), np.sum(b * b), T(0.0)
    it = 0
    status = CONVERGED if rr <= rtol2 * bb else MAX_ITERS if max_iters == 0 else None
    while status is None:
        q = matvec(c, p, T, scale)
        pq = np.sum(p * q)
        if not (pq > 0 and np.isfinite(pq)):
            status = BREAKDOWN
            break
        alpha = rz / pq
        x = x + alpha * p
        r = r - alpha * q
        z = r if d is None else d * r
        rz_new, rr = np.sum(r * z), np.sum(r * r)
        beta = rz_new / rz
        rz = rz_new
        it += 1
        if rr <= rtol2 * bb:
            status = CONVERGED
        elif it == max_iters:
            status = MAX_ITERS
        else:
            p = z + beta * p
    return x, {"status": status, "iterations": it, "rr": rr, "bb": bb, "rz": rz, "pq": pq}


def true_relres(c, x, b, scale=1.0):
    """|b - (scale * A) x| / |b| with the matvec, the difference and the norms in longdouble."""
    L = np.longdouble
    r = np.asarray(b, L) - matvec(c, x, L, scale)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(np.asarray(b, L) ** 2)))


def rel_distance(x, ref):
    """|x - ref| / |ref| in longdouble (ref: a longdouble vector)."""
    L = np.longdouble
    d = np.asarray(x, L) - np.asarray(ref, L)
    return float(np.sqrt(np.sum(d * d)) / np.sqrt(np.sum(np.asarray(ref, L) ** 2)))


@functools.lru_cache(maxsize=None)
def reference(name, use_dinv):
    """ref_iters, true_relres, x5 and d_ref of a case from its x0 (module docstring)."""
    c = case(name)
    dinv = c["dinv"] if use_dinv else None
    x, info = ref_cg(c, c["b"], c["x0"], dinv, RTOL, 1000)
    x5, _ = ref_cg(c, c["b"], c["x0"], dinv, 0.0, FIXED, np.longdouble)
    x5_64, info5 = ref_cg(c, c["b"], c["x0"], dinv, 0.0, FIXED)
    x5.setflags(write=False)
    return {"status": info["status"], "ref_iters": info["iterations"], "true_relres": true_relres(c, x, c["b"]),
            "recurred_relres": float(np.sqrt(info["rr"] / info["bb"])), "x5": x5, "status5": info5["status"],
            "d_ref": rel_distance(x5_64, x5)}
