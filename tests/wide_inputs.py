"""Tiny matrices over a very wide x: the inputs that put every format on the
far side of its 32-bit / 64-bit x addressing switch.

The kernels form the byte offset of x[c] in 32 bits while x stays below 4 GiB
and in 64 bits beyond.  The switch sits at n = 2^29 (WIDE) in

    formats.cpp  csr_plan_lanes     c.off32 = slab_max + 512 < 2^28 && p->n < 2^29
    k_ell.hip    ell_o32(p, ldx)    p->n * ldx < 2^29 && ldx < 2^28 && max_width * 64 * 8 < 2^31

(ldx = 1 for the single vector; the fused multi-vector launch reaches it at
n = 2^26 for ldx = 8, MULTI_WIDE).  A wrong offset does not
fault: it reads x[c mod 2^29] and returns a finite, plausible y.  Only x has to
be big to get there, so the matrices here have about 4 000 rows and at most
about 150 k entries.

Compact, then spread.  No n doubles are ever allocated on the host.  A case is
generated on the columns it can reach,

    ucol = unique(reach columns)     special_values.reach of the exact, the
                                     padded and (banded structures) the DIA
                                     layout together: the rows' own columns,
                                     column 0 for the empty rows, DIA's clamp
                                     targets
    ccol = searchsorted(ucol, col)   monotone: every row keeps its column
                                     order and its duplicates

with val and the compact x_c from signed_inputs' `cancel` family on (rp, ccol,
len(ucol)).  The sequential reference is oracle.csr_spmv(rp, ccol, val, x_c),
the per-row bound signed_inputs.ref_rows / row_tol / assert_rows on the compact
arrays, unchanged.  The device x is NaN over all n entries with x[ucol] = x_c:
a read of any column outside the reach poisons its row wherever the wrapped
address lands -- no tolerance involved, the contract special_values states
(pad and dummy slots are dropped by selects, never multiplied).

Plain helper module (numpy only, besides signed_inputs, special_values and the
oracle; torch only inside the two device builders);
tests/test_wide_inputs.py checks it on the CPU, tests/test_gpu_wide_x.py uses
it on the GPU.
"""
import functools

import numpy as np

import signed_inputs as si
import special_values as sv

WIDE = 1 << 29  # x reaches 4 GiB: the three guards quoted above
NS = (WIDE - 1,         # the last 32-bit case: the last column's byte offset is 2^32 - 16
      WIDE,             # the first 64-bit case; every offset still fits 32 bits
      WIDE + 4099,      # offsets truly beyond 2^32; n is odd
      2 * WIDE + 4099,  # columns beyond 2^30
      4 * WIDE - 2)     # the API's largest n
MULTI_WIDE = WIDE // 8  # the fused ELL / JDS switch at ldx = 8
MULTI_NS = (MULTI_WIDE - 1, MULTI_WIDE, MULTI_WIDE + 4099)
CPU_N = 1 << 22  # a full host x is cheap here (tests/test_wide_inputs.py)

M = 4003  # rows: odd, no multiple of 64, 256 or 512
CLUSTER = 2048
END = 4096
STRUCTURES = ("far_uniform", "far_band", "two_bands", "far_long")
UNSORTED = "far_long_unsorted"  # the device builders' sort paths only
BANDED = ("far_band", "two_bands")  # the structures DIA is built on
BAND = 8  # diagonals -BAND..BAND
LONG_ROWS = si.STAIR_LONG  # row: entries
EMPTY_FRAC = 1.0 / 11.0


# ---------------------------------------------------------------- structures
def clusters(n):
    """[lo, hi) column ranges: 2048 columns at 0, around 2^28, 2^29 and 2^30
    (those that fit below the last one), and the end [n - 4096, n)."""
    assert n >= 4 * END
    out = [(0, CLUSTER)]
    for p in (28, 29, 30):
        lo = (1 << p) - CLUSTER // 2
        if lo >= CLUSTER and lo + CLUSTER <= n - END:
            out.append((lo, lo + CLUSTER))
    out.append((n - END, n))
    return out


def _pool(n):
    return np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in clusters(n)])


def _emptied(rp, col, keep_rows, seed):
    """signed_inputs.with_empty_rows at 1 / 11, with the first seed from
    `seed` on that leaves keep_rows alone."""
    lens = np.diff(rp)
    for s in range(seed, seed + 1000):
        rp2, col2, _ = si.with_empty_rows(rp, col, np.zeros(len(col)), EMPTY_FRAC, s)
        if (np.diff(rp2)[keep_rows] == lens[keep_rows]).all():
            return rp2, col2
    raise AssertionError("no seed keeps the rows")


def _from_rows(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rp, np.concatenate(rows).astype(np.int64)


def _far_uniform(n, rng):
    """16 distinct ascending entries per row, each from one of the clusters;
    every row touches the first and the last cluster, every fifth row columns
    0 and n - 1."""
    cl, pool = clusters(n), _pool(n)
    rows = []
    for r in range(M):
        first = 0 if r % 5 == 0 else rng.integers(*cl[0])
        last = n - 1 if r % 5 == 0 else rng.integers(*cl[-1])
        while True:
            c = np.unique(np.concatenate([[first, last], pool[rng.choice(len(pool), 14, replace=False)]]))
            if len(c) == 16:
                break
        rows.append(c)
    return _from_rows(rows)


def _band(n, base):
    r = np.repeat(np.arange(M, dtype=np.int64), 2 * BAND + 1)
    c = r + base + np.tile(np.arange(-BAND, BAND + 1, dtype=np.int64), M)
    keep = (c >= 0) & (c < n)
    return r[keep], c[keep]


def _far_band(n, rng):
    """17 diagonals col = r + B + d, d in -8..8, B = n - M - 8: a band parked
    at the far end of a rectangular M x n matrix (row M - 1 ends at column
    n - 1, nothing is clipped; with the last five rows emptied the last
    stored entry is column n - 6)."""
    r, c = _band(n, n - M - BAND)
    assert len(c) == M * (2 * BAND + 1) and c.max() == n - 1
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]).astype(np.int64), c


def _two_bands(n, rng):
    """far_band plus the same 17 diagonals at col = r + d, clipped at 0: 34
    diagonals whose x window is far beyond what the LDS holds."""
    r0, c0 = _band(n, 0)
    r1, c1 = _band(n, n - M - BAND)
    r, c = np.concatenate([r0, r1]), np.concatenate([c0, c1])
    o = np.lexsort((c, r))
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=M))]).astype(np.int64), c[o]


def _far_long(n, rng):
    """Power-law row lengths 1..700 plus the three rows of
    signed_inputs.STAIR_LONG (4096, 4097 and 9000 entries, columns with
    duplicates), columns spread over all clusters, ascending."""
    pool = _pool(n)
    lens = np.minimum(700, 1 + np.floor(3.0 * rng.pareto(1.0, M))).astype(np.int64)
    lens[7], lens[8], lens[9] = 700, 129, 128
    rows = []
    for r in range(M):
        if r in LONG_ROWS:
            rows.append(np.sort(pool[rng.integers(0, len(pool), LONG_ROWS[r])]))
        else:
            rows.append(np.sort(pool[rng.choice(len(pool), int(lens[r]), replace=False)]))
    return _from_rows(rows)


def _unsorted(rp, col, rng):
    """The rows of (rp, col) out of column order, every third row of >= 2
    entries with one column repeated."""
    col = col.copy()
    for r in range(len(rp) - 1):
        a, b = int(rp[r]), int(rp[r + 1])
        if b - a >= 2:
            col[a:b] = col[a:b][rng.permutation(b - a)]
            if r % 3 == 0:
                col[a + int(rng.integers(1, b - a))] = col[a]
    return col


_KEEP = {"far_uniform": [5, 10], "far_band": [5], "two_bands": [5], "far_long": [7, 8, 9] + sorted(LONG_ROWS)}


@functools.lru_cache(maxsize=None)
def structure(name, n):
    """(m, n, rp, col) of one named structure at width n: about every 11th
    row empty, col int64, ascending within each row except in
    far_long_unsorted (arrays shared: do not write)."""
    if name == UNSORTED:
        m, _, rp, col = structure("far_long", n)
        out = m, n, rp, _unsorted(rp, col, np.random.default_rng(n % 1000003 + 77))
    else:
        k = STRUCTURES.index(name)
        rng = np.random.default_rng(n % 1000003 + 1000 * k)
        rp, col = {"far_uniform": _far_uniform, "far_band": _far_band, "two_bands": _two_bands,
                   "far_long": _far_long}[name](n, rng)
        rp, col = _emptied(rp, col, np.array(_KEEP[name]), seed=100 * k)
        out = M, n, rp, col
    assert int(out[2][-1]) <= 160_000 and out[3].min() >= 0 and out[3].max() < n
    for a in out[2:]:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- compact cases
def reach_columns(name, rp, col, m, n):
    """The sorted distinct columns any layout may multiply: the reach of the
    exact layouts, of the padded ones (column 0 for the empty rows) and, on
    the banded structures DIA is built on, of DIA (its clamp targets)."""
    kinds = ["csr", "ell"] + (["dia"] if name in BANDED else [])
    return np.unique(np.concatenate([sv.reach({"format": f}, rp, col, m, n)[1] for f in kinds]))


@functools.lru_cache(maxsize=None)
def case(name, n):
    """One structure at width n with the `cancel` family's values on its
    compact columns: col (int32, the wide columns the plan is built from),
    ucol, ccol, val, x_c, ref (signed_inputs.ref_rows on the compact arrays)
    and y_oracle (the oracle's sequential sums) -- computed once, read-only."""
    import oracle
    m, _, rp, col = structure(name, n)
    ucol = reach_columns(name, rp, col, m, n)
    ccol = np.searchsorted(ucol, col).astype(np.int32)
    names = STRUCTURES + (UNSORTED,)
    val, x_c = si.FAMILIES["cancel"](rp, ccol, len(ucol), seed=names.index(name) * 7 + n % 1000003)
    val, x_c = np.ascontiguousarray(val), np.ascontiguousarray(x_c)
    ref = si.ref_rows(rp, ccol, val, x_c)
    c = {"name": name, "m": m, "n": n, "rp": rp, "col": col.astype(np.int32), "col64": col, "ucol": ucol,
         "ccol": ccol, "val": val, "x_c": x_c, "ref": ref, "y_oracle": oracle.csr_spmv(rp, ccol, val, x_c)}
    return sv._freeze(c)


@functools.lru_cache(maxsize=None)
def column(name, n, j):
    """Column j of the case's multi-vector X on the compact columns, with its
    references: column 0 is the case's own x_c, column j >= 1 an independent
    +-U(0.5, 2) draw seeded by j (as multi_inputs.column)."""
    import oracle
    c = case(name, n)
    if j == 0:
        return {"x_c": c["x_c"], "ref": c["ref"], "y_oracle": c["y_oracle"]}
    rng = np.random.default_rng(j)
    k = len(c["ucol"])
    x = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 2.0, k)
    return sv._freeze({"x_c": x, "ref": si.ref_rows(c["rp"], c["ccol"], c["val"], x),
                       "y_oracle": oracle.csr_spmv(c["rp"], c["ccol"], c["val"], x)})


# ---------------------------------------------------------------- sparse x
def sparse_x(ucol, x_c):
    """x as a lookup: x_c on ucol, NaN on every other column, without the n
    doubles -- what the NaN-filled device x holds."""
    table = dict(zip(ucol.tolist(), np.asarray(x_c).tolist()))

    def at(c):
        return np.array([table.get(int(v), np.nan) for v in np.asarray(c).ravel()]).reshape(np.shape(c))
    return at


def gathered_spmv(c, colmap):
    """The sequential row sums of a kernel that reads x[colmap(col)] in place
    of x[col], on the NaN-filled x of the case (colmap = identity: y_oracle)."""
    import oracle
    xg = np.ascontiguousarray(sparse_x(c["ucol"], c["x_c"])(colmap(c["col64"])))
    return oracle.csr_spmv(c["rp"], np.arange(len(xg), dtype=np.int32), c["val"], xg)


def wrap32(col):
    """A 32-bit byte offset: x[(c * 8 mod 2^32) / 8]."""
    return ((np.asarray(col, np.int64) * 8) % (1 << 32)) // 8


def wrap28(col):
    return np.asarray(col, np.int64) % (1 << 28)


def check_y(y, c, what, x_col=None):
    """What every wide test asks of a y: finite on every row and within
    signed_inputs.row_tol of the compact reference.  Returns err / row_tol."""
    ref = c["ref"] if x_col is None else x_col["ref"]
    x_c = c["x_c"] if x_col is None else x_col["x_c"]
    assert np.isfinite(y).all(), (f"{what}: {int((~np.isfinite(y)).sum())} rows read x outside the reach, "
                                  f"first {np.flatnonzero(~np.isfinite(y))[:5].tolist()}")
    return si.assert_rows(y, c["rp"], c["ccol"], c["val"], x_c, what, ref=ref)


# ---------------------------------------------------------------- device x
def device_x(n, ucol, x_c, device, out=None):
    """The device x: NaN over all n entries, x[ucol] = x_c (filled on the
    device; `out`: an n-entry tensor to fill instead of a new one)."""
    import torch
    x = torch.empty(n, dtype=torch.float64, device=device) if out is None else out
    x.fill_(float("nan"))
    x[torch.from_numpy(np.array(ucol)).to(device)] = torch.from_numpy(np.array(x_c)).to(device)
    return x


def device_X(n, ldx, ucol, cols, device, out=None):
    """The multi-vector block: n x ldx, NaN everywhere, rows ucol carrying the
    k columns of `cols` (len(ucol) x k); columns [k, ldx) stay NaN."""
    import torch
    X = torch.empty((n, ldx), dtype=torch.float64, device=device) if out is None else out
    X.fill_(float("nan"))
    k = cols.shape[1]
    assert k <= ldx
    X[torch.from_numpy(np.array(ucol)).to(device), :k] = torch.from_numpy(np.array(cols)).to(device)
    return X
