"""Non-finite x, subnormal products and products near 2^1000: inputs, the
columns a layout may multiply (`reach`) and the checkers for them.

Poisoned x.  On finite data a term the kernel should not have added --
mask * v instead of a select, a scan step across a segment boundary with
weight 0, a dummy slot read back -- is 0 * x[c] = 0 and invisible.  With
x[c] = NaN or +-Inf it is NaN and lands in a row that never referenced
column c, so a poisoned x detects cross-row and pad coupling without a
tolerance:

    every row whose columns meet a poisoned column is non-finite
        (with the class -- NaN, +Inf, -Inf -- of the sequential sum where
        the layout multiplies exactly the row's own entries);
    every row whose reach misses every poisoned column is bit for bit what
        the same plan gives on the clean x.

`reach` is what the resolved layout may multiply for row r:

    CSR (every kernel), SS, COO, CSS, BIN   cols(r)
    ELL, JDS, HYB                           cols(r), plus column 0 when r is empty
                                            (padding repeats the row's last real
                                            column, 0 for an empty row)
    DIA                                     clamp(r + off, 0, n - 1) over the stored
                                            diagonals off = unique(col - row)
                                            (zero-filled slots read a clamped x)

Extreme range.  `tiny` (val 2^-530, x 2^-535 scales: every product is
subnormal, every row sum of <= 9000 entries stays below 2^-1022) and `huge`
(2^500 each: products up to 2^1000, sums finite).  A rounded subnormal product
errs by <= 2^-1075; sums of subnormals are exact while the result stays
subnormal; the extended-precision reference has a 15-bit exponent and does not
underflow.  So

    tiny_tol_i = (len_i + 8) * 2^-1074

covers len products with a factor two to spare (and a fused multiply-add,
which rounds once per add to the same grid).  `huge` keeps
signed_inputs.row_tol, a relative bound.

Plain helper module (numpy only, besides signed_inputs);
tests/test_special_values.py checks it on the CPU, tests/test_gpu_special.py
uses it on the GPU.
"""
import functools

import numpy as np

import signed_inputs as si

POISON = (np.nan, np.inf, -np.inf)
EXACT_REACH = ("csr", "ss", "coo", "css", "bin")
PADDED_REACH = ("ell", "jds", "hyb")
TINY_ULP = np.longdouble(2.0) ** -1074  # the spacing of the f64 subnormals


# ---------------------------------------------------------------- small tools
def bits(a):
    """The int64 patterns of a float64 array (NaN payloads and the sign of zero count)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def classify(y):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf per element."""
    y = np.asarray(y, np.float64)
    return np.where(np.isnan(y), 1, np.where(y == np.inf, 2, np.where(y == -np.inf, 3, 0))).astype(np.int8)


def rows_touching(rrp, rcol, colmask):
    """Per row of the column lists (rrp, rcol): does any column have colmask set?"""
    hit = np.asarray(colmask, bool)[rcol].astype(np.int64)
    return np.diff(np.concatenate([[0], np.cumsum(hit)])[rrp]) > 0


def _unique_pairs(row, c, m, n):
    """(rrp, rcol) of the distinct (row, column) pairs, columns ascending per row."""
    key = np.unique(np.asarray(row, np.int64) * n + np.asarray(c, np.int64))
    r = key // n
    rrp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64)
    return rrp, (key - r * n).astype(np.int64)


# ---------------------------------------------------------------- reach
def reach(info, rp, col, m, n):
    """(rrp, rcol): per row, the columns whose x the resolved layout of
    `info` (Plan.info()) may multiply -- the table in the module docstring."""
    fmt = info["format"]
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int64)
    lens = np.diff(rp)
    row = np.repeat(np.arange(m, dtype=np.int64), lens)
    if fmt in EXACT_REACH:
        return _unique_pairs(row, col, m, n)
    if fmt in PADDED_REACH:
        empty = np.flatnonzero(lens == 0)
        return _unique_pairs(np.concatenate([row, empty]), np.concatenate([col, np.zeros(len(empty), np.int64)]), m, n)
    if fmt == "dia":
        off = np.unique(col - row)
        r = np.repeat(np.arange(m, dtype=np.int64), len(off))
        return _unique_pairs(r, np.clip(r + np.tile(off, m), 0, n - 1), m, n)
    raise KeyError(fmt)


def cols_of(rp, col, m, n):
    """(rrp, rcol) of the rows' own distinct columns."""
    return reach({"format": "csr"}, rp, col, m, n)


# ---------------------------------------------------------------- poisoned x
def poison_cols(n, seed):
    """Columns 0 and n - 1 (the pad column of SS tiles and of the ELL family's
    empty rows; DIA's clamp targets) plus max(1, n // 400) seeded distinct
    columns of [1, n - 2], sorted."""
    rng = np.random.default_rng(seed)
    inner = 1 + rng.choice(n - 2, max(1, n // 400), replace=False)
    return np.sort(np.concatenate([[0, n - 1], inner])).astype(np.int64)


def poison_values(k):
    """NaN, +Inf, -Inf cycling over k (sorted) columns."""
    return np.array([POISON[i % 3] for i in range(k)])


def _freeze(d):
    for a in d.values():
        for b in (a if isinstance(a, tuple) else (a,)):
            if isinstance(b, np.ndarray):
                b.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """signed_inputs.case(name, "cancel") with x poisoned at poison_cols and
    val = +0.0 on every entry that references every second poisoned column
    (P[::2]): those rows are non-finite only through 0 * NaN / 0 * Inf, so a
    stored zero must be multiplied (no pad fix may key on val == 0).

    x_clean with the same val is the clean run (ref, y_clean: its
    extended-precision reference and sequential sum); y_oracle the sequential
    sum on the poisoned x; hit = rows whose columns meet P."""
    import oracle
    base = si.case(name, "cancel")
    m, n, rp, col = base["m"], base["n"], base["rp"], base["col"]
    P = poison_cols(n, seed=1000 + si.STRUCTURES.index(name))
    zeroed = np.zeros(n, bool)
    zeroed[P[::2]] = True
    val = np.where(zeroed[col], 0.0, base["val"])
    x = base["x"].copy()
    x[P] = poison_values(len(P))
    poisoned = ~np.isfinite(x)
    crp, ccol = cols_of(rp, col, m, n)
    c = dict(base)
    c.update(val=val, x=x, x_clean=base["x"], P=P, poisoned=poisoned, hit=rows_touching(crp, ccol, poisoned),
             ref=si.ref_rows(rp, col, val, base["x"]), y_clean=oracle.csr_spmv(rp, col, val, base["x"]),
             y_oracle=oracle.csr_spmv(rp, col, val, x))
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def inverse_case(name):
    """The forward case's (zeroed) val with x finite only on the columns that
    K references and NaN everywhere else; K = the non-empty rows with
    r % 211 == 3 and at most 129 entries.  clean = the non-empty rows whose
    columns are all finite (K and whichever rows share its columns); hit =
    every other non-empty row."""
    import oracle
    f = forward_case(name)
    m, n, rp, col = f["m"], f["n"], f["rp"], f["col"]
    lens = np.diff(rp)
    K = np.flatnonzero((np.arange(m) % 211 == 3) & (lens > 0) & (lens <= 129))
    finite = np.zeros(n, bool)
    for r in K:
        finite[col[rp[r]:rp[r + 1]]] = True
    x = np.where(finite, f["x_clean"], np.nan)
    crp, ccol = cols_of(rp, col, m, n)
    hit = rows_touching(crp, ccol, ~finite)
    c = dict(f)
    c.update(x=x, K=K, poisoned=~finite, hit=hit, clean=(lens > 0) & ~hit, y_oracle=oracle.csr_spmv(rp, col, f["val"], x))
    del c["P"]
    return _freeze(c)


def poison_failing_rows(y, y_clean, hit, reached, y_class=None, loose=None, rp=None, ref=None):
    """Rows of y (computed on a poisoned x) that break the contract:

      hit      (the row's own columns meet a poisoned column): y non-finite,
               and of class y_class (classify() of the sequential sum) where
               y_class is given -- the exact-reach layouts;
      ~reached (the layout's reach misses every poisoned column): bit for bit
               y_clean, that plan's y on the clean x.  Rows in `loose` (COO
               rows split across units: unordered atomics) must instead be
               within signed_inputs.row_tol of ref.

    Rows reached but not hit (pads of the padded layouts) are not judged."""
    y = np.asarray(y, np.float64)
    hit = np.asarray(hit, bool)
    reached = np.asarray(reached, bool) | hit
    loose = np.zeros(len(y), bool) if loose is None else np.asarray(loose, bool)
    bad = hit & np.isfinite(y)
    if y_class is not None:
        bad |= hit & (classify(y) != y_class)
    bad |= ~reached & ~loose & (bits(y) != bits(y_clean))
    if loose.any():
        out = np.zeros(len(y), bool)
        out[si.failing_rows(y, rp, ref)[0]] = True
        bad |= ~reached & loose & out
    return np.flatnonzero(bad)


def assert_poisoned(y, y_clean, hit, reached, what, y_class=None, loose=None, rp=None, ref=None):
    """poison_failing_rows must be empty; reports the first failing row and
    which clause it breaks.  Returns the number of rows reached, not hit and
    non-finite (a measurement: pads that multiplied a poisoned x)."""
    bad = poison_failing_rows(y, y_clean, hit, reached, y_class, loose, rp, ref)
    if len(bad):
        w = int(bad[0])
        if hit[w]:
            why = "references a poisoned column, must be non-finite" + (
                "" if y_class is None else f" of class {int(y_class[w])} (1 NaN, 2 +Inf, 3 -Inf)")
        else:
            why = f"is out of the poison's reach, must equal the clean run's {y_clean[w]!r}"
        raise AssertionError(f"{what}: {len(bad)} rows break the poisoned-x contract, first {bad[:5].tolist()}; "
                             f"row {w} {why}, got {y[w]!r}")
    return int((np.asarray(reached, bool) & ~np.asarray(hit, bool) & ~np.isfinite(y)).sum())


# ---------------------------------------------------------------- tiny / huge
def _scaled(rp, n, seed, val_exp, x_exp):
    rng = np.random.default_rng(seed)
    nnz = int(rp[-1])
    val = rng.choice([-1.0, 1.0], nnz) * rng.uniform(0.5, 1.0, nnz) * 2.0 ** val_exp
    x = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 1.0, n) * 2.0 ** x_exp
    return val, x


def tiny(rp, col, n, seed):
    """val = +-U(0.5,1) 2^-530, x = +-U(0.5,1) 2^-535: every product lies in
    [2^-1067, 2^-1065], subnormal; 9000 of them sum below 2^-1051."""
    return _scaled(rp, n, seed, -530, -535)


def huge(rp, col, n, seed):
    """val, x = +-U(0.5,1) 2^500: products up to 2^1000, 9000 of them sum
    below 2^1014, finite."""
    return _scaled(rp, n, seed, 500, 500)


EXTREME = {"tiny": tiny, "huge": huge}


@functools.lru_cache(maxsize=None)
def extreme_case(name, family):
    """As signed_inputs.case for the `tiny` / `huge` families."""
    import oracle
    m, n, rp, col = si.structure(name)
    val, x = EXTREME[family](rp, col, n, seed=2000 + si.STRUCTURES.index(name) * 2 + sorted(EXTREME).index(family))
    row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    return _freeze({"name": name, "family": family, "m": m, "n": n, "rp": rp, "row": row, "col": col, "val": val, "x": x,
                    "ref": si.ref_rows(rp, col, val, x), "y_oracle": oracle.csr_spmv(rp, col, val, x)})


def tiny_tol(rp):
    """(len + 8) * 2^-1074 per row (derived in the module docstring)."""
    return (np.diff(np.asarray(rp, np.int64)) + 8).astype(np.longdouble) * TINY_ULP


def tiny_failing_rows(y, rp, ref):
    """(rows with |y - y_hi| > tiny_tol or a non-finite y, err / tol per row)."""
    tol = tiny_tol(rp)
    err = np.abs(np.asarray(y, np.float64).astype(np.longdouble) - ref[0])
    ratio = (err / tol).astype(np.float64)
    ratio[np.isnan(ratio)] = np.inf
    return np.flatnonzero(~(err <= tol)), ratio


def extreme_failing_rows(family, y, rp, ref):
    return tiny_failing_rows(y, rp, ref) if family == "tiny" else si.failing_rows(y, rp, ref)


def assert_extreme(family, y, rp, ref, what):
    """Every row within tiny_tol (`tiny`) or signed_inputs.row_tol (`huge`);
    reports the worst row.  Returns the largest err / tol (a measurement)."""
    bad, ratio = extreme_failing_rows(family, y, rp, ref)
    if len(bad):
        w = int(bad[np.argmax(ratio[bad])])
        lens = np.diff(np.asarray(rp, np.int64))
        raise AssertionError(f"{what}: {len(bad)} rows beyond the {family} bound, first {bad[:5].tolist()}; worst row {w} "
                             f"(len {int(lens[w])}): y {y[w]!r} vs {float(ref[0][w])!r}, err/tol {ratio[w]:.3g}")
    return float(ratio.max()) if len(ratio) else 0.0
