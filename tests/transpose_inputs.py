"""Inputs of the transposition tests (tests/test_transpose_host.py on the CPU,
tests/test_gpu_transpose.py on the GPU): a numpy reference, the edge list, the
inputs that must be refused, and `twin` -- the transpose of a signed_inputs
case, so that A^T is that very case and all its references apply as they stand.

Plain helper module (numpy only, besides signed_inputs).
"""
import functools

import numpy as np

import signed_inputs as si

NAN_PAYLOAD = np.array([0x7FF8000000ABCDEF], np.uint64).view(np.float64)[0]
SPECIALS = np.array([NAN_PAYLOAD, -0.0, np.inf, 3 * 5e-324])  # a NaN with a payload, -0.0, +Inf, a subnormal


def np_transpose(m, n, rp, col, val=None):
    """(t_rp, t_col, t_val, perm) of the CSR of A^T: the entries stably sorted
    by column (output row c = A's entries of column c in source order),
    t_col = the source rows, values moved, perm = source entry of each output
    entry.  val = None: t_val is None."""
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col, np.int32)
    perm = np.argsort(col, kind="stable").astype(np.int64)
    row = np.repeat(np.arange(m, dtype=np.int32), np.diff(rp))
    t_rp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n)[:n])]).astype(np.int64)
    t_val = None if val is None else np.ascontiguousarray(np.asarray(val, np.float64)[perm])
    return t_rp, np.ascontiguousarray(row[perm]), t_val, perm


def bits(a):
    """float64 array as uint64 (NaN payloads and signed zeros compare)."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_same_csr(got, want, what):
    """(t_rp, t_col, t_val[, perm]) equal array by array, values as bits."""
    for k, name in enumerate(("t_row_ptr", "t_col", "t_val", "perm")[:len(want)]):
        g, w = got[k], want[k]
        if w is None or g is None:
            assert g is None and w is None, f"{what}: {name} present on one side only"
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        same = np.array_equal(bits(g), bits(w)) if name == "t_val" else np.array_equal(g, w)
        assert same, f"{what}: {name} differs"


def _values(nnz, seed):
    val = np.random.default_rng(seed).standard_normal(nnz)
    k = min(nnz, len(SPECIALS))
    val[:k] = SPECIALS[:k]
    return val


def _rows_with(m, n, cols_per_row, seed):
    """m rows, each holding the columns `cols_per_row`, shuffled inside the row."""
    rng = np.random.default_rng(seed)
    col = np.concatenate([rng.permutation(cols_per_row) for _ in range(m)]).astype(np.int32)
    rp = (np.arange(m + 1) * len(cols_per_row)).astype(np.int64)
    return m, n, rp, col


def _random(m, n, nnz, seed):
    """Unsorted rows with duplicates."""
    rng = np.random.default_rng(seed)
    row = np.sort(rng.integers(0, m, nnz))
    rp = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=m))]).astype(np.int64)
    return m, n, rp, rng.integers(0, n, nnz).astype(np.int32)


def _column7():
    # rect513x40 with an entry of column 7 appended to every row (out of order, a duplicate where the row had one)
    m, n, rp, col = si.structure("rect513x40")
    lens = np.diff(rp) + 1
    rp2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col2 = np.empty(int(rp2[-1]), np.int32)
    last = rp2[1:] - 1
    col2[last] = 7
    keep = np.ones(len(col2), bool)
    keep[last] = False
    col2[keep] = col
    return m, n, rp2, col2


SPARSE_COLS = np.array([0, 1, 63, 64, 65, 255, 256, 257, 65535, 65536, 69999])
SHIFTED_COLS = np.array([1, 2, 64, 65, 66, 256, 257, 258, 65536, 65537, 69998])  # column 0 and column n - 1 empty


@functools.lru_cache(maxsize=None)
def edges():
    """{name: (m, n, rp, col, val)}: the smallest shapes at which the pipeline
    can go wrong (arrays shared: do not write)."""
    z64, z32 = np.zeros(1, np.int64), np.zeros(0, np.int32)
    shapes = {
        "m0-n5": (0, 5, z64, z32),
        "n0-m5": (5, 0, np.zeros(6, np.int64), z32),
        "empty-7x9": (7, 9, np.zeros(8, np.int64), z32),
        "1x1": (1, 1, np.array([0, 1], np.int64), np.zeros(1, np.int32)),
        "300x1": (300, 1, np.arange(301, dtype=np.int64), np.zeros(300, np.int32)),  # zero key bits, one output row
        "1x300-dense": (1, 300, np.array([0, 300], np.int64), np.arange(300, dtype=np.int32)),
        "5x70000-sparse-cols": _rows_with(5, 70000, SPARSE_COLS, 70000),
        "5x70000-empty-ends": _rows_with(5, 70000, SHIFTED_COLS, 70001),
        "513x40-column7": _column7(),
    }
    for nnz in (1, 255, 256, 257, 65537):
        shapes[f"random1000-nnz{nnz}"] = _random(1000, 1000, nnz, nnz)
    out = {}
    for k, (name, (m, n, rp, col)) in enumerate(shapes.items()):
        val = _values(len(col), 900 + k)
        for a in (rp, col, val):
            a.setflags(write=False)
        out[name] = (m, n, rp, col, val)
    return out


def refused():
    """{name: (m, n, nnz, rp or None, col)}: inputs both transpositions refuse
    with SPMV_ERROR_INVALID_VALUE, outputs untouched."""
    rp = np.array([0, 2, 3, 5], np.int64)
    col = np.array([0, 3, 1, 2, 3], np.int32)
    hi, neg = col.copy(), col.copy()
    hi[3] = 4    # = n
    neg[1] = -1
    return {
        "col-eq-n": (3, 4, 5, rp, hi),
        "col-negative": (3, 4, 5, rp, neg),
        "row_ptr-decreasing": (3, 4, 5, np.array([0, 3, 2, 5], np.int64), col),
        "row_ptr-null": (3, 4, 5, None, col),
    }


@functools.lru_cache(maxsize=None)
def twin(name, family):
    """A := the transpose of signed_inputs.case(name, family), pattern and
    values: {"m", "n", "rp", "col", "val"} of A (n_case x m_case), "case" the
    case itself.  Every structure's rows ascend in column order, so A^T is the
    case byte for byte -- asserted here."""
    c = si.case(name, family)
    t_rp, t_col, t_val, _ = np_transpose(c["m"], c["n"], c["rp"], c["col"], c["val"])
    back = np_transpose(c["n"], c["m"], t_rp, t_col, t_val)
    assert_same_csr(back[:3], (c["rp"], c["col"], np.ascontiguousarray(c["val"])), f"twin({name}, {family}) round trip")
    for a in (t_rp, t_col, t_val):
        a.setflags(write=False)
    return {"m": c["n"], "n": c["m"], "rp": t_rp, "col": t_col, "val": t_val, "case": c}
