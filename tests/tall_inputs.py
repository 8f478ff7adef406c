"""Tiny matrices spread over very many rows: the inputs that put every format's
row side -- y[r], the row pointers, perm, rmap, nzrow, empty_rows, the row
lists of adaptive CSR and of the HYB / JDS overflow -- beyond 4 GiB.

What crosses where (TALL = 2^29 rows):

    m = 2^29      the byte offset of y[r], of 64-bit row pointers and of
                  per-row 8-byte arrays passes 2^32
    m = 2^30      the byte offset into 4-byte per-row arrays passes 2^32;
                  2 * r leaves int32
    m = 2^31 - 2  the API's largest m: m + 63, m + 1, (m + 1) / 2 + 255 leave
                  int32
    m = 2^26      Y[r * ldy + j] passes 2^32 bytes at ldy = 8 (MULTI_TALL)

A wrong offset does not fault: it wraps and stores a finite, plausible value
2^29 rows away (wide_inputs.py says the same of x).  Only y and the per-row
arrays have to be big to get there, so the matrices here have 4003 live rows
and at most about 150 k entries.

Compact, then spread.  A case is generated on its M = 4003 compact rows over
n = 8192 columns (tall_band: n = m, the columns compacted as wide_inputs does),
with val and x from signed_inputs' `cancel` family; the sequential reference is
oracle.csr_spmv on the compact arrays, the per-row bound signed_inputs.ref_rows
/ row_tol / assert_rows, unchanged.  Compact row i is row rowmap[i] of the tall
matrix; every other row is empty.  No m-sized array is ever made on the host:
the tall row pointers are a cumsum on the device, and check_y looks at y there
-- the live rows gathered and judged as every other test judges a y, then
zeroed in place, after which all of y must be +0.0 bit for bit.  A store at a
wrapped offset therefore fails twice: a stray non-zero on an empty row, and a
live row still holding its fill.

y = alpha A x + beta y (check_axpby_y) starts from a y0 that is a formula of
the row, y0_rows: never zero, another value 2^29, 2^30 and 2^31 rows away, and
cheap to evaluate on the device a chunk at a time, so every row off the live
ones is checked bit for bit against beta * y0[r] without an m-sized copy.

Plain helper module (numpy only, besides signed_inputs, special_values,
wide_inputs, axpby_inputs and the oracle; torch only inside the device
builders and the two checks);
tests/test_tall_inputs.py checks it on the CPU, tests/test_gpu_tall_y.py uses
it on the GPU.
"""
import functools

import numpy as np

import axpby_inputs as ai
import signed_inputs as si
import special_values as sv
import wide_inputs as wi

TALL = 1 << 29  # y reaches 4 GiB
MS = (TALL - 1,         # the control: the last size with every row-side offset in 32 bits
      TALL + 4099,      # y offsets truly beyond 2^32; m is odd
      2 * TALL + 4099,  # rows beyond 2^30: the 4-byte per-row arrays beyond 4 GiB
      4 * TALL - 2)     # the API's largest m
MULTI_TALL = TALL // 8  # Y[r * ldy] reaches 4 GiB at ldy = 8
MULTI_MS = (MULTI_TALL - 1, MULTI_TALL + 4099)
CPU_M = 1 << 20  # a full host y is cheap here (tests/test_tall_inputs.py)

M = wi.M  # live rows: odd, no multiple of 64, 256 or 512
N = 8192  # columns of tall_uniform and tall_long
STRUCTURES = ("tall_uniform", "tall_long")
BAND = "tall_band"  # DIA only: n = m
BAND_OFFSETS = (-1, 0, 1)
LONG_ROWS = si.STAIR_LONG  # compact row: entries
EMPTY_EVERY = 11  # compact row i is empty when i % 11 == 5 (and no row below asks to stay)
CUMSUM_CHUNK = 1 << 27  # device_csr's cumsum and check_y's count walk the big tensors in pieces of this size
X_FILL = 1.0  # tall_band: x off the live columns (DIA multiplies its zero slots by it)
AXPBY = (-2.5, 0.75)  # (alpha, beta) of the one execute_axpby every tall case adds
# y0[r] = +-((r mod Y0_PERIOD) + 1) / 8192.  The period must not divide 2^29, 2^30 or 2^31 (8191 is prime: they leave
# 8, 16 and 32), so a y0 loaded that many rows away is another value -- never make it a power of two.  It stays below
# 8192 so that y0 has at most 13 significant bits and 0.75 * y0 is exact.
Y0_PERIOD = 8191


# ---------------------------------------------------------------- the row map
def clusters(m):
    """[lo, hi) row ranges, wide_inputs.clusters on the rows: 2048 rows at 0,
    around 2^28, 2^29 and 2^30 (those that fit below the last one), and the
    end [m - 4096, m)."""
    return wi.clusters(m)


def promised_rows(m):
    """The rows every map holds, inside a cluster or not: 0, m - 1 and, where
    the matrix has them, the pairs (2^29 - 1, 2^29) and (2^30 - 1, 2^30)."""
    out = [0, m - 1]
    for p in (29, 30):
        if m > 1 << p:
            out += [(1 << p) - 1, 1 << p]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def rowmap(m):
    """M ascending distinct rows of [0, m): the promised rows, the others
    drawn from the clusters (int64, read-only)."""
    pool = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in clusters(m)])
    must = np.array(promised_rows(m), np.int64)
    rest = np.setdiff1d(pool, must)
    rng = np.random.default_rng(m % 1000003 + 29)
    rows = np.sort(np.concatenate([must, rng.choice(rest, M - len(must), replace=False)]))
    assert len(rows) == M and (np.diff(rows) > 0).all() and rows[0] == 0 and rows[-1] == m - 1
    rows.setflags(write=False)
    return rows


# ---------------------------------------------------------------- structures
def _from_rows(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate(rows).astype(np.int64)


def _empty_rows(m, keep=()):
    """Compact rows left empty: one in eleven, never a promised row's, never
    one of `keep`."""
    e = np.arange(M) % EMPTY_EVERY == 5
    e[np.searchsorted(rowmap(m), promised_rows(m))] = False
    e[list(keep)] = False
    return e


def _tall_uniform(m, rng):
    """16 distinct ascending columns per row."""
    empty = _empty_rows(m)
    none = np.zeros(0, np.int64)
    return _from_rows([none if empty[r] else np.sort(rng.choice(N, 16, replace=False)) for r in range(M)])


def _tall_long(m, rng):
    """Power-law row lengths 1..700 plus the three rows of
    signed_inputs.STAIR_LONG (4096, 4097 and 9000 entries, columns with
    duplicates), ascending: the HYB / JDS overflow, the CSS split, adaptive
    CSR's row lists, BIN's long rows at bin_long_len = 40."""
    empty = _empty_rows(m, keep=[7, 8, 9] + sorted(LONG_ROWS))
    lens = np.minimum(700, 1 + np.floor(3.0 * rng.pareto(1.0, M))).astype(np.int64)
    lens[7], lens[8], lens[9] = 700, 129, 128
    rows = []
    for r in range(M):
        if empty[r]:
            rows.append(np.zeros(0, np.int64))
        elif r in LONG_ROWS:
            rows.append(np.sort(rng.integers(0, N, LONG_ROWS[r])))
        else:
            rows.append(np.sort(rng.choice(N, int(lens[r]), replace=False)))
    return _from_rows(rows)


def _tall_band(m, rng):
    """Diagonals -1, 0, +1 of an m x m matrix on the live rows: col = row + o,
    clamped out at the two ends (row 0 has no -1, row m - 1 no +1)."""
    empty = _empty_rows(m)
    rows = []
    for i, r in enumerate(rowmap(m).tolist()):
        c = np.array([r + o for o in BAND_OFFSETS if 0 <= r + o < m], np.int64)
        rows.append(c[:0] if empty[i] else c)
    return _from_rows(rows)


_NAMES = STRUCTURES + (BAND,)
_BUILD = {"tall_uniform": _tall_uniform, "tall_long": _tall_long, "tall_band": _tall_band}


@functools.lru_cache(maxsize=None)
def case(name, m):
    """One structure spread over m rows, with the `cancel` family's values on
    its compact arrays: rowmap, rp (compact, M + 1), col (int32, the columns
    the plan is built from), ucol / ccol (tall_band: the live columns and col
    on them; else ucol = arange(N), ccol = col), val, x_c, ref
    (signed_inputs.ref_rows on the compact arrays) and y_oracle (the oracle's
    sequential sums) -- computed once, read-only."""
    import oracle
    k = _NAMES.index(name)
    rp, col = _BUILD[name](m, np.random.default_rng(m % 1000003 + 1000 * k))
    n = m if name == BAND else N
    ucol = np.unique(col) if name == BAND else np.arange(N, dtype=np.int64)
    ccol = np.searchsorted(ucol, col).astype(np.int32)
    assert int(rp[-1]) <= 160_000 and col.min() >= 0 and col.max() < n
    val, x_c = si.FAMILIES["cancel"](rp, ccol, len(ucol), seed=k * 7 + m % 1000003)
    val, x_c = np.ascontiguousarray(val), np.ascontiguousarray(x_c)
    c = {"name": name, "m": m, "n": n, "rowmap": rowmap(m), "rp": rp, "col": col.astype(np.int32), "col64": col,
         "ucol": ucol, "ccol": ccol, "val": val, "x_c": x_c, "ref": si.ref_rows(rp, ccol, val, x_c),
         "y_oracle": oracle.csr_spmv(rp, ccol, val, x_c)}
    return sv._freeze(c)


@functools.lru_cache(maxsize=None)
def column(name, m, j):
    """Column j of the case's multi-vector X on the compact columns, with its
    references (as wide_inputs.column): column 0 is the case's own x_c."""
    import oracle
    c = case(name, m)
    if j == 0:
        return {"x_c": c["x_c"], "ref": c["ref"], "y_oracle": c["y_oracle"]}
    rng = np.random.default_rng(j)
    k = len(c["ucol"])
    x = rng.choice([-1.0, 1.0], k) * rng.uniform(0.5, 2.0, k)
    return sv._freeze({"x_c": x, "ref": si.ref_rows(c["rp"], c["ccol"], c["val"], x),
                       "y_oracle": oracle.csr_spmv(c["rp"], c["ccol"], c["val"], x)})


# ---------------------------------------------------------------- device builders
def device_csr(c, m, device, out=None):
    """(row_ptr, col, val) of the tall CSR on `device`: row_ptr is the int64
    cumsum of the row lengths scattered through rowmap, made on the device
    (`out`: an m + 1 entry int64 tensor to fill instead of a new one); col
    and val are the compact ones."""
    import torch
    assert c["m"] == m
    rp = torch.empty(m + 1, dtype=torch.int64, device=device) if out is None else out
    assert rp.numel() == m + 1 and rp.dtype == torch.int64
    rp.zero_()
    rp[torch.from_numpy(c["rowmap"] + 1).to(device)] = torch.from_numpy(np.diff(c["rp"])).to(device)
    carry = None
    for a in range(0, m + 1, CUMSUM_CHUNK):  # in place, 2^27 entries at a time, the running total carried on the device
        part = rp[a:a + CUMSUM_CHUNK]
        part.cumsum_(0)
        if carry is not None:
            part += carry
        carry = part[-1].clone()
    return rp, torch.from_numpy(np.array(c["col"])).to(device), torch.from_numpy(np.array(c["val"])).to(device)


def device_x(c, device, x_c=None):
    """The device x.  tall_uniform / tall_long: the N compact values, every
    one of them live.  tall_band: m doubles filled as wide_inputs.device_x
    fills them, x[ucol] = x_c -- but DIA's reach (special_values.reach: its
    zero-filled slots multiply x[r + o] on every row) is every column, so the
    fill off the live columns is the finite X_FILL, not NaN."""
    import torch
    x_c = c["x_c"] if x_c is None else x_c
    if c["name"] != BAND:
        return torch.from_numpy(np.array(x_c)).to(device)
    x = torch.full((c["n"],), X_FILL, dtype=torch.float64, device=device)
    x[torch.from_numpy(np.array(c["ucol"])).to(device)] = torch.from_numpy(np.array(x_c)).to(device)
    return x


def device_X(c, ldx, k, device):
    """The multi-vector block (n x ldx; columns [k, ldx) NaN, never read) of
    the k columns of `column`."""
    import torch
    cols = np.stack([column(c["name"], c["m"], j)["x_c"] for j in range(k)], axis=1)
    X = torch.full((c["n"], ldx), float("nan"), dtype=torch.float64, device=device)
    if c["name"] == BAND:
        X[:, :k] = X_FILL
    X[torch.from_numpy(np.array(c["ucol"])).to(device), :k] = torch.from_numpy(cols).to(device)
    return X


# ---------------------------------------------------------------- the check
def live(y_dev, c):
    """y on the live rows, on the host."""
    import torch
    idx = torch.from_numpy(np.array(c["rowmap"])).to(y_dev.device)
    return y_dev[idx].cpu().numpy()


def nonzero_bits(y_dev):
    """How many entries of y_dev are not +0.0 bit for bit, counted 2^27
    entries at a time (the count's temporaries stay below the chunk's size)."""
    import torch
    bits = y_dev.view(torch.int64)
    return sum(int(torch.count_nonzero(bits[a:a + CUMSUM_CHUNK])) for a in range(0, bits.numel(), CUMSUM_CHUNK))


def _bin_rows(info, y, c, x_c, y_oracle, what):
    """test_gpu_parity.assert_bin_rows on the compact arrays, from the
    plan's info: rows below the long-row threshold bit for bit, long rows
    within 1e-12 of sum |a x|."""
    ll = info["bin_long_len"]
    if ll == 0:
        assert np.array_equal(y, y_oracle), f"bin {what}: not bit-exact"
        return
    long_rows = np.diff(c["rp"]) >= ll
    assert np.array_equal(y[~long_rows], y_oracle[~long_rows]), f"bin {what}: short rows not bit-exact"
    import oracle
    mag = oracle.csr_spmv(c["rp"], c["ccol"], np.abs(c["val"]), np.abs(x_c))
    err = np.abs(y[long_rows] - y_oracle[long_rows])
    assert np.all(err <= 1e-12 * mag[long_rows] + 1e-300), f"bin {what}: long rows off by {err.max()}"


def check_y(y_dev, c, what, info=None, col=None, prev=None):
    """What every tall test asks of a y (an m-entry tensor, or the strided
    view Y[:, j] of a block), on the device it lives on.

    The live rows, gathered: finite and within signed_inputs.row_tol of the
    compact reference; +0.0 where the compact row is empty; with the plan's
    `info`, bit for bit the oracle's sequential sum where
    signed_inputs.plan_is_sequential, and BIN as assert_bin_rows; with `prev`
    (the live rows of an earlier execute of the same plan over another fill)
    bit for bit those -- COO: only the rows inside one 128-entry unit.  Then
    0 is stored at the live rows, in place, and no non-zero bit may be left
    anywhere in y: every other row is +0.0 exactly.  `col`: the references of
    another column (`column`).  Returns the largest err / row_tol."""
    import torch
    x_c = c["x_c"] if col is None else col["x_c"]
    ref = c["ref"] if col is None else col["ref"]
    y_oracle = c["y_oracle"] if col is None else col["y_oracle"]
    rp = c["rp"]
    lens = np.diff(rp)
    assert y_dev.dim() == 1 and y_dev.numel() == c["m"] and y_dev.dtype == torch.float64
    idx = torch.from_numpy(np.array(c["rowmap"])).to(y_dev.device)
    y = y_dev[idx].cpu().numpy()
    assert np.isfinite(y).all(), (f"{what}: {int((~np.isfinite(y)).sum())} live rows are not finite, first compact "
                                  f"rows {np.flatnonzero(~np.isfinite(y))[:5].tolist()} "
                                  f"(rows {c['rowmap'][~np.isfinite(y)][:5].tolist()})")
    worst = si.assert_rows(y, rp, c["ccol"], c["val"], x_c, what, ref=ref)
    assert (sv.bits(y[lens == 0]) == 0).all(), f"{what}: an empty live row is not +0.0"
    if info is not None:
        if info["format"] == "bin":
            _bin_rows(info, y, c, x_c, y_oracle, what)
        if si.plan_is_sequential(info):
            assert np.array_equal(y, y_oracle), f"{what}: {info['format']} is sequential, must be bit-exact"
    if prev is not None:
        if info is not None and info["format"] == "coo":
            # f64 atomics: a row split across 128-entry units may round differently
            # run to run; a row inside one unit gets exactly one atomic
            inside = (rp[:-1] // 128 == (rp[1:] - 1) // 128) & (lens > 0)
            assert np.array_equal(y[inside], prev[inside]), f"{what}: rows inside one unit differ run to run"
        else:
            assert np.array_equal(sv.bits(y), sv.bits(prev)), f"{what}: y depends on what y held before"
    y_dev[idx] = 0.0
    stray = nonzero_bits(y_dev)
    if stray:
        at = torch.nonzero(y_dev.view(torch.int64))[:5, 0].cpu().tolist() if stray <= 1 << 20 else []
        raise AssertionError(f"{what}: {stray} rows off the live ones are not +0.0, first {at}: "
                             f"{[float(y_dev[r]) for r in at]}")
    return worst


# ---------------------------------------------------------------- y = alpha A x + beta y
def y0_rows(rows):
    """y0 on the given rows (numpy): (+1 if r is even else -1) * ((r mod 8191) + 1) / 8192."""
    r = np.asarray(rows, np.int64)
    return np.where(r % 2 == 0, 1.0, -1.0) * ((r % Y0_PERIOD + 1).astype(np.float64) / 8192.0)


def _y0_chunk(a, b, device, scale=1.0):
    """scale * y0 on rows [a, b), on `device`.  Evaluated in float64: the rows (< 2^31), fmod and the division by
    8192 are exact, and so is scale = 0.75 on the 13 bits of y0."""
    import torch
    sign = torch.arange(a, b, dtype=torch.float64, device=device).fmod_(2.0).mul_(-2.0).add_(1.0)
    v = torch.arange(a, b, dtype=torch.float64, device=device).fmod_(float(Y0_PERIOD)).add_(1.0).mul_(1.0 / 8192.0)
    v.mul_(sign)
    return v if scale == 1.0 else v.mul_(scale)


def fill_y0(y_dev, shift=0):
    """y_dev[r] = y0[r + shift], CUMSUM_CHUNK rows at a time (`shift`: the CPU tests' planted error)."""
    for a in range(0, y_dev.numel(), CUMSUM_CHUNK):
        b = min(a + CUMSUM_CHUNK, y_dev.numel())
        y_dev[a:b] = _y0_chunk(a + shift, b + shift, y_dev.device)


def off_pattern(y_dev, beta):
    """(how many entries of y_dev are not beta * y0[r] bit for bit, the first five of them), counted
    CUMSUM_CHUNK rows at a time against the pattern recomputed for the chunk (a chunk with more than 2^20 of
    them is counted, not listed)."""
    import torch
    bits = y_dev.view(torch.int64)
    count, at = 0, []
    for a in range(0, bits.numel(), CUMSUM_CHUNK):
        b = min(a + CUMSUM_CHUNK, bits.numel())
        diff = bits[a:b] != _y0_chunk(a, b, y_dev.device, beta).view(torch.int64)
        k = int(torch.count_nonzero(diff))
        if 0 < k <= 1 << 20 and len(at) < 5:
            at += (torch.nonzero(diff)[:5 - len(at), 0] + a).cpu().tolist()
        count += k
    return count, at


def check_axpby_y(y_dev, c, first_live, alpha, beta, what, info):
    """What every tall test asks of y after execute_axpby(x, y, alpha, beta) on a y that fill_y0 filled (an
    m-entry tensor, on the device it lives on).  beta * y0 must be exact and non-zero (AXPBY's 0.75 is).

    The live rows, gathered: finite; unless the plan is COO, bit for bit axpby_inputs.expected(first_live, y0,
    alpha, beta), first_live = the live rows of a plain execute of the same plan -- the header's two rounded
    multiplies and one rounded add on the plan's own row sums; where signed_inputs.plan_is_sequential, bit for bit
    expected(y_oracle, ...) too; every plan within axpby_inputs.assert_bound of the extended-precision reference;
    COO: the rows inside one 128-entry unit bit for bit, as check_y treats them.  Then beta * y0[row] is stored at
    the live rows, in place, and every entry of y must be bit for bit beta * y0[r], which is what
    alpha * (+0.0) + beta * y0[r] gives on a row without entries.  Returns the largest err / bound."""
    import torch
    rp = c["rp"]
    lens = np.diff(rp)
    assert y_dev.dim() == 1 and y_dev.numel() == c["m"] and y_dev.dtype == torch.float64
    idx = torch.from_numpy(np.array(c["rowmap"])).to(y_dev.device)
    y = y_dev[idx].cpu().numpy()
    bad = ~np.isfinite(y)
    assert not bad.any(), (f"{what}: axpby: {int(bad.sum())} live rows are not finite, first compact rows "
                           f"{np.flatnonzero(bad)[:5].tolist()} (rows {c['rowmap'][bad][:5].tolist()})")
    y0 = y0_rows(c["rowmap"])
    off = np.multiply(np.float64(beta), y0)
    assert np.array_equal(ai.expected(np.zeros(len(y0)), y0, alpha, beta), off) and (off != 0).all()

    def same(want, rows, why):
        d = np.flatnonzero((ai.bits(y) != ai.bits(want)) & rows)
        assert not len(d), (f"{what}: axpby: {len(d)} live rows are not {why}, first compact rows {d[:5].tolist()} "
                            f"(rows {c['rowmap'][d[:5]].tolist()}): {y[d[:5]].tolist()} vs {want[d[:5]].tolist()}")

    want = ai.expected(first_live, y0, alpha, beta)
    if info["format"] == "coo":
        # f64 atomics: only a row inside one 128-entry unit (and a row without entries) gets its sum in one piece
        same(want, (rp[:-1] // 128 == (rp[1:] - 1) // 128) | (lens == 0), "expected(execute) inside one unit")
    else:
        same(want, np.ones(len(y), bool), "expected(execute): alpha * s + beta * y0 on the plan's own row sums")
    if si.plan_is_sequential(info):
        same(ai.expected(c["y_oracle"], y0, alpha, beta), np.ones(len(y), bool), "expected(sequential sum)")
    worst = ai.assert_bound(y, rp, c["ref"], y0, alpha, beta, what + ": axpby")
    y_dev[idx] = torch.from_numpy(off).to(y_dev.device)
    stray, at = off_pattern(y_dev, beta)
    if stray:
        raise AssertionError(f"{what}: axpby: {stray} rows off the live ones are not beta * y0, first {at}: "
                             f"{[float(y_dev[r]) for r in at]} vs {(beta * y0_rows(at)).tolist()}")
    return worst
