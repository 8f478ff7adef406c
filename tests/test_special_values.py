"""CPU checks of tests/special_values.py: the poisoned inputs, the reach
table, the tiny / huge families and bounds, and the checkers themselves on
numpy models of the kernel bugs they exist for -- what keeps
tests/test_gpu_special.py honest.
"""
import numpy as np
import pytest

import oracle
import signed_inputs as si
import special_values as sv

EXACT = {"format": "csr"}


def _nonempty(c):
    return np.diff(c["rp"]) > 0


# ---------------------------------------------------------------- inputs
@pytest.mark.parametrize("n", [40, 1000, 2048, 20077])
def test_poison_cols(n):
    P = sv.poison_cols(n, seed=n)
    assert P[0] == 0 and P[-1] == n - 1 and len(P) == 2 + max(1, n // 400)
    assert (np.diff(P) > 0).all()  # sorted, distinct, the seeded ones inside [1, n - 2]
    assert np.array_equal(P, sv.poison_cols(n, seed=n))
    v = sv.poison_values(len(P))
    assert np.isnan(v[0::3]).all() and (v[1::3] == np.inf).all() and (v[2::3] == -np.inf).all()


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_forward_case(name):
    """The conditions on the forward case and what the sequential sum makes
    of it: non-finite exactly on the hit rows, every class present, the other
    rows bit for bit the clean run."""
    c = sv.forward_case(name)
    base = si.case(name, "cancel")
    rp, col, P = c["rp"], c["col"], c["P"]
    ne = _nonempty(c)
    hit = c["hit"]
    print(f"forward {name}: {int(hit.sum())} hit rows ({hit.sum() / ne.sum():.3f} of non-empty), {len(P)} poisoned columns")
    assert hit.sum() >= 1 and hit.sum() <= 0.5 * ne.sum()
    assert not hit[~ne].any()
    # x differs from the clean x on P alone; val is +0.0 exactly on the entries of P[::2]
    assert np.array_equal(np.flatnonzero(sv.bits(c["x"]) != sv.bits(base["x"])), P)
    assert np.array_equal(c["x_clean"], base["x"]) and np.isfinite(c["x_clean"]).all()
    z = np.isin(col, P[::2])
    assert z.any() and (sv.bits(c["val"][z]) == 0).all() and np.array_equal(c["val"][~z], base["val"][~z])
    assert (base["val"] != 0).all()  # every zero of val is one of ours
    # some row is non-finite through 0 * NaN / 0 * Inf alone
    row = np.repeat(np.arange(c["m"]), np.diff(rp))
    only_zeroed = np.zeros(c["m"], bool)
    only_zeroed[row[z]] = True
    only_zeroed[row[np.isin(col, P[1::2])]] = False
    assert only_zeroed.any() and not np.isfinite(c["y_oracle"][only_zeroed]).any()
    # the oracle
    assert np.array_equal(~np.isfinite(c["y_oracle"]), hit)
    assert np.array_equal(sv.bits(c["y_oracle"][~hit]), sv.bits(c["y_clean"][~hit]))
    assert np.isfinite(c["y_clean"]).all()
    si.assert_rows(c["y_clean"], rp, col, c["val"], c["x_clean"], f"oracle, clean {name}", ref=c["ref"])
    if name != "rect7x1000":
        assert set(sv.classify(c["y_oracle"]).tolist()) == {0, 1, 2, 3}
    # a checker fed the oracle's own y passes, under the exact reach and under ELL's
    for info in (EXACT, {"format": "ell"}):
        reached = sv.rows_touching(*sv.reach(info, rp, col, c["m"], c["n"]), c["poisoned"])
        extra = sv.assert_poisoned(c["y_oracle"], c["y_clean"], hit, reached, name, y_class=sv.classify(c["y_oracle"]))
        assert extra == 0


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_inverse_case(name):
    c = sv.inverse_case(name)
    rp, col = c["rp"], c["col"]
    ne = _nonempty(c)
    lens = np.diff(rp)
    clean, hit, K = c["clean"], c["hit"], c["K"]
    print(f"inverse {name}: {int(clean.sum())} clean rows, {len(K)} K rows, {int(hit.sum())} of {int(ne.sum())} non-clean")
    assert clean.sum() >= 1 and hit.sum() >= 0.5 * ne.sum()
    assert len(K) >= 1 and clean[K].all() and (K % 211 == 3).all() and (lens[K] <= 129).all()
    assert np.array_equal(clean | hit, ne) and not (clean & hit).any()
    # x: finite (the clean x) exactly on K's columns, NaN elsewhere
    kc = np.unique(np.concatenate([col[rp[r]:rp[r + 1]] for r in K]))
    assert np.array_equal(np.flatnonzero(np.isfinite(c["x"])), kc) and np.isnan(c["x"][c["poisoned"]]).all()
    assert np.array_equal(c["x"][kc], c["x_clean"][kc])
    # the oracle: finite exactly on clean and empty rows, there the clean run bit for bit
    assert np.array_equal(np.isfinite(c["y_oracle"]), clean | ~ne)
    assert np.array_equal(sv.bits(c["y_oracle"][~hit]), sv.bits(c["y_clean"][~hit]))
    reached = sv.rows_touching(*sv.reach(EXACT, rp, col, c["m"], c["n"]), c["poisoned"])
    assert np.array_equal(reached, hit)
    assert sv.assert_poisoned(c["y_oracle"], c["y_clean"], hit, reached, name, y_class=sv.classify(c["y_oracle"])) == 0


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_tiny_case(name):
    """Every product subnormal, every sum subnormal; the sequential sum is
    within tiny_tol (by derivation; the figure is printed), and a y flushed to
    zero would fail on > 95 % of the non-empty rows."""
    c = sv.extreme_case(name, "tiny")
    rp, col = c["rp"], c["col"]
    tinyn = np.finfo(np.float64).tiny  # 2^-1022
    p = np.abs(c["val"] * c["x"][col])
    assert (p > 0).all() and (p < tinyn).all() and p.max() <= 2.0 ** -1065 and p.min() >= 2.0 ** -1067
    assert (c["ref"][1] < np.longdouble(tinyn)).all()  # sum |a x| (hence every partial sum) stays subnormal
    worst = sv.assert_extreme("tiny", c["y_oracle"], rp, c["ref"], f"oracle {name}/tiny")
    print(f"oracle err/tiny_tol {name}: {worst:.3f}")
    assert worst <= 1.0
    ne = _nonempty(c)
    big = np.abs(c["ref"][0]) > sv.tiny_tol(rp)
    assert big[ne].sum() > 0.95 * ne.sum(), f"{name}: only {int(big[ne].sum())} of {int(ne.sum())} rows exceed tiny_tol"
    assert (c["y_oracle"][~ne] == 0).all()


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_huge_case(name):
    c = sv.extreme_case(name, "huge")
    p = np.abs(c["val"] * c["x"][c["col"]])
    assert np.isfinite(p).all() and p.min() >= 2.0 ** 998 and p.max() < 2.0 ** 1000
    assert np.isfinite(c["ref"][1].astype(np.float64)).all() and np.isfinite(c["y_oracle"]).all()
    worst = sv.assert_extreme("huge", c["y_oracle"], c["rp"], c["ref"], f"oracle {name}/huge")
    print(f"oracle err/row_tol {name}/huge: {worst:.3f}")
    assert worst <= 1.0


# ---------------------------------------------------------------- reach
@pytest.mark.parametrize("name", si.STRUCTURES)
def test_reach_of_the_padded_layouts(name):
    """ELL / JDS / HYB: the rows' own columns, plus column 0 exactly for the
    empty rows; the exact layouts: the rows' own columns."""
    m, n, rp, col = si.structure(name)
    lens = np.diff(rp)
    crp, ccol = sv.cols_of(rp, col, m, n)
    for r in (0, m // 2, m - 1, int(np.argmax(lens))):  # duplicates collapse, columns ascend
        assert np.array_equal(ccol[crp[r]:crp[r + 1]], np.unique(col[rp[r]:rp[r + 1]]))
    for fmt in sv.EXACT_REACH:
        rrp, rcol = sv.reach({"format": fmt}, rp, col, m, n)
        assert np.array_equal(rrp, crp) and np.array_equal(rcol, ccol)
    for fmt in sv.PADDED_REACH:
        rrp, rcol = sv.reach({"format": fmt}, rp, col, m, n)
        extra = np.diff(rrp) - np.diff(crp)
        assert np.array_equal(extra, (lens == 0).astype(np.int64))
        assert (rcol[rrp[:-1][lens == 0]] == 0).all()
        keep = np.ones(len(rcol), bool)
        keep[rrp[:-1][lens == 0]] = False
        assert np.array_equal(rcol[keep], ccol)
    if name not in ("uniform16", "banded"):  # no empty row there
        assert (lens == 0).any()


def _is_superset(rrp, rcol, crp, ccol, n):
    m = len(rrp) - 1
    a = np.repeat(np.arange(m), np.diff(rrp)) * n + rcol
    b = np.repeat(np.arange(m), np.diff(crp)) * n + ccol
    return np.isin(b, a).all()


@pytest.mark.parametrize("name", ["banded", "rect513x40", "rect7x1000"])
def test_reach_of_dia_holds_the_rows_columns(name):
    m, n, rp, col = si.structure(name)
    rrp, rcol = sv.reach({"format": "dia"}, rp, col, m, n)
    assert _is_superset(rrp, rcol, *sv.cols_of(rp, col, m, n), n)
    assert (rcol >= 0).all() and (rcol < n).all()


def test_reach_of_dia_clamps_at_the_matrix_edges():
    """Diagonals -2 and +2 of a 9 x 9 matrix: rows 0, 1 have no entry on -2
    and rows 7, 8 none on +2; their zero-filled slots read the clamped x[0] /
    x[8], columns these rows do not reference.  On `banded` the first and last
    40 rows have such slots too, but with every diagonal of the band present
    the clamp targets (columns 0 and n - 1) are columns those rows reference
    anyway: reach = cols there."""
    m = n = 9
    rows, cols = [], []
    for r in range(m):
        for o in (-2, 2):
            if 0 <= r + o < n:
                rows.append(r)
                cols.append(r + o)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    rrp, rcol = sv.reach({"format": "dia"}, rp, np.array(cols), m, n)
    got = [rcol[rrp[r]:rrp[r + 1]].tolist() for r in range(m)]
    assert got == [[0, 2], [0, 3], [0, 4], [1, 5], [2, 6], [3, 7], [4, 8], [5, 8], [6, 8]]
    poisoned = np.zeros(n, bool)
    poisoned[[0, 8]] = True
    assert sv.rows_touching(rrp, rcol, poisoned).tolist() == [True, True, True, False, False, False, True, True, True]
    assert sv.rows_touching(*sv.cols_of(rp, np.array(cols), m, n), poisoned).tolist() == [
        False, False, True, False, False, False, True, False, False]

    m, n, rp, col = si.structure("banded")
    row = np.repeat(np.arange(m), np.diff(rp))
    off = np.unique(col - row)
    assert off.tolist() == list(range(-40, 41))
    clamped = ((np.arange(m)[:, None] + off[None, :] < 0) | (np.arange(m)[:, None] + off[None, :] >= n)).any(axis=1)
    assert np.array_equal(np.flatnonzero(clamped), np.concatenate([np.arange(40), np.arange(m - 40, m)]))
    rrp, rcol = sv.reach({"format": "dia"}, rp, col, m, n)
    crp, ccol = sv.cols_of(rp, col, m, n)
    assert np.array_equal(rrp, crp) and np.array_equal(rcol, ccol)


# ---------------------------------------------------------------- the checkers catch what they exist for
def _exact_reached(c):
    return sv.rows_touching(*sv.reach(EXACT, c["rp"], c["col"], c["m"], c["n"]), c["poisoned"])


def _flagged(c, y):
    return sv.poison_failing_rows(y, c["y_clean"], c["hit"], _exact_reached(c), y_class=sv.classify(c["y_oracle"]))


def _leak(c, rows, cols):
    """The oracle's y with a 0 * x[cols] term added to `rows`, and the rows it
    changes: those out of the poison's reach that now hold NaN, and hit rows
    whose +-Inf became NaN."""
    y = c["y_oracle"].copy()
    with np.errstate(invalid="ignore"):
        y[rows] = y[rows] + 0.0 * c["x"][cols]
    got = c["poisoned"][cols] & (~c["hit"][rows] | np.isinf(c["y_oracle"][rows]))
    return y, rows[got]


@pytest.mark.parametrize("case", [sv.forward_case, sv.inverse_case])
@pytest.mark.parametrize("name", si.STRUCTURES)
def test_checker_catches_a_leak_from_the_next_row(name, case):
    """mask * v instead of a select at a row boundary: row r also adds
    0 * x[first column of the next non-empty row]."""
    c = case(name)
    rp, col = c["rp"], c["col"]
    starts = rp[:-1][_nonempty(c)]
    nxt = np.searchsorted(starts, rp[1:], side="left")  # the first non-empty row after r
    rows = np.flatnonzero(nxt < len(starts))
    y, affected = _leak(c, rows, col[starts[nxt[rows]]])
    assert np.array_equal(_flagged(c, y), affected), name
    # nothing to see in two cases: rect7x1000's one poisoned reference is row 0's (no row before it); in
    # `banded` the next row's first column is one of row r's own, finite whenever an inverse-clean row r is
    if (name, case) in (("rect7x1000", sv.forward_case), ("banded", sv.inverse_case)):
        assert len(affected) == 0
        return
    assert len(affected) >= 1
    with pytest.raises(AssertionError, match="poisoned-x contract"):
        sv.assert_poisoned(y, c["y_clean"], c["hit"], _exact_reached(c), name, y_class=sv.classify(c["y_oracle"]))


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_checker_catches_a_leak_from_the_pad_column(name):
    """A pad slot (column 0) multiplied into every 64th row."""
    c = sv.forward_case(name)
    rows = np.arange(0, c["m"], 64)
    y, affected = _leak(c, rows, np.zeros(len(rows), np.int64))
    if name != "rect7x1000":  # its only 64th row, row 0, references column 0 itself
        assert len(affected) >= 1
    assert np.array_equal(_flagged(c, y), affected), name
    # ELL's reach absorbs the empty rows among them and nothing else
    reached = sv.rows_touching(*sv.reach({"format": "ell"}, c["rp"], c["col"], c["m"], c["n"]), c["poisoned"])
    bad = sv.poison_failing_rows(y, c["y_clean"], c["hit"], reached)
    assert np.array_equal(bad, affected[_nonempty(c)[affected] & ~c["hit"][affected]])


@pytest.mark.parametrize("name", [s for s in si.STRUCTURES if s != "rect7x1000"])
def test_checker_catches_a_class_swap(name):
    """+Inf reported as NaN: caught where the class is asserted (the
    exact-reach layouts), on exactly the +Inf rows."""
    c = sv.forward_case(name)
    rows = np.flatnonzero(c["y_oracle"] == np.inf)
    assert len(rows) >= 1
    y = c["y_oracle"].copy()
    y[rows] = np.nan
    assert np.array_equal(_flagged(c, y), rows)
    assert len(sv.poison_failing_rows(y, c["y_clean"], c["hit"], _exact_reached(c))) == 0  # not without the class


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_checker_catches_a_finite_hit_row_and_a_changed_clean_row(name):
    c = sv.forward_case(name)
    h, k = np.flatnonzero(c["hit"])[0], np.flatnonzero(~c["hit"] & _nonempty(c))[0]
    y = c["y_oracle"].copy()
    y[h] = c["y_clean"][h]  # the poisoned entry skipped (a pad fix keyed on val == 0)
    y[k] = np.nextafter(y[k], np.inf)
    want = [int(h), int(k)]
    if not _nonempty(c).all():  # an empty row's +0.0 turned -0.0
        want.append(int(np.flatnonzero(~_nonempty(c))[0]))
        y[want[-1]] = -0.0
    assert _flagged(c, y).tolist() == sorted(want)


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_checker_catches_flushed_products(name):
    """Every 3rd row summed from products flushed to zero (y = 0): flagged on
    exactly those whose reference exceeds tiny_tol."""
    c = sv.extreme_case(name, "tiny")
    rows = np.arange(0, c["m"], 3)
    y = c["y_oracle"].copy()
    y[rows] = 0.0
    big = np.abs(c["ref"][0]) > sv.tiny_tol(c["rp"])
    bad, _ = sv.tiny_failing_rows(y, c["rp"], c["ref"])
    assert big[rows].any() and np.array_equal(bad, rows[big[rows]])
    with pytest.raises(AssertionError, match="beyond the tiny bound"):
        sv.assert_extreme("tiny", y, c["rp"], c["ref"], name)
    # inputs flushed instead (x = 0 to the kernel): the same rows
    y0 = oracle.csr_spmv(c["rp"], c["col"], np.ascontiguousarray(c["val"]), np.zeros(c["n"]))
    assert np.array_equal(sv.tiny_failing_rows(y0, c["rp"], c["ref"])[0], np.flatnonzero(big))


@pytest.mark.parametrize("name", si.STRUCTURES)
def test_checker_catches_f32_range_products(name):
    """Every 3rd row with its products formed in f32 range (2^1000 overflows
    to Inf there): flagged on exactly those rows that have an entry."""
    c = sv.extreme_case(name, "huge")
    rp, col = c["rp"], c["col"]
    with np.errstate(over="ignore", invalid="ignore"):
        p = (c["val"].astype(np.float32) * c["x"][col].astype(np.float32)).astype(np.float64)
        y32 = si._segment_sums(p, rp)
    rows = np.arange(0, c["m"], 3)
    y = c["y_oracle"].copy()
    y[rows] = y32[rows]
    bad, _ = si.failing_rows(y, rp, c["ref"])
    assert np.array_equal(bad, rows[_nonempty(c)[rows]])
    with pytest.raises(AssertionError, match="beyond the huge bound"):
        sv.assert_extreme("huge", y, rp, c["ref"], name)
