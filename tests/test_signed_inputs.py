"""CPU checks of tests/signed_inputs.py: the reference, the bound, the value
families and the checker itself -- what keeps tests/test_gpu_signed.py honest.
"""
import numpy as np
import pytest

import oracle
import signed_inputs as si

FAMILIES = sorted(si.FAMILIES)


def _oracle(rp, col, val, x):
    return oracle.csr_spmv(np.ascontiguousarray(rp, np.int64), np.ascontiguousarray(col, np.int32),
                           np.ascontiguousarray(val, np.float64), np.ascontiguousarray(x, np.float64))


def test_reference_handles_empty_rows_and_matches_exact_sums():
    """ref_rows on a matrix with empty rows at the start, in the middle and
    at the end (np.add.reduceat alone returns a neighbour's element there),
    against exact rational arithmetic."""
    assert si.LONGDOUBLE_OK, "np.longdouble has fewer than 63 mantissa bits: ref_rows falls back to Fraction"
    rp = np.array([0, 0, 3, 3, 3, 7, 8, 8], np.int64)
    rng = np.random.default_rng(1)
    col = rng.integers(0, 5, 8).astype(np.int32)
    val, x = si.spread(rp, col, 5, seed=2)
    y, mag = si.ref_rows(rp, col, val, x)
    ye, mage = si._ref_rows_fraction(rp, col, val, x)
    assert (y[[0, 2, 3, 6]] == 0).all() and (mag[[0, 2, 3, 6]] == 0).all()
    assert np.all(np.abs(y - ye) <= 8 * 2.0 ** -64 * mage) and np.all(np.abs(mag - mage) <= 8 * 2.0 ** -64 * mage)
    # rows with mag == 0 must give y == 0, NaN never passes
    bad, _ = si.failing_rows(np.array([0, ye[1], 1e-300, 0, ye[4], np.nan, 0], np.float64), rp, (y, mag))
    assert bad.tolist() == [2, 5]


def test_structures_are_what_the_gpu_tests_rely_on():
    seen = {name: (m, n, rp, col) for name, m, n, rp, col in si.structures()}
    assert list(seen) == list(si.STRUCTURES)
    for name, (m, n, rp, col) in seen.items():
        assert len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(col) and (np.diff(rp) >= 0).all(), name
        assert col.dtype == np.int32 and (col >= 0).all() and (col < n).all(), name
        # ascending columns within every row (the sequential layouts' premise)
        inner = np.ones(len(col), bool)
        inner[rp[:-1][np.diff(rp) > 0]] = False
        assert (np.diff(col, prepend=0)[inner] >= 0).all(), name
    m, n, rp, col = seen["staircase"]
    lens = np.diff(rp)
    assert (m, n) == (2048, 2048) and set(si.STAIR_LENS) | {4096, 4097, 9000} == set(lens.tolist())
    r = 2047
    assert lens[r] == 9000 and (np.diff(col[rp[r]:rp[r + 1]]) == 0).any()  # sorted, with duplicates
    # adaptive CSR: no length bin holds 99 % of the rows
    edges = np.array([4, 8, 16, 32, 64, 128, 4096])
    assert np.bincount(np.searchsorted(edges, lens), minlength=8).max() < 0.99 * m
    m, n, rp, col = seen["powerlaw"]
    assert rp[1] == 0 and rp[-1] == rp[-2] and np.diff(rp).max() > 700
    assert seen["uniform16"][0] % 64 and (np.diff(seen["uniform16"][2]) == 16).all()
    lens = np.diff(seen["banded"][2])
    assert lens.max() == 81 and lens[0] == 41 and lens[-1] == 41
    assert set(np.diff(seen["short"][2]).tolist()) == {0, 1, 2, 3}
    assert (seen["rect513x40"][:2], seen["rect7x1000"][:2]) == ((513, 40), (7, 1000))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", si.STRUCTURES)
def test_sequential_sum_is_within_the_bound(name, family):
    """The oracle's sequential double sum passes assert_rows (err / row_tol
    <= 1 by derivation; the figure is printed, never asserted)."""
    c = si.case(name, family)
    worst = si.assert_rows(c["y_oracle"], c["rp"], c["col"], c["val"], c["x"], f"oracle {name}/{family}", ref=c["ref"])
    print(f"oracle err/row_tol {name}/{family}: {worst:.3f}")
    assert worst <= 1.0, f"oracle {name}/{family}: err/row_tol {worst:.3f}"


def _reversed_rows(rp, a):
    """a with the entries of every row in reverse order."""
    lens = np.diff(rp)
    pos = np.arange(len(a)) - np.repeat(rp[:-1], lens)
    return a[np.repeat(rp[1:], lens) - 1 - pos]


@pytest.mark.parametrize("family", FAMILIES)
def test_families_are_order_sensitive(family):
    """Over the rows with >= 3 entries, summing in reverse order changes the
    bits of at least half the sequential sums: a kernel that adds in another
    order than it claims cannot pass a bit-exact assertion by luck."""
    changed = total = 0
    for name in si.STRUCTURES:
        c = si.case(name, family)
        rp = c["rp"]
        yr = _oracle(rp, _reversed_rows(rp, c["col"]), _reversed_rows(rp, c["val"]), c["x"])
        rows = np.diff(rp) >= 3
        n_changed = int((yr[rows] != c["y_oracle"][rows]).sum())
        print(f"order-sensitive rows {name}/{family}: {n_changed} of {int(rows.sum())}")
        changed += n_changed
        total += int(rows.sum())
    assert changed >= 0.5 * total, f"{family}: only {changed} of {total} rows change with the add order"


def test_cancel_rows_cancel():
    """|y_hi| <= 1e-12 sum |a x| on >= 95 % of cancel's even-length rows."""
    for name in si.STRUCTURES:
        c = si.case(name, "cancel")
        lens = np.diff(c["rp"])
        rows = (lens >= 2) & (lens % 2 == 0)
        y_hi, mag = c["ref"]
        ok = np.abs(y_hi[rows]) <= 1e-12 * mag[rows]
        assert rows.sum() > 0 and ok.sum() >= 0.95 * rows.sum(), f"{name}: {int(ok.sum())} of {int(rows.sum())} rows cancel"
        assert (mag[lens > 0] >= 0.5 * lens[lens > 0] * (1 - 1e-12)).all(), name  # every |a x| is in [0.5, 2]


def _one_row_per_length_class(rp):
    """One row (the first) of every length class: each distinct length up to
    129 and the adaptive-CSR bins beyond (<= 4096, > 4096)."""
    lens = np.diff(rp)
    cls = np.where(lens <= 129, lens, np.where(lens <= 4096, 4096, 4097))
    rows = []
    for k in np.unique(cls[lens > 0]):
        rows.append(int(np.flatnonzero(cls == k)[0]))
    return rows


def _perturbed(kind, rp, col, val, n, rows):
    """The CSR with one entry of each of `rows` dropped (its last), doubled
    (its middle one stored twice) or gathering x from the next column."""
    rp, col, val = np.array(rp), np.array(col), np.array(val)
    if kind == "gather":
        for r in rows:
            js = np.arange(rp[r], rp[r + 1])
            js = js[col[js] < n - 1]
            col[js[len(js) // 2]] += 1
        return rp, col, val
    at = np.array([rp[r + 1] - 1 if kind == "drop" else (rp[r] + rp[r + 1]) // 2 for r in rows])
    if kind == "drop":
        col, val = np.delete(col, at), np.delete(val, at)
        step = -1
    else:
        col, val = np.insert(col, at, col[at]), np.insert(val, at, val[at])
        step = 1
    bump = np.zeros(len(rp), np.int64)
    bump[np.asarray(rows) + 1] = step
    return rp + np.cumsum(bump), col, val


@pytest.mark.parametrize("kind", ["drop", "double", "gather"])
@pytest.mark.parametrize("name", ["staircase", "powerlaw"])
def test_checker_catches_one_wrong_entry(name, kind):
    """One entry dropped, added twice or multiplied by the wrong x in one row
    per length class: assert_rows against the unperturbed reference fails on
    exactly those rows."""
    c = si.case(name, "cancel")
    rows = _one_row_per_length_class(c["rp"])
    assert len(rows) >= 12
    rp2, col2, val2 = _perturbed(kind, c["rp"], c["col"], c["val"], c["n"], rows)
    assert int(rp2[-1]) == int(c["rp"][-1]) + {"drop": -1, "double": 1, "gather": 0}[kind] * len(rows)
    y = _oracle(rp2, col2, val2, c["x"])
    bad, _ = si.failing_rows(y, c["rp"], c["ref"])
    assert bad.tolist() == sorted(rows), f"{name}/{kind}: perturbed {sorted(rows)}, flagged {bad.tolist()}"
    with pytest.raises(AssertionError, match="beyond row_tol"):
        si.assert_rows(y, c["rp"], c["col"], c["val"], c["x"], f"{name}/{kind}", ref=c["ref"])
    for r in rows:  # each perturbed row alone is caught too
        y1 = c["y_oracle"].copy()
        y1[r] = y[r]
        assert si.failing_rows(y1, c["rp"], c["ref"])[0].tolist() == [r]
