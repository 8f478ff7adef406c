"""CPU checks of tests/axpby_inputs.py: the reference, y0 and the bound --
what keeps tests/test_gpu_axpby.py honest.
"""
import numpy as np
import pytest

import axpby_inputs as ai
import signed_inputs as si

U = 2.0 ** -53


def test_alpha_beta_list_is_the_issues():
    assert ai.ALPHA_BETA == ((1, 1), (1, -1), (-2.5, 0.75), (0.3, 1e-3), (0, 2), (2, -0.0))
    assert np.signbit(ai.ALPHA_BETA[-1][1]) and ai.ALPHA_BETA[-1][1] == 0


def test_y0_is_signed_mixed_magnitude_and_shared():
    y = ai.y0(20011)
    assert y is ai.y0(20011) and not y.flags.writeable
    assert (y != 0).all() and (y < 0).any() and (y > 0).any()
    assert 0.5e-4 <= np.abs(y).min() < 1e-3 and 1e3 < np.abs(y).max() <= 1e4
    assert not np.array_equal(y[:100], ai.y0(20011, seed=1)[:100])


@pytest.mark.parametrize("alpha,beta", ai.ALPHA_BETA)
def test_expected_against_longdouble(alpha, beta):
    """Two rounded multiplies and a rounded add stay within
    2^-53 (1 + 2^-52) * 2 (|alpha s| + |beta y0|) of the extended evaluation;
    with exact products (alpha, beta in {0, +-1, +-2}) the add is the only
    rounding: half an ulp of the result."""
    assert si.LONGDOUBLE_OK
    rng = np.random.default_rng(3)
    s = rng.choice([-1.0, 1.0], 5000) * rng.uniform(0.5, 1.0, 5000) * 10.0 ** rng.integers(-6, 7, 5000)
    y0 = ai.y0(5000)
    e = ai.expected(s, y0, alpha, beta)
    L = np.longdouble
    want = L(alpha) * s.astype(L) + (L(beta) * y0.astype(L) if beta != 0 else 0)
    mag = abs(alpha) * np.abs(s) + abs(beta) * np.abs(y0)
    assert np.all(np.abs(e.astype(L) - want) <= 2 * U * (1 + 2 * U) * mag)
    if all(v in (0.0, 1.0, -1.0, 2.0, -2.0) for v in (alpha, beta)):
        assert np.all(np.abs(e.astype(L) - want) <= np.spacing(np.abs(e)) / 2)
    # the products are rounded on their own: an FMA of the second one differs somewhere
    if (alpha, beta) == (-2.5, 0.75):
        fma = (L(alpha) * s.astype(L) + L(beta) * y0.astype(L)).astype(np.float64)
        assert (fma != e).any()


def test_beta_zero_ignores_y0():
    s = np.array([1.5, -0.0, 0.0, np.inf, -3.0])
    nan = np.full(5, np.nan)
    with np.errstate(invalid="ignore"):  # 0 * Inf
        for beta in (0.0, -0.0):
            for alpha in (1.0, -2.5, 0.0):
                e = ai.expected(s, nan, alpha, beta)
                assert np.array_equal(ai.bits(e), ai.bits(np.float64(alpha) * s))
        # alpha = 0 is no shortcut: 0 * Inf is NaN, and the zeros keep their signs
        e = ai.expected(s, nan, 0.0, 0.0)
    assert np.isnan(e[3]) and np.signbit(e[1]) and not np.signbit(e[2]) and np.signbit(e[4])
    # beta != 0 does read it
    assert np.isnan(ai.expected(s, nan, 1.0, 1.0)).all()


def test_bound_accepts_the_reference_and_rejects_a_wrong_row():
    c = si.case("rect513x40", "cancel")
    rp, ref = c["rp"], c["ref"]
    y0 = ai.y0(c["m"])
    s = c["y_oracle"]
    for alpha, beta in ai.ALPHA_BETA:
        y = ai.expected(s, y0, alpha, beta)
        worst = ai.assert_bound(y, rp, ref, y0, alpha, beta, "oracle")
        assert worst <= 1.0
        bad = y.copy()
        r = 100
        # a beta applied twice, a y0 dropped, one entry of the row (>= 0.5 in `cancel`) dropped
        for wrong in (y[r] + beta * y0[r], alpha * s[r], alpha * (s[r] + 0.5) + beta * y0[r]):
            if wrong == y[r]:
                continue
            bad[r] = wrong
            rows, _ = ai.failing_rows(bad, rp, ref, y0, alpha, beta)
            assert rows.tolist() == [r], (alpha, beta, wrong, y[r])
        bad[r] = np.nan
        assert ai.failing_rows(bad, rp, ref, y0, alpha, beta)[0].tolist() == [r]


def test_bound_formula():
    """tol = |alpha| row_tol + 3 * 2^-53 (|alpha| mag + |beta y0|), want = alpha y_hi + beta y0."""
    rp = np.array([0, 2, 2, 5], np.int64)
    y_hi = np.array([1.0, 0.0, -3.0], np.longdouble)
    mag = np.array([4.0, 0.0, 8.0], np.longdouble)
    y0 = np.array([10.0, -20.0, 0.5])
    want, tol = ai.bound(rp, (y_hi, mag), y0, -2.0, 0.5)
    assert np.array_equal(want, np.array([-2 + 5, -10, 6 + 0.25], np.longdouble))
    rt = si.row_tol(rp, mag)
    assert np.array_equal(tol, 2 * rt + 3 * np.longdouble(U) * (2 * mag + np.abs(0.5 * y0.astype(np.longdouble))))
    # beta = 0: y0 is not looked at
    want0, tol0 = ai.bound(rp, (y_hi, mag), np.full(3, np.nan), -2.0, -0.0)
    assert np.array_equal(want0, -2 * y_hi) and np.array_equal(tol0, 2 * rt + 3 * np.longdouble(U) * 2 * mag)


@pytest.mark.parametrize("name", ai.REFRESH_STRUCTURES)
def test_refresh_cases_differ_on_most_rows(name):
    """The two value sets of refresh_cases share the pattern and x, each
    passes its own bound, and with the reference alone y = -2.5 A x + 0.75 y0
    differs between them on at least half of the non-empty rows (here: on all
    of them) -- a refreshed plan that still computed with A cannot pass as B."""
    a, b = ai.refresh_cases(name)
    assert a["rp"] is b["rp"] and a["col"] is b["col"] and a["x"] is b["x"] and a["val"].shape == b["val"].shape
    assert not np.array_equal(a["val"], b["val"])
    y0 = ai.y0(b["m"])
    ya, yb = (ai.expected(c["y_oracle"], y0, -2.5, 0.75) for c in (a, b))
    for c, y in ((a, ya), (b, yb)):
        assert ai.assert_bound(y, c["rp"], c["ref"], y0, -2.5, 0.75, f"{name} {c['family']}") <= 1.0
    live = np.diff(b["rp"]) > 0
    assert np.array_equal(ai.bits(ya[~live]), ai.bits(yb[~live]))
    assert (ai.bits(ya) != ai.bits(yb))[live].all()
    assert len(ai.failing_rows(ya, b["rp"], b["ref"], y0, -2.5, 0.75)[0]) >= live.sum() // 2  # and far beyond B's bound
