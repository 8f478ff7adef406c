"""tests/dot_inputs.py on the CPU: the exact sums are exact, the integer family
is what it says, and the checker of tests/test_gpu_dot.py can fail -- dots
that drop or double a term, carry a stale slot of an earlier call or include
the row past the end are rejected on every structure, while the correctly
rounded dots and any re-ordering of the adds pass.
"""
from fractions import Fraction

import numpy as np
import pytest

import dot_inputs as di
import signed_inputs as si

CHECKED = ("staircase", "uniform16", "banded")
# staircase's last row is the 9000-entry one: its `cancel` sum is rounding
# noise (1e-13 against a bound of 1e-10), so one more term of it is invisible
# to any bound on that family; test_checker_rejects_wrong_dots_of_the_integer_family
# shows the checker rejecting it on staircase, where the term is an integer >= 1
BELOW_THE_BOUND = {("staircase", "w[m] * y[m - 1] included")}


def _round(f):
    """The double nearest to a Fraction (Python's int / int division rounds correctly)."""
    return f.numerator / f.denominator


def test_w_is_seeded_signed_and_bounded():
    a, b = di.w(1000), di.w(1000)
    assert a is b and not a.flags.writeable
    assert ((np.abs(a) >= 0.5) & (np.abs(a) <= 2.0)).all() and (a < 0).any() and (a > 0).any()
    assert not np.array_equal(di.w(1000, 1), a)


def test_exact_sums_against_plain_fractions():
    rng = np.random.default_rng(1)
    a = rng.standard_normal(300) * 10.0 ** rng.integers(-200, 200, 300)
    b = rng.standard_normal(300) * 10.0 ** rng.integers(-100, 100, 300)
    a[7], b[9] = 0.0, -0.0
    a[11] = 5e-324  # subnormal
    s, mag = di.exact_sums(a, b)
    ts = [Fraction(float(p)) * Fraction(float(q)) for p, q in zip(a, b)]
    assert s == sum(ts) and mag == sum(abs(t) for t in ts)
    assert di.exact_sums(np.zeros(0), np.zeros(0)) == (0, 0)
    with pytest.raises(AssertionError):
        di.exact_sums(np.array([np.nan]), np.array([1.0]))


@pytest.mark.parametrize("name", si.STRUCTURES + ("tri1500",))
def test_integer_family_is_exact(name):
    c = di.int_case(name)
    m = c["m"]
    assert set(np.unique(c["val"])) <= set(range(1, 10)) and set(np.unique(c["x"])) <= set(range(1, 10))
    assert set(np.unique(c["w"])) <= {1.0, 2.0, 3.0} and len(c["w"]) == m and len(c["y"]) == m
    # y against the exact rows, the dots against the exact reference over that y
    ref = si.ref_rows(c["rp"], c["col"], c["val"], c["x"])[0]
    assert np.array_equal(ref.astype(np.float64), c["y"])
    (t, a0), (q, _) = di.reference(c["y"], c["w"])
    assert t == c["wy"] == a0 and q == c["yy"]
    assert c["wy"] < 2 ** 53 and c["yy"] < 2 ** 53
    assert di.failures((float(c["wy"]), float(c["yy"])), c["y"], c["w"]) == []
    assert di.ratios((float(c["wy"]), float(c["yy"])), c["y"], c["w"]) == [0.0, 0.0]


@pytest.mark.parametrize("name", CHECKED)
def test_checker_accepts_what_it_must(name):
    c = si.case(name, "cancel")
    y, m = c["y_oracle"], c["m"]
    wv = di.w(m)
    (t, _), (q, _) = di.reference(y, wv)
    assert di.failures((_round(t), _round(q)), y, wv) == []
    # any order of rounded adds: ascending, descending, pairwise (numpy)
    p = np.multiply(wv, y)
    s = np.multiply(y, y)
    for d0, d1 in ((float(np.sum(p)), float(np.sum(s))),
                   (float(np.cumsum(p)[-1]), float(np.cumsum(s)[-1])),
                   (float(np.cumsum(p[::-1])[-1]), float(np.cumsum(s[::-1])[-1]))):
        assert di.failures((d0, d1), y, wv) == [], (d0, d1)
    # no w: +0.0, and only +0.0
    assert di.failures((0.0, _round(q)), y, None) == []
    assert di.failures((-0.0, _round(q)), y, None) != []
    assert di.failures((1e-300, _round(q)), y, None) != []
    # dots[1] must not be negative, NaN is no dot of finite data
    assert di.failures((_round(t), -_round(q)), y, wv) != []
    assert di.failures((float("nan"), _round(q)), y, wv) != []
    assert di.failures((_round(t), float("inf")), y, wv) != []


@pytest.mark.parametrize("name", CHECKED)
def test_checker_rejects_wrong_dots(name):
    c = si.case(name, "cancel")
    y, m = c["y_oracle"], c["m"]
    wv = di.w(m + 1)  # one entry past the end, for the last mutation
    w_in = wv[:m]
    (t, _), (q, _) = di.reference(y, w_in)
    good = (_round(t), _round(q))
    assert di.failures(good, y, w_in) == []
    tw = di.terms(y, w_in)
    tq = di.terms(y, y)
    big_w = max(range(m), key=lambda r: abs(tw[r]))
    big_q = max(range(m), key=lambda r: tq[r])
    some = m // 3
    while tw[some] == 0:
        some += 1
    # a stale slot: the pair a 256-row workgroup left in an earlier call with another w
    stale_w = sum(tw[256:512]) * 3
    stale_q = sum(tq[256:512])
    assert stale_w != 0 and stale_q != 0 and y[m - 1] != 0
    mutations = {
        "largest term dropped": (t - tw[big_w], q - tq[big_q]),
        "one term doubled": (t + tw[some], q + tq[some]),
        "a stale slot added": (t + stale_w, q + stale_q),
        "w[m] * y[m - 1] included": (t + Fraction(float(wv[m])) * Fraction(float(y[m - 1])), None),
    }
    for what, (t2, q2) in mutations.items():
        bad = di.failures((_round(t2), good[1]), y, w_in)
        if (name, what) in BELOW_THE_BOUND:
            # the extra term is rounding noise of a cancelling row, smaller than the bound
            # itself: no bound can see it on this family; the checker does on the integer one (next test)
            assert abs(t2 - t) < di.tol(m, di.reference(y, w_in)[0][1])
            continue
        assert any("dots[0]" in b for b in bad), f"{name}: {what} in dots[0] passed"
        if q2 is not None:
            bad = di.failures((good[0], _round(q2)), y, w_in)
            assert any("dots[1]" in b for b in bad), f"{name}: {what} in dots[1] passed"


def _exact(dots, c):
    """The integer family's check in tests/test_gpu_dot.py: the bits of the exact integers."""
    return di.bits(dots).tolist() == di.bits((float(c["wy"]), float(c["yy"]))).tolist()


@pytest.mark.parametrize("name", CHECKED)
def test_checker_rejects_wrong_dots_of_the_integer_family(name):
    """The same four mutations on the integer family, through both checks the
    GPU test applies to it: the bound (di.failures) and the bit-exact
    comparison.  Every term is an integer >= 1 there and the bound is about
    1e-4 or less, so every mutation -- the row past the end of `staircase`
    included -- is rejected by both."""
    c = di.int_case(name)
    y, m = c["y"], c["m"]
    wv = np.concatenate([c["w"], [2.0]])  # one entry past the end, for the last mutation
    w_in = c["w"]
    good = (float(c["wy"]), float(c["yy"]))
    assert di.failures(good, y, w_in) == [] and _exact(good, c)
    assert float(di.tol(m, di.reference(y, w_in)[0][1])) < 0.5
    tw = [int(a) * int(b) for a, b in zip(w_in, y)]
    tq = [int(b) * int(b) for b in y]
    assert sum(tw) == c["wy"] and sum(tq) == c["yy"] and y[m - 1] >= 1
    some = next(r for r in range(m // 3, m) if tw[r])
    mutations = {
        "largest term dropped": (c["wy"] - max(tw), c["yy"] - max(tq)),
        "one term doubled": (c["wy"] + tw[some], c["yy"] + tq[some]),
        "a stale slot added": (c["wy"] + 3 * sum(tw[256:512]), c["yy"] + sum(tq[256:512])),
        "w[m] * y[m - 1] included": (c["wy"] + int(wv[m]) * int(y[m - 1]), None),
    }
    for what, (wy, yy) in mutations.items():
        bad = di.failures((float(wy), good[1]), y, w_in)
        assert any("dots[0]" in b for b in bad), f"{name}: {what} in dots[0] passed the bound"
        assert not _exact((float(wy), good[1]), c), f"{name}: {what} in dots[0] passed the exact check"
        if yy is not None:
            bad = di.failures((good[0], float(yy)), y, w_in)
            assert any("dots[1]" in b for b in bad), f"{name}: {what} in dots[1] passed the bound"
            assert not _exact((good[0], float(yy)), c), f"{name}: {what} in dots[1] passed the exact check"
