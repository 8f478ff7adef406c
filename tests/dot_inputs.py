"""Inputs, the exact reference and the bound for Plan.execute_dot
(y = A x, dots[0] = sum w[r] y[r], dots[1] = sum y[r]^2).

The reference is exact: over the y the call returned, T = sum w[r] y[r] and
Q = sum y[r]^2 as rationals (fractions.Fraction; a double is a dyadic
rational, so are its products and their sums), with A0 = sum |w[r] y[r]| and
Q itself as the magnitudes.  The bound the header promises for every path and
format,

    |dots[0] - T| <= (m + 8) * 2^-53 * A0,   |dots[1] - Q| <= (m + 8) * 2^-53 * Q,

is compared in rationals too, so the check itself rounds nothing.
Derivation: each term is one rounded product (relative error u = 2^-53), the
m terms meet in at most m - 1 rounded adds in any order -- lanes, butterflies,
waves, slots -- which errs by at most gamma_m * sum |term|, gamma_n = n u /
(1 - n u); the 8 covers the second-order terms for every m below 2^31
(signed_inputs.row_tol has the same shape).  No order of the adds passes that
drops, doubles or adds a term of the `cancel` family's y: one term is about
1 / m of the magnitude, the bound about m * 1e-16 of it.

The integer family (val, x in 1..9, w in 1..3 on the structures of
signed_inputs) makes every y[r], every term and every partial sum an integer
below 2^53: every add order is exact, and the dots must equal Python-int
arithmetic bit for bit.

Plain helper module (numpy only, besides signed_inputs / multi_inputs);
tests/test_dot_inputs.py checks it on the CPU, tests/test_gpu_dot.py uses it
on the GPU.
"""
import functools
from fractions import Fraction

import numpy as np

import multi_inputs as mi
import signed_inputs as si

U = Fraction(1, 2 ** 53)
POS_ZERO_BITS = 0


def bits(a):
    """The int64 patterns of a float64 array (NaN payloads and signed zeros count)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def w(m, seed=0):
    """A seeded w of m entries, +-U(0.5, 2); never zero.  Shared and
    read-only: copy it before writing."""
    rng = np.random.default_rng(9000 + seed)
    v = rng.choice([-1.0, 1.0], m) * rng.uniform(0.5, 2.0, m)
    v.setflags(write=False)
    return v


# ---------------------------------------------------------------- exact sums
def _mant_exp(a):
    """Finite doubles as (integer mantissa, exponent) lists: a = mant * 2^exp."""
    a = np.asarray(a, np.float64)
    assert np.isfinite(a).all(), "the exact reference takes finite values"
    f, e = np.frexp(a)
    mant = np.ldexp(f, 53).astype(np.int64)  # |f| < 1: 53 bits, exact
    return mant.tolist(), (e.astype(np.int64) - 53).tolist()


def exact_sums(a, b):
    """(sum a[i] b[i], sum |a[i] b[i]|) as Fractions, exact.  Integer
    arithmetic on the mantissas at the smallest exponent (tests/test_dot_inputs.py
    holds it against the plain sum of Fraction(a[i]) * Fraction(b[i]))."""
    ma, ea = _mant_exp(a)
    mb, eb = _mant_exp(b)
    if not ma:
        return Fraction(0), Fraction(0)
    ex = [p + q for p, q in zip(ea, eb)]
    emin = min(ex)
    s = mag = 0
    for p, q, e in zip(ma, mb, ex):
        t = (p * q) << (e - emin)
        s += t
        mag += abs(t)
    scale = Fraction(2) ** emin
    return s * scale, mag * scale


def terms(y, wv):
    """The exact terms w[r] y[r] as Fractions (the mutations of
    tests/test_dot_inputs.py pick among them)."""
    return [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(wv, y)]


def reference(y, wv):
    """((T, A0), (Q, Q)): the exact dots over the y a call returned and their
    magnitudes.  wv None: T = A0 = 0."""
    y = np.asarray(y, np.float64)
    q, _ = exact_sums(y, y)
    if wv is None:
        return (Fraction(0), Fraction(0)), (q, q)
    return exact_sums(np.asarray(wv, np.float64)[:len(y)], y), (q, q)


def tol(m, mag):
    """(m + 8) * 2^-53 * mag, a Fraction (module docstring)."""
    return (m + 8) * U * mag


def ratios(dots, y, wv):
    """err / tol of the two dots (a measurement; inf for a non-finite dot or
    an error with tol == 0, 0.0 for an exact dot)."""
    m = len(y)
    out = []
    for d, (want, mag) in zip(dots, reference(y, wv)):
        d = float(d)
        if not np.isfinite(d):
            out.append(float("inf"))
            continue
        err, t = abs(Fraction(d) - want), tol(m, mag)
        out.append(0.0 if err == 0 else float("inf") if t == 0 else float(err / t))
    return out


def failures(dots, y, wv):
    """The reasons (dots[0], dots[1]) over this y and w break the contract; []
    when they meet it: both within the bound, dots[1] >= 0, and with w None
    dots[0] the bits of +0.0."""
    bad = []
    r = ratios(dots, y, wv)
    for k, v in enumerate(r):
        if not v <= 1.0:
            bad.append(f"dots[{k}] = {float(dots[k])!r}: err/tol {v:.3g} beyond the bound (m = {len(y)})")
    if not float(dots[1]) >= 0.0:
        bad.append(f"dots[1] = {float(dots[1])!r} is negative")
    if wv is None and int(bits([dots[0]])[0]) != POS_ZERO_BITS:
        bad.append(f"dots[0] = {float(dots[0])!r} without a w: not the bits of +0.0")
    return bad


def assert_dots(dots, y, wv, what):
    """failures() is empty; returns the larger err / tol (a measurement)."""
    bad = failures(dots, y, wv)
    assert not bad, f"{what}: " + "; ".join(bad)
    return max(ratios(dots, y, wv))


# ---------------------------------------------------------------- structures
def pattern(name):
    """(m, n, rp, col) of a signed_inputs structure or a multi_inputs tridiagonal."""
    if name in mi.TRIDIAGS:
        c = mi.case(name, "cancel")
        return c["m"], c["n"], c["rp"], c["col"]
    return si.structure(name)


def case(name, family):
    """multi_inputs.case: signed_inputs' structures and the tridiagonals."""
    return mi.case(name, family)


@functools.lru_cache(maxsize=None)
def int_case(name):
    """The integer family on one structure: val, x in 1..9, w in 1..3, y and
    the two dots as exact integers (y as float64, the dots as Python ints).
    sum |t| and sum q stay below 2^53 -- asserted -- so every add order of
    every path is exact."""
    m, n, rp, col = pattern(name)
    rng = np.random.default_rng(500 + sum(map(ord, name)))
    nnz = int(rp[-1])
    val = rng.integers(1, 10, nnz).astype(np.float64)
    x = rng.integers(1, 10, n).astype(np.float64)
    wv = rng.integers(1, 4, m).astype(np.float64)
    prod = val.astype(np.int64) * x.astype(np.int64)[np.asarray(col, np.int64)]
    yi = si._segment_sums(prod, np.asarray(rp, np.int64))
    wy = sum(int(a) * int(b) for a, b in zip(wv.astype(np.int64).tolist(), yi.tolist()))
    yy = sum(int(b) * int(b) for b in yi.tolist())
    assert 0 <= wy < 2 ** 53 and 0 <= yy < 2 ** 53 and int(yi.max(initial=0)) < 2 ** 53
    y = yi.astype(np.float64)
    for a in (val, x, wv, y):
        a.setflags(write=False)
    return {"name": name, "family": "integer", "m": m, "n": n, "rp": rp, "col": col, "val": val, "x": x, "w": wv,
            "y": y, "wy": wy, "yy": yy}
