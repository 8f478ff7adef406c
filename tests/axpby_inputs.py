"""Inputs, the reference and the bound for Plan.execute_axpby
(y = alpha * A x + beta * y).

The reference is what the header promises, evaluated by numpy: two rounded
multiplies and one rounded add per row, as separate ufuncs (numpy never fuses
them),

    expected(s, y0, alpha, beta) = float64(alpha) * s + float64(beta) * y0,

and float64(alpha) * s alone when beta == 0 (either sign: y0 is not read).
With s = the plan's own spmv_execute result this is a bit-for-bit reference
for every plan whose row sums are reproducible (all but COO's split rows).

The bound every plan must meet whatever its own execute gives, against the
extended-precision row sums y_hi of signed_inputs.ref_rows:

    |y - (alpha y_hi + beta y0)| <= |alpha| row_tol + 3 * 2^-53 * (|alpha| mag + |beta y0|)

Derivation: s errs by at most row_tol = (len + 8) 2^-53 mag (signed_inputs),
and |s| <= mag (1 + len 2^-53).  p = fl(alpha s) errs by 2^-53 |alpha s|,
q = fl(beta y0) by 2^-53 |beta y0|, fl(p + q) by 2^-53 |p + q| <=
2^-53 (|alpha s| + |beta y0|) (1 + 2^-53): together below
2 * 2^-53 (1 + 2^-52) (|alpha| mag (1 + len 2^-53) + |beta y0|), which
3 * 2^-53 (|alpha| mag + |beta y0|) covers for rows of up to 2^51 entries.
The extended-precision evaluation of alpha y_hi + beta y0 itself errs by a few
2^-64 of the same magnitudes, inside that slack.  It is the only bound COO is
held to.

Plain helper module (numpy only, besides signed_inputs);
tests/test_axpby_inputs.py checks it on the CPU, tests/test_gpu_axpby.py uses
it on the GPU.
"""
import functools

import numpy as np

import signed_inputs as si

# (alpha, beta): the BLAS defaults, a residual, generic scalars, a small beta,
# alpha = 0 (no shortcut: 0 * s is computed) and beta = -0.0 (y0 never read)
ALPHA_BETA = ((1.0, 1.0), (1.0, -1.0), (-2.5, 0.75), (0.3, 1e-3), (0.0, 2.0), (2.0, -0.0))


def bits(a):
    """The int64 patterns of a float64 array (NaN payloads and signed zeros count)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def y0(m, seed=0):
    """A seeded signed y of mixed magnitude: +-U(0.5, 1) 10^k, k in [-4, 4];
    never zero.  Shared and read-only: copy it before handing it to an execute."""
    rng = np.random.default_rng(7000 + seed)
    y = rng.choice([-1.0, 1.0], m) * rng.uniform(0.5, 1.0, m) * 10.0 ** rng.integers(-4, 5, m)
    y.setflags(write=False)
    return y


def expected(s, y0, alpha, beta):
    """float64(alpha) * s + float64(beta) * y0 as two multiplies and an add,
    each a numpy ufunc of its own (no FMA); beta == 0: float64(alpha) * s, y0
    unread."""
    s = np.asarray(s, np.float64)
    p = np.multiply(np.float64(alpha), s)
    if beta == 0:
        return p
    q = np.multiply(np.float64(beta), np.asarray(y0, np.float64))
    return np.add(p, q)


REFRESH_STRUCTURES = ("staircase", "powerlaw", "uniform16", "banded")


@functools.lru_cache(maxsize=None)
def refresh_cases(name):
    """(A, B): one structure and one x with two value sets, for a plan built
    from A and refreshed to B (tests/test_gpu_update_values.py).  B is
    signed_inputs.case(name, "cancel"); A carries the `spread` family's
    values on B's x, with its own reference and sequential sums."""
    import oracle
    b = si.case(name, "cancel")
    val = si.case(name, "spread")["val"]
    ref = si.ref_rows(b["rp"], b["col"], val, b["x"])
    yo = oracle.csr_spmv(b["rp"], b["col"], np.ascontiguousarray(val), np.ascontiguousarray(b["x"]))
    for a in (yo,) + ref:
        a.setflags(write=False)
    return dict(b, family="spread", val=val, ref=ref, y_oracle=yo), b


def bound(rp, ref, y0, alpha, beta):
    """(want, tol) in extended precision: alpha y_hi + beta y0 and
    |alpha| row_tol + 3 * 2^-53 (|alpha| mag + |beta y0|) per row (module
    docstring).  ref = signed_inputs.ref_rows(...)."""
    y_hi, mag = ref
    a, b = np.longdouble(alpha), np.longdouble(beta)
    by0 = b * np.asarray(y0, np.float64).astype(np.longdouble) if beta != 0 else np.zeros(len(y_hi), np.longdouble)
    want = a * y_hi + by0
    tol = abs(a) * si.row_tol(rp, mag) + 3 * np.longdouble(si.U) * (abs(a) * mag + np.abs(by0))
    return want, tol


def failing_rows(y, rp, ref, y0, alpha, beta):
    """(rows beyond the bound or non-finite, err / tol per row).  A row with
    tol == 0 passes only with err == 0."""
    want, tol = bound(rp, ref, y0, alpha, beta)
    err = np.abs(np.asarray(y, np.float64).astype(np.longdouble) - want)
    ok = err <= tol  # False for NaN
    ratio = np.full(len(err), np.inf)
    pos = tol > 0
    ratio[pos] = (err[pos] / tol[pos]).astype(np.float64)
    ratio[~pos & ok] = 0.0
    ratio[np.isnan(ratio)] = np.inf
    return np.flatnonzero(~ok), ratio


def assert_bound(y, rp, ref, y0, alpha, beta, what):
    """Every row within the bound; reports the worst row.  Returns the
    largest err / tol (a measurement)."""
    bad, ratio = failing_rows(y, rp, ref, y0, alpha, beta)
    if len(bad):
        w = int(bad[np.argmax(ratio[bad])])
        want, _ = bound(rp, ref, y0, alpha, beta)
        raise AssertionError(f"{what} alpha={alpha} beta={beta}: {len(bad)} rows beyond the axpby bound, first "
                             f"{bad[:5].tolist()}; worst row {w}: y {y[w]!r} vs {float(want[w])!r}, "
                             f"err/tol {ratio[w]:.3g}")
    return float(ratio.max()) if len(ratio) else 0.0
