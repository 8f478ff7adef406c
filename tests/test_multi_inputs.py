"""tests/multi_inputs.py on the CPU: the k-column X and its buffers, the
per-column references, the greedy width cut and the Python block checks of
Plan.execute_multi.  No GPU needed."""
import numpy as np
import pytest

import multi_inputs as mi
import oracle
import signed_inputs as si
import singlespmv_amd as sp


def test_greedy_cut_for_every_k():
    """k = 1..32: widths from {8, 4, 2, 1} summing to k, non-increasing, at
    most one block each of 4, 2 and 1, and every block of width >= 2 starts
    at an even column."""
    for k in range(1, mi.MULTI_MAX + 1):
        w = mi.greedy_cut(k)
        assert sum(w) == k and set(w) <= {8, 4, 2, 1}
        assert w == sorted(w, reverse=True)
        assert w.count(8) == k // 8 and all(w.count(c) <= 1 for c in (4, 2, 1))
        starts = np.concatenate([[0], np.cumsum(w)[:-1]])
        assert all(s % 2 == 0 for s, c in zip(starts, w) if c >= 2)
        assert mi.expected_path(k, True) == w and mi.expected_path(k, False) == [1] * k
    assert mi.greedy_cut(13) == [8, 4, 1] and mi.greedy_cut(7) == [4, 2, 1] and mi.greedy_cut(32) == [8] * 4


@pytest.mark.parametrize("name,family", [("rect7x1000", "cancel"), ("rect513x40", "spread"), ("tri1500", "cancel")])
def test_columns_and_references(name, family):
    c = mi.case(name, family)
    k = 5
    buf, X = mi.x_block(name, family, k, ldx=8)
    assert X.shape == (c["n"], k) and X.base is buf and X.strides == (64, 8)
    assert np.isnan(buf[:, k:]).all() and np.isfinite(X).all()
    assert np.array_equal(X[:, 0], c["x"])  # column 0: the family's own x
    for j in range(1, k):
        x = X[:, j]
        assert ((np.abs(x) >= 0.5) & (np.abs(x) <= 2.0)).all()
        assert not np.array_equal(x, X[:, j - 1])
        col = mi.column(name, family, j)
        assert col is mi.column(name, family, j)  # computed once
        yo = oracle.csr_spmv(c["rp"], c["col"], np.ascontiguousarray(c["val"]), np.ascontiguousarray(x))
        assert np.array_equal(col["y_oracle"], yo)
        y_hi, mag = si.ref_rows(c["rp"], c["col"], c["val"], np.ascontiguousarray(x))
        assert np.array_equal(col["ref"][0], y_hi) and np.array_equal(col["ref"][1], mag)
        # the sequential sum passes the derived bound; a column swapped for its neighbour does not
        si.assert_rows(yo, c["rp"], c["col"], c["val"], x, f"{name} column {j}", ref=col["ref"])
        if c["rp"][-1]:
            with pytest.raises(AssertionError):
                si.assert_rows(mi.column(name, family, j - 1)["y_oracle"], c["rp"], c["col"], c["val"], x, "swapped",
                               ref=col["ref"])


def test_cancel_rows_cancel_in_column_zero_only():
    c = mi.case("tri1500", "cancel")
    even = np.diff(c["rp"]) == 2
    assert even.any()
    y0, mag0 = mi.column("tri1500", "cancel", 0)["ref"]
    y1, mag1 = mi.column("tri1500", "cancel", 1)["ref"]
    assert (np.abs(y0[even]) < 1e-14 * mag0[even]).all()
    assert (np.abs(y1[even]) > 1e-3 * mag1[even]).mean() > 0.9


def test_tridiagonal_windows():
    """The x window of a 512-row DIA workgroup is 512 + span + 1 doubles."""
    for name, doubles in (("tri1500", 3513), ("tri5000", 10513)):
        m, n, offs = mi.TRIDIAGS[name]
        c = mi.case(name, "cancel")
        row = np.repeat(np.arange(m), np.diff(c["rp"]))
        assert sorted(set((c["col"] - row).tolist())) == sorted(offs)
        assert 512 + max(offs) - min(offs) + 1 == doubles
    lds = 160 * 1024
    assert 3513 * 2 * 8 <= lds < 3513 * 8 * 8 and 10513 * 2 * 8 > lds


def test_y_block_and_pads():
    buf, Y = mi.y_block(7, 3, 5)
    assert Y.shape == (7, 3) and Y.base is buf and mi.pads_untouched(buf, 3)
    Y[:] = 0.0
    assert mi.pads_untouched(buf, 3)
    buf[4, 3] = -1.2345e300 * (1 + 2.0 ** -52)  # one ulp off the sentinel
    assert not mi.pads_untouched(buf, 3)
    buf, Y = mi.y_block(7, 3, 5, fill=np.nan)
    assert mi.pads_untouched(buf, 3, fill=np.nan)
    buf[0, 4] = 0.0
    assert not mi.pads_untouched(buf, 3, fill=np.nan)
    assert [mi.ld_for(k) for k in (1, 2, 3, 8, 13)] == [2, 4, 4, 10, 14]


def test_block_checks():
    """Plan.execute_multi's argument checks (sp._check_block): shape, dtype,
    strides, writability and k, before any address reaches the C-ABI."""
    chk = sp._check_block
    wide = np.zeros((10, 6))
    assert chk(wide, 10, "X", 0, False) == (6, 6)
    assert chk(wide[:, :3], 10, "X", 0, False) == (3, 6)  # a view of a wider array
    assert chk(wide[:, 1:2], 10, "X", 0, False) == (1, 6)
    assert chk(np.zeros((10, 1)), 10, "X", 0, False) == (1, 1)
    assert chk(np.zeros((1, 4)), 1, "X", 0, False) == (4, 4)
    assert chk(np.zeros((0, 5))[:, :3], 0, "Y", 0, True) == (3, 3)  # no element: any strides
    with pytest.raises(ValueError, match="2-D"):
        chk(np.zeros(10), 10, "X", 0, False)
    with pytest.raises(ValueError, match="rows"):
        chk(wide, 11, "X", 0, False)
    with pytest.raises(ValueError, match="float64"):
        chk(np.zeros((10, 2), np.float32), 10, "X", 0, False)
    with pytest.raises(ValueError, match="unit stride"):
        chk(np.zeros((6, 10)).T, 10, "X", 0, False)
    with pytest.raises(ValueError, match="unit stride"):
        chk(wide[:, ::2], 10, "X", 0, False)
    with pytest.raises(ValueError, match="row stride"):
        chk(wide[::-1, :3], 10, "X", 0, False)
    with pytest.raises(ValueError, match="columns"):
        chk(np.zeros((10, 33)), 10, "X", 0, False)
    with pytest.raises(ValueError, match="columns"):
        chk(np.zeros((10, 0)), 10, "X", 0, False)
    ro = np.zeros((10, 2))
    ro.setflags(write=False)
    chk(ro, 10, "X", 0, False)
    with pytest.raises(ValueError, match="read-only"):
        chk(ro, 10, "Y", 0, True)
    with pytest.raises(ValueError, match="numpy array or torch tensor"):
        chk([[1.0]], 1, "X", 0, False)
    import torch
    with pytest.raises(ValueError, match="numpy array"):
        chk(torch.zeros((10, 2), dtype=torch.float64), 10, "X", 0, False)
