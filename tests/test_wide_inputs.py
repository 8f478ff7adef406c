"""CPU checks of tests/wide_inputs.py: the structures reach the columns they
are there for, the compact reference is the full one, every layout's reach
lies on written entries of the NaN-filled x, and the checks reject a kernel
whose x offsets wrap at 32 bits -- what keeps tests/test_gpu_wide_x.py honest.
"""
import numpy as np
import pytest

import oracle
import signed_inputs as si
import special_values as sv
import wide_inputs as wi

ALL = wi.STRUCTURES + (wi.UNSORTED,)
ALL_NS = wi.NS + wi.MULTI_NS + (wi.CPU_N,)
CASES = [pytest.param(name, n, id=f"{name}-{n}") for n in ALL_NS for name in ALL]


def test_sizes():
    W = wi.WIDE
    assert W == 1 << 29 and wi.NS == (W - 1, W, W + 4099, 2 * W + 4099, 4 * W - 2)
    assert (W - 2) * 8 == (1 << 32) - 16  # the last column of the last 32-bit case
    assert wi.NS[-1] == (1 << 31) - 2 and wi.NS[2] % 2 == 1
    assert [n * 8 for n in wi.MULTI_NS] == [W - 8, W, W + 8 * 4099]  # n * ldx around the fused switch at ldx = 8


@pytest.mark.parametrize("name,n", CASES)
def test_structure_and_remap(name, n):
    c = wi.case(name, n)
    m, rp, col, ucol, ccol = c["m"], c["rp"], c["col64"], c["ucol"], c["ccol"]
    lens = np.diff(rp)
    assert m == wi.M and 3500 <= m <= 4500 and int(rp[-1]) <= 160_000
    assert 0.05 <= (lens == 0).mean() <= 0.13  # about every 11th row
    assert col.min() >= 0 and col.max() < n and np.array_equal(c["col"], col)
    # the remap is monotone: strictly increasing on ucol, so every comparison
    # of two columns of a row survives it (order and duplicates alike)
    assert (np.diff(ucol) > 0).all() and np.array_equal(ucol[ccol], col)
    inner = np.ones(len(col), bool)
    inner[rp[:-1][lens > 0]] = False  # entry j and j - 1 share a row
    d, dc = np.diff(col)[inner[1:]], np.diff(ccol.astype(np.int64))[inner[1:]]
    assert np.array_equal(np.sign(d), np.sign(dc))
    if name == wi.UNSORTED:
        assert (d < 0).any() and (d == 0).any()  # out of order, with duplicates
        assert np.array_equal(np.sort(lens), np.sort(np.diff(wi.case("far_long", n)["rp"])))
    elif name == "far_long":
        assert (d >= 0).all()
    else:
        assert (d > 0).all()
    assert np.isfinite(c["x_c"]).all() and np.isfinite(c["val"]).all() and np.isfinite(c["y_oracle"]).all()
    si.assert_rows(c["y_oracle"], rp, ccol, c["val"], c["x_c"], f"oracle {name} {n}", ref=c["ref"])


@pytest.mark.parametrize("name", ALL)
def test_compact_reference_is_the_full_one(name):
    """n = 2^22: the oracle on a full NaN-filled host x, bit for bit."""
    c = wi.case(name, wi.CPU_N)
    x = np.full(c["n"], np.nan)
    x[c["ucol"]] = c["x_c"]
    y = oracle.csr_spmv(c["rp"], c["col"], c["val"], x)
    assert np.array_equal(sv.bits(y), sv.bits(c["y_oracle"]))
    assert np.array_equal(sv.bits(wi.gathered_spmv(c, lambda col: col)), sv.bits(c["y_oracle"]))
    for j in (1, 2):
        cj = wi.column(name, wi.CPU_N, j)
        x[c["ucol"]] = cj["x_c"]
        assert np.array_equal(sv.bits(oracle.csr_spmv(c["rp"], c["col"], c["val"], x)), sv.bits(cj["y_oracle"]))
        assert not np.array_equal(cj["y_oracle"], c["y_oracle"])


@pytest.mark.parametrize("name,n", CASES)
def test_every_reach_lies_on_written_entries(name, n):
    """Each layout's reach is inside ucol, and a CPU model of the layout on
    the NaN-filled x -- the row's own products plus 0 * x[c] for every other
    column of its reach -- is finite."""
    c = wi.case(name, n)
    m, rp, col = c["m"], c["rp"], c["col64"]
    at = wi.sparse_x(c["ucol"], c["x_c"])
    for fmt in ["csr", "ell"] + (["dia"] if name in wi.BANDED else []):
        rrp, rcol = sv.reach({"format": fmt}, rp, col, m, n)
        assert np.isin(rcol, c["ucol"]).all(), fmt
        pads = si._segment_sums(0.0 * at(rcol), rrp)
        assert np.isfinite(c["y_oracle"] + pads).all(), fmt
    if (np.diff(rp) == 0).any():
        assert c["ucol"][0] == 0  # the padded layouts' column of an empty row
    # and a read one column off the reach is not
    assert np.isnan(at(np.array([c["ucol"][-1] + 1, -1]))).all()


@pytest.mark.parametrize("name,n", [p for p in CASES if p.values[1] in wi.NS])
def test_clusters_hit(name, n):
    c = wi.case(name, n)
    col, m = c["col64"], c["m"]
    W = wi.WIDE
    if name in wi.BANDED:  # with_empty_rows empties the last five rows: the band ends at row m - 6
        assert col.max() == n - 6
        assert (col == 0).any() == (name == "two_bands")
    else:
        assert (col == n - 1).any() and (col == 0).any()
    # columns at and beyond 2^28 (c * 8 leaves int32), 2^29 (the byte offset
    # leaves 32 bits), 2^30 (2 * c leaves int32), where n allows
    assert (col >= 1 << 28).any()
    assert (col >= W).any() == (n > W)
    assert (col >= 2 * W).any() == (n > 2 * W)
    if n > W + wi.END:  # offsets truly beyond 2^32
        assert ((col >= W) & (col % W != col)).any() and (col * 8 >= 1 << 32).any()
    if name in ("far_uniform", "far_long", wi.UNSORTED):
        for lo, hi_ in wi.clusters(n):  # every cluster, in many rows
            assert ((col >= lo) & (col < hi_)).sum() >= 100, (lo, hi_)
        assert len(wi.clusters(n)) == {W - 1: 3, W: 3, W + 4099: 3, 2 * W + 4099: 4, 4 * W - 2: 5}[n]
    if name in wi.BANDED:
        row = np.repeat(np.arange(m), np.diff(c["rp"]))
        off = np.unique(col - row)
        assert len(off) == {"far_band": 17, "two_bands": 34}[name]
        assert off.max() == n - m and (off >= n - m - 16).sum() == 17 and off.min() == {"far_band": n - m - 16}.get(name, -8)
        # the DIA window (512 rows + span + 1): on the LDS path for far_band, far beyond it for two_bands
        assert (512 + off.max() - off.min() + 1 <= 8192) == (name == "far_band")
    if name == "far_uniform":
        assert (np.diff(c["rp"])[np.diff(c["rp"]) > 0] == 16).all()
        rows_first = np.add.reduceat(col < wi.CLUSTER, c["rp"][:-1][np.diff(c["rp"]) > 0])
        rows_last = np.add.reduceat(col >= n - wi.END, c["rp"][:-1][np.diff(c["rp"]) > 0])
        assert (rows_first >= 1).all() and (rows_last >= 1).all()


def csr_bin_of(length):
    """csr_bin_of of formats.cpp: L = the smallest power of two with 4 L >=
    len, capped at 64; a workgroup per row beyond 4096 entries."""
    if length > 4096:
        return 7
    b = 0
    while b < 6 and 4 * (1, 2, 4, 8, 16, 32, 64)[b] < length:
        b += 1
    return b


@pytest.mark.parametrize("n", wi.NS)
def test_far_long_covers_every_csr_bin(n):
    lens = np.diff(wi.case("far_long", n)["rp"])
    assert {csr_bin_of(int(v)) for v in lens[lens > 0]} == set(range(8))
    assert {4096, 4097, 9000, 700, 128, 129} <= set(lens.tolist())
    assert np.array_equal(lens, np.diff(wi.case(wi.UNSORTED, n)["rp"]))


@pytest.mark.parametrize("wrap", [wi.wrap32, wi.wrap28], ids=["wrap32", "wrap28"])
@pytest.mark.parametrize("name,n", [p for p in CASES if p.values[1] in wi.NS])
def test_checker_rejects_wrapped_offsets(name, n, wrap):
    """A simulated kernel reading x[(c * 8 mod 2^32) / 8], or x[c mod 2^28],
    over the sparse NaN-filled x: rejected by check_y at every n >= WIDE +
    4099 (mod 2^28: at every n here); at n <= WIDE the 32-bit offset is right
    and must pass."""
    c = wi.case(name, n)
    y = wi.gathered_spmv(c, wrap)
    wrong = n >= wi.WIDE + 4099 or wrap is wi.wrap28
    if n == wi.WIDE and wrap is wi.wrap32:
        assert c["col64"].max() * 8 < 1 << 32  # every offset still fits 32 bits
    if not wrong:
        wi.check_y(y, c, f"{name} {n}")
        assert np.array_equal(sv.bits(y), sv.bits(c["y_oracle"]))
        return
    with pytest.raises(AssertionError):
        wi.check_y(y, c, f"{name} {n}")
    # every row with a column the wrap moves is rejected -- poisoned, or far
    # beyond its bound -- and no other; that is most rows
    bad, _ = si.failing_rows(y, c["rp"], c["ref"])
    moved = sv.rows_touching(c["rp"], np.arange(len(c["col64"])), wrap(c["col64"]) != c["col64"])
    if name == wi.UNSORTED:  # a +t, -t pair on one repeated column cancels whatever x it reads
        assert not np.setdiff1d(bad, np.flatnonzero(moved)).size
    else:
        assert np.array_equal(bad, np.flatnonzero(moved))
    assert len(bad) >= 0.7 * int((np.diff(c["rp"]) > 0).sum())


@pytest.mark.parametrize("n", wi.MULTI_NS)
def test_checker_rejects_wrapped_multi_offsets(n):
    """The fused kernels' (uint32_t)c * (ldx * 8) at ldx = 8: wrong from n =
    2^26 + 4099 on."""
    for name in ("far_uniform", "far_band"):
        c = wi.case(name, n)
        y = wi.gathered_spmv(c, lambda col: ((col * 64) % (1 << 32)) // 64)
        if n <= wi.MULTI_WIDE:
            wi.check_y(y, c, name)
        else:
            with pytest.raises(AssertionError):
                wi.check_y(y, c, name)
