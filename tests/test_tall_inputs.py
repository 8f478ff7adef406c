"""CPU checks of tests/tall_inputs.py: the row map holds the rows it promises
at every size, the spread CSR is the compact one scattered through it, the
reference alone passes check_y on every structure, and check_y rejects a y
whose stores wrapped; the y0 formula of the axpby step is what its comment
says, the reference alone passes check_axpby_y and a y0 loaded or a y stored
rows away does not -- what keeps tests/test_gpu_tall_y.py honest.
"""
import numpy as np
import pytest

import oracle
import signed_inputs as si
import special_values as sv
import tall_inputs as ti
from multi_inputs import SENTINEL

ALL = ti.STRUCTURES + (ti.BAND,)
ALL_MS = ti.MS + ti.MULTI_MS + (ti.CPU_M,)
FILLS = [pytest.param(float("nan"), id="nan"), pytest.param(SENTINEL, id="sentinel")]


def test_sizes():
    T = ti.TALL
    assert T == 1 << 29 and ti.MS == (T - 1, T + 4099, 2 * T + 4099, 4 * T - 2)
    assert (T - 2) * 8 == (1 << 32) - 16  # the last row of the control: its byte offset still fits 32 bits
    assert ti.MS[-1] == (1 << 31) - 2 and ti.MS[1] % 2 == 1
    assert ti.MS[2] * 4 > 1 << 32 > ti.MS[1] * 4  # the 4-byte per-row arrays
    assert [m * 8 for m in ti.MULTI_MS] == [T - 8, T + 8 * 4099]  # m * ldy around 2^29 at ldy = 8
    assert ti.CPU_M == 1 << 20 and ti.M == 4003 and ti.N == 8192


@pytest.mark.parametrize("m", ALL_MS)
def test_rowmap_holds_the_promised_rows(m):
    """Index arithmetic only: nothing of size m is allocated."""
    T = ti.TALL
    rows = ti.rowmap(m)
    assert rows.dtype == np.int64 and len(rows) == ti.M and (np.diff(rows) > 0).all()
    assert rows[0] == 0 and rows[-1] == m - 1
    inside = np.zeros(len(rows), bool)
    for lo, hi in ti.clusters(m):
        assert hi - lo in (wi_cluster(), 2 * wi_cluster())
        inside |= (rows >= lo) & (rows < hi)
        assert ((rows >= lo) & (rows < hi)).sum() >= 500, (lo, hi)  # every cluster, in many rows
    assert inside[~np.isin(rows, ti.promised_rows(m))].all()
    for p in (29, 30):
        assert np.isin([(1 << p) - 1, 1 << p], rows).all() == (m > 1 << p), p
    if m in ti.MS:
        assert len(ti.clusters(m)) == {T - 1: 3, T + 4099: 3, 2 * T + 4099: 4, 4 * T - 2: 5}[m]
        assert (rows >= 1 << 28).any()
        assert (rows >= T).any() == (m > T) and (rows >= 2 * T).any() == (m > 2 * T)
        if m > T:  # y offsets truly beyond 2^32, and rows the 32-bit offset wraps onto other rows
            assert (rows * 8 >= 1 << 32).sum() >= 1000
    if m in ti.MULTI_MS:
        assert (rows * 64 >= 1 << 32).any() == (m > ti.MULTI_TALL)
    assert ti.promised_rows(m) == sorted(set(ti.promised_rows(m))) and np.isin(ti.promised_rows(m), rows).all()


def wi_cluster():
    import wide_inputs as wi
    return wi.CLUSTER


@pytest.mark.parametrize("m", ALL_MS)
@pytest.mark.parametrize("name", ALL)
def test_structure(name, m):
    c = ti.case(name, m)
    rp, col, lens = c["rp"], c["col64"], np.diff(c["rp"])
    assert len(rp) == ti.M + 1 and c["m"] == m and c["n"] == (m if name == ti.BAND else ti.N)
    assert 0.05 <= (lens == 0).mean() <= 0.13  # about every 11th row
    at = np.searchsorted(c["rowmap"], ti.promised_rows(m))
    assert (lens[at] > 0).all()  # rows 0, m - 1 and the pairs carry entries
    assert col.min() >= 0 and col.max() < c["n"] and np.array_equal(c["col"], col)
    assert (np.diff(c["ucol"]) > 0).all() and np.array_equal(c["ucol"][c["ccol"]], col)
    inner = np.ones(len(col), bool)
    inner[rp[:-1][lens > 0]] = False
    d = np.diff(col)[inner[1:]]
    if name == "tall_uniform":
        assert set(lens.tolist()) == {0, 16} and (d > 0).all()
    elif name == "tall_long":
        assert (d >= 0).all() and (d == 0).any()
        assert {4096, 4097, 9000, 700, 128, 129} <= set(lens.tolist())
        assert all(lens[r] == k for r, k in ti.LONG_ROWS.items())
    else:
        row = np.repeat(c["rowmap"], lens)
        assert sorted(set((col - row).tolist())) == [-1, 0, 1] and (d > 0).all()
        assert lens[0] == 2 and lens[-1] == 2 and set(lens[1:-1].tolist()) == {0, 3}  # clamped out at the two ends
        assert 10_000 <= int(rp[-1]) <= 12_100
    assert np.isfinite(c["x_c"]).all() and np.isfinite(c["val"]).all() and np.isfinite(c["y_oracle"]).all()
    si.assert_rows(c["y_oracle"], rp, c["ccol"], c["val"], c["x_c"], f"oracle {name} {m}", ref=c["ref"])
    for j in (1, 2):
        cj = ti.column(name, m, j)
        si.assert_rows(cj["y_oracle"], rp, c["ccol"], c["val"], cj["x_c"], f"oracle {name} {m} column {j}", ref=cj["ref"])
        assert not np.array_equal(cj["y_oracle"], c["y_oracle"])


# ---------------------------------------------------------------- CPU_M: a full host y
def _full(name):
    """The tall CSR at CPU_M as numpy arrays, x, and the oracle's y on all m rows."""
    c = ti.case(name, ti.CPU_M)
    rp, col, val = (t.numpy() for t in ti.device_csr(c, ti.CPU_M, "cpu"))
    x = ti.device_x(c, "cpu").numpy()
    return c, rp, col, val, x, oracle.csr_spmv(rp, col, val, x)


@pytest.mark.parametrize("name", ALL)
def test_spread_csr_is_the_compact_one_scattered(name):
    c, rp, col, val, x, y = _full(name)
    m = ti.CPU_M
    assert rp.dtype == np.int64 and len(rp) == m + 1 and rp[0] == 0 and rp[-1] == len(val) == c["rp"][-1]
    lens = np.zeros(m, np.int64)
    lens[c["rowmap"]] = np.diff(c["rp"])
    assert np.array_equal(np.diff(rp), lens)
    assert len(x) == c["n"] and np.isfinite(x).all()
    want = np.zeros(m)
    want[c["rowmap"]] = c["y_oracle"]
    assert np.array_equal(sv.bits(y), sv.bits(want))


def test_cumsum_chunks(monkeypatch):
    """device_csr's chunked in-place cumsum, with chunks far smaller than m."""
    c = ti.case("tall_long", ti.CPU_M)
    whole = ti.device_csr(c, ti.CPU_M, "cpu")[0].numpy()
    monkeypatch.setattr(ti, "CUMSUM_CHUNK", 4099)
    assert np.array_equal(ti.device_csr(c, ti.CPU_M, "cpu")[0].numpy(), whole)


class _Info(dict):
    """A stand-in for Plan.info() of a sequential plan."""

    def __init__(self):
        super().__init__(format="ell", csr_lanes=0, overflow_nnz=0, css_split_rows=0, bin_long_len=0)


def _y(c, fill, col=None):
    """The reference's own y on all m rows of a tensor that held `fill`."""
    import torch
    y = torch.full((c["m"],), fill, dtype=torch.float64)
    y.zero_()
    y[torch.from_numpy(np.array(c["rowmap"]))] = torch.from_numpy(np.array((c if col is None else col)["y_oracle"]))
    return y


@pytest.mark.parametrize("name", ALL)
def test_reference_passes_check_y(name):
    """Nothing is left out by construction: the reference alone passes, as a
    sequential plan, run to run, and column by column of a strided block."""
    import torch
    c = ti.case(name, ti.CPU_M)
    assert ti.check_y(_y(c, SENTINEL), c, name) <= 1.0
    y = _y(c, float("nan"))
    prev = ti.live(y, c)
    assert np.array_equal(sv.bits(prev), sv.bits(c["y_oracle"]))
    ti.check_y(y, c, name, info=_Info(), prev=prev)
    assert int(torch.count_nonzero(y)) == 0  # the live rows were zeroed in place
    Y = torch.full((c["m"], 8), SENTINEL, dtype=torch.float64)
    for j in range(3):
        Y[:, j] = _y(c, SENTINEL, ti.column(name, c["m"], j))
    for j in range(3):
        ti.check_y(Y[:, j], c, f"{name} column {j}", info=_Info(), col=ti.column(name, c["m"], j))
    assert (sv.bits(Y[:, 3:].numpy()) == sv.bits(np.array([SENTINEL]))[0]).all()


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ALL)
def test_check_y_rejects_planted_errors(name, fill):
    """One live value moved to row r - 2^k (what a wrapped byte offset does),
    one live row left at its fill, a -0.0 on an empty row."""
    import torch
    c = ti.case(name, ti.CPU_M)
    lens = np.diff(c["rp"])
    i = int(np.flatnonzero(c["y_oracle"] != 0)[-1])  # the last live row with a non-zero sum: in the end cluster
    r = int(c["rowmap"][i])
    for k in (17, 19):
        assert r - (1 << k) > 0 and r - (1 << k) not in c["rowmap"]
        y = _y(c, fill)
        y[r - (1 << k)] = y[r]
        y[r] = fill
        with pytest.raises(AssertionError, match="not finite|beyond row_tol"):
            ti.check_y(y, c, name)
        y = _y(c, fill)  # the stray store alone
        y[r - (1 << k)] = y[r]
        with pytest.raises(AssertionError, match="off the live ones"):
            ti.check_y(y, c, name)
    y = _y(c, fill)
    y[r] = fill
    with pytest.raises(AssertionError, match="not finite|beyond row_tol"):
        ti.check_y(y, c, name)
    for row in (1 if 1 not in c["rowmap"] else 3000, c["m"] // 2):
        assert row not in c["rowmap"]
        y = _y(c, fill)
        y[row] = -0.0
        with pytest.raises(AssertionError, match="off the live ones"):
            ti.check_y(y, c, name)
    e = int(np.flatnonzero(lens == 0)[0])  # and on a live row without entries
    y = _y(c, fill)
    y[int(c["rowmap"][e])] = -0.0
    with pytest.raises(AssertionError, match="empty live row"):
        ti.check_y(y, c, name)
    # a sequential plan one ulp off the oracle, and a y that changes run to run
    y = _y(c, fill)
    y[r] = float(np.nextafter(c["y_oracle"][i], np.inf))
    prev = ti.live(_y(c, fill), c)
    with pytest.raises(AssertionError, match="bit-exact"):
        ti.check_y(y.clone(), c, name, info=_Info())
    with pytest.raises(AssertionError, match="held before"):
        ti.check_y(y.clone(), c, name, prev=prev)
    ti.check_y(y, c, name)  # within row_tol all the same


# ---------------------------------------------------------------- y = alpha A x + beta y
def test_y0_formula():
    """Never zero, at most 13 significant bits (beta * y0 exact), another value 2^29, 2^30 and 2^31 rows away,
    and the device evaluation chunk by chunk is the numpy one bit for bit."""
    import torch
    T = ti.TALL
    assert [(1 << p) % ti.Y0_PERIOD for p in (29, 30, 31)] == [8, 16, 32]
    rows = np.concatenate([np.arange(0, 3 * ti.Y0_PERIOD), ti.rowmap(4 * T - 2), [4 * T - 3]])
    y0 = ti.y0_rows(rows)
    P = ti.Y0_PERIOD
    assert y0[0] == 1 / 8192 and y0[1] == -2 / 8192 and y0[P - 1] == 8191 / 8192 and y0[P] == -1 / 8192
    assert (y0 != 0).all() and (np.abs(y0) < 1).all() and (np.sign(y0) == np.where(rows % 2 == 0, 1, -1)).all()
    assert np.array_equal(y0 * 8192, np.rint(y0 * 8192))  # k / 8192 with k <= 8191: 13 bits
    beta = ti.AXPBY[1]
    exact = (beta * y0).astype(np.longdouble) == np.longdouble(beta) * y0.astype(np.longdouble)
    assert exact.all()
    for p in (29, 30, 31):
        far = rows[rows + (1 << p) < 1 << 32]
        assert (ti.y0_rows(far + (1 << p)) != ti.y0_rows(far)).all(), p
    for a, b in ((0, 20000), (T - 5, T + 9000), (4 * T - 9000, 4 * T - 2)):
        r = np.arange(a, b)
        assert np.array_equal(sv.bits(ti._y0_chunk(a, b, "cpu").numpy()), sv.bits(ti.y0_rows(r)))
        assert np.array_equal(sv.bits(ti._y0_chunk(a, b, "cpu", beta).numpy()), sv.bits(beta * ti.y0_rows(r)))
    y = torch.empty(ti.CPU_M, dtype=torch.float64)
    ti.fill_y0(y)
    assert np.array_equal(sv.bits(y.numpy()), sv.bits(ti.y0_rows(np.arange(ti.CPU_M))))


def _axpby_y(c, s=None, shift=0):
    """The reference's own y after y = alpha A x + beta y0 on all m rows: expected(s, y0, ...) on the live rows
    (s: the oracle's sums), beta * y0 elsewhere."""
    import torch
    import axpby_inputs as ai
    s = c["y_oracle"] if s is None else s
    y = torch.empty(c["m"], dtype=torch.float64)
    ti.fill_y0(y, shift)
    y.mul_(ti.AXPBY[1])
    live = ai.expected(s, ti.y0_rows(c["rowmap"] + shift), *ti.AXPBY)
    y[torch.from_numpy(np.array(c["rowmap"]))] = torch.from_numpy(live)
    return y


def _nudged(c, s, rows):
    """s with a quarter of row_tol added on `rows`: inside the axpby bound, and far above the last bit of
    alpha * s + beta * y0 (the cancel family's sums are rounding noise, one ulp of s would vanish in the add)."""
    s2 = np.array(s)
    s2[rows] += 0.25 * np.asarray(si.row_tol(c["rp"], c["ref"][1]), np.float64)[rows]
    return s2


class _Coo(_Info):
    def __init__(self):
        super().__init__()
        self["format"] = "coo"


@pytest.mark.parametrize("name", ALL)
def test_reference_passes_check_axpby_y(name, monkeypatch):
    c = ti.case(name, ti.CPU_M)
    s = c["y_oracle"]
    assert ti.check_axpby_y(_axpby_y(c), c, s, *ti.AXPBY, name, _Info()) <= 1.0
    monkeypatch.setattr(ti, "CUMSUM_CHUNK", 4099)  # chunks far smaller than m
    y = _axpby_y(c)
    assert ti.check_axpby_y(y, c, s, *ti.AXPBY, name, _Info()) <= 1.0
    want = ti.AXPBY[1] * ti.y0_rows(np.arange(c["m"]))
    assert np.array_equal(sv.bits(y.numpy()), sv.bits(want))  # the live rows were overwritten in place
    # COO: a row split across units may differ from expected(execute) inside the bound; a row of one unit may not
    rp = c["rp"]
    split = np.flatnonzero(rp[:-1] // 128 != (rp[1:] - 1) // 128)
    inside = np.flatnonzero((rp[:-1] // 128 == (rp[1:] - 1) // 128) & (np.diff(rp) > 0) & (s != 0))
    for rows, info, ok in ((split[:1], _Coo(), True), (split[:1], _Info(), False), (inside[:1], _Coo(), False)):
        if not len(rows):
            assert name == "tall_uniform"  # rows of 16 entries never straddle a unit
            continue
        s2 = _nudged(c, s, rows)
        if ok:
            ti.check_axpby_y(_axpby_y(c), c, s2, *ti.AXPBY, name, info)
        else:
            with pytest.raises(AssertionError, match=r"expected\(execute\)"):
                ti.check_axpby_y(_axpby_y(c), c, s2, *ti.AXPBY, name, info)


@pytest.mark.parametrize("name", ALL)
def test_check_axpby_y_rejects_planted_errors(name):
    """One off-live row keeps y0, one live row takes the value of the row 8 below it (a y0 load or a store 2^29
    rows away at the period's remainder), one off-live row is +0.0 (execute's store, not axpby's), y0 shifted by
    one row; and a sequential plan off the oracle's sum, a live row not finite."""
    c = ti.case(name, ti.CPU_M)
    s = c["y_oracle"]
    lens = np.diff(c["rp"])
    rowmap = c["rowmap"]

    def check(y, info=None, first=s):
        return ti.check_axpby_y(y, c, first, *ti.AXPBY, name, info or _Info())

    for row in (1 if 1 not in rowmap else 3000, c["m"] // 2, c["m"] - 5000):
        assert row not in rowmap
        y = _axpby_y(c)
        y[row] = float(ti.y0_rows([row])[0])
        with pytest.raises(AssertionError, match=rf"1 rows off the live ones are not beta \* y0, first \[{row}\]"):
            check(y)
        y = _axpby_y(c)
        y[row] = 0.0
        with pytest.raises(AssertionError, match=r"off the live ones are not beta \* y0"):
            check(y)
    live = np.flatnonzero((lens > 0) & (rowmap >= 8))
    cut = live[c["rp"][live] // 128 != (c["rp"][live + 1] - 1) // 128]
    assert len(cut) or name == "tall_uniform"  # tall_uniform's rows of 16 entries never straddle a unit
    for i in [int(live[0]), int(live[-1])] + cut[:1].tolist():
        r = int(rowmap[i])
        y = _axpby_y(c)
        y[r] = y[r - 8].clone()
        with pytest.raises(AssertionError, match=r"expected\(execute\)"):
            check(y)
        split = c["rp"][i] // 128 != (c["rp"][i + 1] - 1) // 128  # COO: the bound alone judges a row split across units
        with pytest.raises(AssertionError, match="beyond the axpby bound" if split else r"expected\(execute\)"):
            check(y, _Coo())
        y = _axpby_y(c)  # the right sum on the y0 of the row 8 below
        y[r] = float(ti.AXPBY[0] * s[i] + ti.AXPBY[1] * ti.y0_rows([r - 8])[0])
        with pytest.raises(AssertionError, match=r"expected\(execute\)"):
            check(y)
    with pytest.raises(AssertionError, match=r"expected\(execute\)|off the live ones"):
        check(_axpby_y(c, shift=1))
    y = _axpby_y(c, shift=1)  # the live rows right, y0 shifted everywhere else
    import torch
    idx = torch.from_numpy(np.array(rowmap))
    y[idx] = _axpby_y(c)[idx]
    with pytest.raises(AssertionError, match=r"off the live ones are not beta \* y0"):
        check(y)
    i = int(live[-1])
    s2 = _nudged(c, s, [i])
    with pytest.raises(AssertionError, match=r"expected\(sequential sum\)"):
        check(_axpby_y(c, s2), first=s2)
    info = _Info()
    info["format"], info["css_split_rows"] = "css", 1  # not sequential: the plan's own sums are the reference
    check(_axpby_y(c, s2), info, first=s2)
    y = _axpby_y(c)
    y[int(rowmap[i])] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        check(y)
