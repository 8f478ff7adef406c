"""Value refresh on a fixed pattern (Plan.prepare_update / Plan.update_values,
spmv_plan_update_prepare / spmv_plan_update_values): an updated plan is, array
by array (spmv_plan_digest), the plan a fresh build from the new values gives,
for every format and option set below, on the suite's seven structures; the
padding and sign rules, the refusals (wrong pattern, merged entries, not
prepared), alignment and tail cases, streams, graphs, multi executes (fused
and column by column), execute_axpby on a refreshed plan that already holds
its scratch, and the memory accounting of include/spmv_hip.h "value
refresh"."""
import numpy as np
import pytest

import axpby_inputs as ai
import signed_inputs as si
import singlespmv_amd as sp

pytestmark = pytest.mark.gpu

FORMATS = [
    ("csr", {}), ("csr", {"csr_lanes": 1}), ("csr", {"csr_lanes": 4}), ("csr", {"csr_lanes": 16}),
    ("csr", {"csr_row_ptr64": True}),
    ("ss", {"ss_sigma": 8}), ("ss", {"ss_sigma": 16}), ("ss", {"ss_sigma": 32}),
    ("ell", {}),
    ("hyb", {}), ("hyb", {"ell_width": 4}),
    ("jds", {}), ("jds", {"ell_width": 8}),
    ("dia", {}),
    ("coo", {}),
    ("css", {}), ("css", {"css_slab_shift": 12}),
    ("bin", {}), ("bin", {"bin_long_len": 40}), ("bin", {"bin_strip_cols": 3001}), ("bin", {"bin_product_order": 2}),
    ("auto", {}),
    ("csr", {"crs_exact": True}),
]
FORMAT_IDS = ["-".join([f] + [f"{k}{int(v)}" for k, v in kw.items()]) for f, kw in FORMATS]


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().tensor(np.asarray(a)).cuda()  # a copy: the shared fixtures are read-only


def _build(m, n, rp, col, val, fmt, kw, device):
    """A plan by the host builders from host arrays, or by from_device_csr
    from CUDA tensors; None where the builder refuses the combination."""
    try:
        if device:
            return sp.Plan.from_device_csr(m, n, _dev(rp), _dev(col), _dev(val), fmt, **kw)
        return sp.Plan.from_csr(m, n, rp, col, val, fmt, build="host", **kw)
    except sp.SpmvError as e:
        assert "not supported" in str(e), (fmt, kw, e)
        return None


def _same_layout(a, b, what):
    assert list(a) == list(b), (what, list(a), list(b))
    bad = [k for k in a if a[k] != b[k]]
    assert not bad, f"{what}: arrays {bad} differ from the fresh build"


def _run(plan, x):
    y = np.full(plan.m, np.nan)
    plan.execute(np.ascontiguousarray(x), y)
    return y


def _refresh_and_compare(m, n, rp, col, v0, v1, x, fmt, kw, device, what, ref=None):
    """P from v0, refreshed to v1, must be F1 (fresh from v1); refreshed back
    to v0, F0.  Returns False where the builder refuses the combination."""
    P = _build(m, n, rp, col, v0, fmt, kw, device)
    if P is None:
        return False
    F0 = _build(m, n, rp, col, v0, fmt, kw, device)
    F1 = _build(m, n, rp, col, v1, fmt, kw, device)
    _same_layout(P.digest(), F0.digest(), what + " (two fresh builds)")
    if device:
        P.prepare_update(_dev(rp), _dev(col))
        P.update_values(_dev(v1))
    else:
        P.prepare_update(rp, col)
        P.update_values(np.ascontiguousarray(v1))
    _same_layout(P.digest(), F1.digest(), what + " after update_values(v1)")
    yP, yF = _run(P, x), _run(F1, x)
    if P.info()["format"] == "coo":  # unordered atomics
        si.assert_rows(yF, rp, col, v1, x, what + " fresh coo", ref=ref)
    else:
        assert np.array_equal(yP, yF, equal_nan=True), what
    if ref is not None or P.info()["format"] == "coo":
        si.assert_rows(yP, rp, col, v1, x, what + " updated", ref=ref)
    P.update_values(_dev(v0) if device else np.ascontiguousarray(v0))
    _same_layout(P.digest(), F0.digest(), what + " after update_values(v0)")
    for q in (P, F0, F1):
        q.destroy()
    return True


# ---- 1. update equals rebuild -----------------------------------------------
@pytest.mark.parametrize("fmt,kw", FORMATS, ids=FORMAT_IDS)
@pytest.mark.parametrize("name", si.STRUCTURES)
def test_update_equals_rebuild(name, fmt, kw):
    """Every structure x format: host builders and host arrays on the even
    structures, from_device_csr and CUDA tensors on the odd ones."""
    device = si.STRUCTURES.index(name) % 2 == 1
    c0, c1 = si.case(name, "spread"), si.case(name, "cancel")
    if not _refresh_and_compare(c1["m"], c1["n"], c1["rp"], c1["col"], c0["val"], c1["val"], c1["x"], fmt, kw,
                                device, f"{name} {fmt} {kw} {'device' if device else 'host'}", ref=c1["ref"]):
        pytest.skip(f"{fmt} {kw} does not hold {name}")


# ---- 2. padding and signs ---------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt,kw", [("dia", {}), ("ell", {}), ("csr", {})])
def test_negative_zero_nan_inf(fmt, kw, device):
    """5 % -0.0, one NaN and one +Inf among the new values: the digests are
    the fresh build's (DIA stores -0.0 as +0.0, ELL and CSR as it is; padding
    stays +0.0), and y is non-finite exactly where the fresh plan's is."""
    c = si.case("banded", "cancel")
    rng = np.random.default_rng(77)
    v1 = c["val"].copy()
    nnz = len(v1)
    v1[rng.random(nnz) < 0.05] = -0.0
    v1[nnz // 3] = np.nan
    v1[2 * nnz // 3] = np.inf
    m, n, rp, col, x = c["m"], c["n"], c["rp"], c["col"], c["x"]
    P, F1 = _build(m, n, rp, col, c["val"], fmt, kw, device), _build(m, n, rp, col, v1, fmt, kw, device)
    if device:
        P.prepare_update(_dev(rp), _dev(col))
        P.update_values(_dev(v1))
    else:
        P.prepare_update(rp, col)
        P.update_values(v1)
    _same_layout(P.digest(), F1.digest(), f"{fmt} special values")
    yP, yF = _run(P, x), _run(F1, x)
    assert np.array_equal(np.isfinite(yP), np.isfinite(yF))
    assert 0 < np.count_nonzero(~np.isfinite(yF)) < m // 100
    assert np.array_equal(yP, yF, equal_nan=True)


# ---- 3. unsorted rows and duplicate columns ------------------------------------
def _unsorted_csr(seed=5):
    """About 3 000 rows: empty, short and a few long rows, columns with
    duplicates, every tenth row (or so) shuffled."""
    rng = np.random.default_rng(seed)
    m, n = 3001, 5000
    lens = rng.integers(0, 9, m)
    lens[rng.random(m) < 0.15] = 0
    lens[rng.choice(m, 15, replace=False)] = rng.integers(100, 600, 15)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rp[-1])
    col = rng.integers(0, n, nnz).astype(np.int32)
    dup = rng.random(nnz) < 0.1
    dup[rp[:-1][lens > 0]] = False  # a row's first entry has no predecessor in its row
    col[dup] = col[np.flatnonzero(dup) - 1]
    for r in range(m):
        a, z = rp[r], rp[r + 1]
        if z - a > 1:
            col[a:z] = np.sort(col[a:z]) if rng.random() > 0.1 else rng.permutation(col[a:z])
    v0 = rng.choice([-1.0, 1.0], nnz) * (rng.random(nnz) + 0.01)
    v1 = rng.choice([-1.0, 1.0], nnz) * (rng.random(nnz) + 0.01)
    x = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)
    return m, n, rp, col, v0, v1, x


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", ["csr", "ell", "ss", "coo", "css", "bin"])
def test_unsorted_rows_and_duplicates(fmt, device):
    m, n, rp, col, v0, v1, x = _unsorted_csr()
    assert _refresh_and_compare(m, n, rp, col, v0, v1, x, fmt, {}, device, f"unsorted {fmt}")


def _dup_band():
    m = n = 1000
    rows, cols = [], []
    for r in range(m):
        cs = [c for c in (r - 1, r, r, r + 1) if 0 <= c < n]  # the diagonal entry twice
        rows.append(len(cs))
        cols += cs
    rp = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    rng = np.random.default_rng(9)
    return m, n, rp, np.asarray(cols, np.int32), rng.random(len(cols)) + 0.5, rng.random(n) + 0.5


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_dia_with_merged_entries_is_not_supported(device):
    m, n, rp, col, val, x = _dup_band()
    P = _build(m, n, rp, col, val, "dia", {}, device)
    y0, d0 = _run(P, x), P.digest()
    with pytest.raises(sp.SpmvError, match="not supported"):
        P.prepare_update(*((_dev(rp), _dev(col)) if device else (rp, col)))
    with pytest.raises(sp.SpmvError, match="not prepared"):
        P.update_values(val * 2.0)
    assert P.digest() == d0 and np.array_equal(_run(P, x), y0)


# ---- 4. wrong pattern -----------------------------------------------------------
def _wrong_patterns(rp, col, n):
    """(same row_ptr, one column index changed), (same nnz, the lengths of two
    neighbouring rows swapped)."""
    lens = np.diff(rp)
    j = len(col) // 2
    col2 = col.copy()
    col2[j] = (int(col[j]) + 1) % n
    r = next(r for r in range(len(lens) // 2, len(lens) - 1) if lens[r] != lens[r + 1] and min(lens[r:r + 2]) > 0)
    rp2 = rp.copy()
    rp2[r + 1] = rp[r] + lens[r + 1]
    assert rp2[-1] == rp[-1] and np.all(np.diff(rp2) >= 0) and not np.array_equal(rp2, rp)
    return [("column", rp, col2), ("row lengths", rp2, col)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt", ["csr", "ell", "hyb", "ss", "coo", "css", "bin"])
def test_wrong_pattern_is_refused(fmt, device):
    c0, c1 = si.case("powerlaw", "spread"), si.case("powerlaw", "cancel")
    m, n, rp, col, x = c0["m"], c0["n"], c0["rp"], c0["col"], c0["x"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, {}, device), _build(m, n, rp, col, c1["val"], fmt, {}, device)
    y0, d0 = _run(P, x), P.digest()

    def unchanged(y):  # COO's atomics are unordered: its y is checked against the reference instead
        if fmt == "coo":
            si.assert_rows(y, rp, col, c0["val"], x, "coo after a refused prepare", ref=c0["ref"])
            return True
        return np.array_equal(y, y0)

    for what, rp2, col2 in _wrong_patterns(rp, col, n):
        with pytest.raises(sp.SpmvError, match="invalid value.*pattern"):
            P.prepare_update(*((_dev(rp2), _dev(col2)) if device else (rp2, col2)))
        with pytest.raises(sp.SpmvError, match="not prepared"):
            P.update_values(c1["val"])
        assert P.digest() == d0, (fmt, what)
        assert unchanged(_run(P, x)), (fmt, what)
    P.prepare_update(*((_dev(rp), _dev(col)) if device else (rp, col)))
    P.prepare_update(rp, col)  # prepared: a cheap success
    P.update_values(c1["val"])
    _same_layout(P.digest(), F1.digest(), f"{fmt} after the right pattern")


def test_wrong_pattern_dia_moved_entry():
    """DIA keeps no column indices: an entry moved to another stored diagonal
    leaves `off` alone and is caught by the value slots (the plan holds a
    non-zero where the pattern leaves the slot empty)."""
    c = si.case("banded", "spread")
    m, n, rp, col, x = c["m"], c["n"], c["rp"], c["col"], c["x"]
    P = _build(m, n, rp, col, c["val"], "dia", {}, False)
    y0, d0 = _run(P, x), P.digest()
    col2 = col.copy()
    j = int(rp[m // 2]) + 3
    col2[j] = col[j] + 1  # inside the band: the neighbour's diagonal
    with pytest.raises(sp.SpmvError, match="invalid value.*pattern"):
        P.prepare_update(rp, col2)
    assert P.digest() == d0 and np.array_equal(_run(P, x), y0)
    P.prepare_update(rp, col)


# ---- 5. alignment and tails -----------------------------------------------------
@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("csr", {"csr_lanes": 4}), ("ell", {}), ("dia", {}), ("bin", {})])
def test_val_view_one_double_into_its_allocation(fmt, kw):
    torch = _torch()
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col = c1["m"], c1["n"], c1["rp"], c1["col"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, kw, True), _build(m, n, rp, col, c1["val"], fmt, kw, True)
    base = torch.zeros(len(col) + 3, dtype=torch.float64, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[1:1 + len(col)]
    view.copy_(_dev(c1["val"]))
    assert view.data_ptr() % 16 == 8
    P.prepare_update(_dev(rp), _dev(col))
    P.update_values(view)
    _same_layout(P.digest(), F1.digest(), f"{fmt} {kw} from an 8-byte aligned val")
    assert base[0].item() == 0.0 and not base[1 + len(col):].any().item()


def _tiny_cases():
    m, n, rp, col = si.structure("rect7x1000")
    yield "rect7x1000", m, n, rp, col
    for k in (1, 2, 3):  # its last row shortened: nnz = 31, 30, 29
        assert rp[-1] - rp[-2] > k
        rp2 = rp.copy()
        rp2[-1] -= k
        yield f"rect7x1000-{k}", m, n, rp2, col[:len(col) - k]
    yield "nnz1", 5, 9, np.array([0, 0, 0, 1, 1, 1], np.int64), np.array([7], np.int32)
    yield "nnz0", 5, 9, np.zeros(6, np.int64), np.zeros(0, np.int32)
    yield "m0", 0, 9, np.zeros(1, np.int64), np.zeros(0, np.int32)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("csr", {"csr_lanes": 4}), ("ell", {}), ("coo", {}), ("ss", {})])
def test_tails_and_empty_plans(fmt, kw, device):
    """Value-slot counts that are no multiple of 4 (CSR in CSR order: nnz + 8
    slots) and plans without entries or rows: both calls succeed."""
    rng = np.random.default_rng(3)
    tails = set()
    for name, m, n, rp, col in _tiny_cases():
        nnz = len(col)
        if device and nnz == 0:  # an empty torch tensor has no address to hand over
            continue
        v0, v1, x = rng.random(nnz) + 0.5, -rng.random(nnz) - 0.5, rng.random(n) + 0.5
        if fmt == "csr" and not kw and m:
            probe = sp.Plan.from_csr(m, n, rp, col, v0, fmt)
            if probe.info()["csr_lanes"] == 0:
                tails.add((nnz + 8) % 4)
            probe.destroy()
        assert _refresh_and_compare(m, n, rp, col, v0, v1, x, fmt, kw, device, f"{name} {fmt} {kw}"), (name, fmt)
    if fmt == "csr" and not kw:
        assert tails == {0, 1, 2, 3}, tails  # every length of the gather's scalar tail ran


# ---- refusals that need a plan ------------------------------------------------
def test_refusals_with_a_plan():
    L = sp.lib()
    c = si.case("rect513x40", "spread")
    P = sp.Plan.from_csr(c["m"], c["n"], c["rp"], c["col"], c["val"], "csr")
    rp, col, val = c["rp"], np.ascontiguousarray(c["col"]), np.ascontiguousarray(c["val"])
    d0 = P.digest()

    def last():
        return L.spmv_last_error().decode()

    assert L.spmv_plan_update_prepare(P._h, None, col.ctypes.data, 0) == 1 and "row_ptr is NULL" in last()
    assert L.spmv_plan_update_prepare(P._h, rp.ctypes.data, None, 0) == 1 and "col_idx is NULL" in last()
    assert L.spmv_plan_update_values(P._h, None, 0) == 1 and "val is NULL" in last()
    assert L.spmv_plan_update_values(P._h, val.ctypes.data, sp.ASYNC) == 1
    assert "SPMV_ASYNC without SPMV_VAL_DEVICE" in last()
    assert L.spmv_plan_update_values(P._h, val.ctypes.data, 0) == 1 and "not prepared" in last()
    assert L.spmv_plan_update_values(P._h, val.ctypes.data, 0x1) == 1 and "flag bits" in last()
    P.prepare_update(rp, col)
    # SPMV_VAL_DEVICE with a host pointer: refused, values untouched
    assert L.spmv_plan_update_values(P._h, val.ctypes.data, sp.VAL_DEVICE) == 1 and "device memory" in last()
    assert P.digest() == d0


# ---- 6. stream and graph ----------------------------------------------------------
@pytest.mark.parametrize("fmt", ["csr", "ss", "bin", "dia", "coo"])
def test_async_update_on_a_stream(fmt):
    torch = _torch()
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col, x = c1["m"], c1["n"], c1["rp"], c1["col"], c1["x"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, {}, True), _build(m, n, rp, col, c1["val"], fmt, {}, True)
    P.prepare_update(_dev(rp), _dev(col))
    dx, dv1 = _dev(x), _dev(c1["val"])
    dy = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    P.set_stream(s)
    try:
        P.update_values(dv1, async_=True)
        P.execute(dx, dy, async_=True)
        s.synchronize()
    finally:
        P.set_stream(None)
    y = dy.cpu().numpy()
    if fmt == "coo":
        si.assert_rows(y, rp, col, c1["val"], x, "coo on a stream", ref=c1["ref"])
    else:
        assert np.array_equal(y, _run(F1, x))
    _same_layout(P.digest(), F1.digest(), f"{fmt} async update")


@pytest.mark.parametrize("fmt", ["csr", "ell", "ss", "dia", "bin", "hyb"])
def test_graph_captured_before_the_update_replays_new_values(fmt):
    torch = _torch()
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col, x = c1["m"], c1["n"], c1["rp"], c1["col"], c1["x"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, {}, False), _build(m, n, rp, col, c1["val"], fmt, {}, False)
    dx = _dev(x)
    dy = torch.full((m,), float("nan"), dtype=torch.float64, device="cuda")
    g = P.graph(dx, dy)
    g.launch()
    y_old = dy.cpu().numpy()
    assert np.array_equal(y_old, _run(P, x))
    P.prepare_update(rp, col)
    P.update_values(c1["val"])
    dy.fill_(float("nan"))
    torch.cuda.synchronize()
    g.launch()
    y_new = dy.cpu().numpy()
    assert np.array_equal(y_new, _run(F1, x)) and not np.array_equal(y_new, y_old)
    g.destroy()


# ---- 7. multi after update ----------------------------------------------------------
@pytest.mark.parametrize("fmt", ["dia", "ell"])
def test_fused_multi_sees_the_new_values(fmt):
    torch = _torch()
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col = c1["m"], c1["n"], c1["rp"], c1["col"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, {}, True), _build(m, n, rp, col, c1["val"], fmt, {}, True)
    P.prepare_update(_dev(rp), _dev(col))
    P.update_values(_dev(c1["val"]))
    rng = np.random.default_rng(8)
    X = rng.choice([-1.0, 1.0], (n, 8)) * rng.uniform(0.5, 2.0, (n, 8))
    dX = _dev(X)
    dY = torch.full((m, 8), float("nan"), dtype=torch.float64, device="cuda")
    assert P.multi_path(dX, dY) == [8]
    P.execute_multi(dX, dY)
    Y = dY.cpu().numpy()
    for j in range(8):
        assert np.array_equal(Y[:, j], _run(F1, X[:, j])), (fmt, j)


@pytest.mark.parametrize("fmt", ["csr", "bin"])
def test_columnwise_multi_sees_the_new_values(fmt):
    """The column-by-column execute_multi (one generic execute per column
    through the plan's pack and unpack buffers) on a refreshed plan."""
    torch = _torch()
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col = c1["m"], c1["n"], c1["rp"], c1["col"]
    P, F1 = _build(m, n, rp, col, c0["val"], fmt, {}, True), _build(m, n, rp, col, c1["val"], fmt, {}, True)
    rng = np.random.default_rng(8)
    X = rng.choice([-1.0, 1.0], (n, 3)) * rng.uniform(0.5, 2.0, (n, 3))
    dX = _dev(X)

    def multi(plan):
        dY = torch.full((m, 3), float("nan"), dtype=torch.float64, device="cuda")
        assert plan.multi_path(dX, dY) == [1, 1, 1]
        plan.execute_multi(dX, dY)
        return dY.cpu().numpy()

    Y_old = multi(P)  # the pack and unpack buffers exist before the refresh
    P.prepare_update(_dev(rp), _dev(col))
    P.update_values(_dev(c1["val"]))
    Y, Y_fresh = multi(P), multi(F1)
    assert np.array_equal(Y, Y_fresh) and not np.array_equal(Y, Y_old), fmt
    for j in range(3):
        assert np.array_equal(Y[:, j], _run(F1, X[:, j])), (fmt, j)
    for q in (P, F1):
        q.destroy()


# ---- 8. axpby after update ----------------------------------------------------------
# the three CSR kernels (uniform16: slab2, banded: slabx, powerlaw: adaptive), sliced ELL with and without perm and
# DIA take alpha and beta in their store; the others run into the plan's scratch, which the first call allocates
AXPBY_AFTER_UPDATE = [("uniform16", "csr", {"csr_lanes": 0}, "csr_slab2_kernel"),
                      ("banded", "csr", {"csr_lanes": 0}, "csr_slabx_kernel"),
                      ("powerlaw", "csr", {"csr_lanes": 0}, "csr_adaptive_kernel"),
                      ("uniform16", "ell", {}, "ell_slice_kernel"),
                      ("staircase", "jds", {"ell_width": 9000}, "ell_slice_kernel<perm>"),  # no overflow rows
                      ("banded", "dia", {}, None), ("powerlaw", "ss", {}, None), ("powerlaw", "hyb", {}, None),
                      ("powerlaw", "css", {}, None), ("powerlaw", "bin", {}, None), ("powerlaw", "coo", {}, None)]
AB = (-2.5, 0.75)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,fmt,kw,kernel", AXPBY_AFTER_UPDATE, ids=[f"{a[0]}-{a[1]}" for a in AXPBY_AFTER_UPDATE])
def test_axpby_sees_the_new_values(name, fmt, kw, kernel, device):
    """execute_axpby on a plan refreshed from values A to values B is, bit for
    bit, execute_axpby on a plan built from B (COO: within
    axpby_inputs.assert_bound, and bit for bit on the rows inside one
    128-entry unit), and back again.  The plan has run execute_axpby before
    the refresh, so a generic plan already owns its scratch: the refreshed
    layout still digests as the fresh one's, and device_bytes does not move
    across update_values (host values: by the staging buffer of 8 nnz, once)
    nor across the next execute_axpby -- nothing was allocated anew."""
    torch = _torch()
    cA, cB = ai.refresh_cases(name)
    m, n, rp, col, nnz = cB["m"], cB["n"], cB["rp"], cB["col"], len(cB["col"])
    what = f"{name} {fmt} {'device' if device else 'host'}"
    P, FA, FB = (_build(m, n, rp, col, v, fmt, kw, device) for v in (cA["val"], cA["val"], cB["val"]))
    info = P.info()
    fused = fmt in ("csr", "ell", "dia", "jds")
    assert info["format"] == fmt and (kernel is None or info["kernel"].startswith(kernel)), info["kernel"]
    assert P.axpby_path() == ("fused" if fused else "generic") and (fmt != "jds" or info["overflow_nnz"] == 0)
    digest_B = FB.digest()  # before FB's own execute_axpby: without a scratch
    dx, y0 = _dev(cB["x"]), ai.y0(m)

    def axpby(plan):
        dy = _dev(y0)
        plan.execute_axpby(dx, dy, *AB)
        return dy.cpu().numpy()

    def same(y, fresh, c, tag):
        rows = np.ones(m, bool)
        if fmt == "coo":  # unordered f64 atomics: only a row inside one unit gets its sum in one piece
            rows = (rp[:-1] // 128 == (rp[1:] - 1) // 128) | (np.diff(rp) == 0)
            ai.assert_bound(fresh, rp, c["ref"], y0, *AB, f"{what} {tag} fresh")
        bad = np.flatnonzero((ai.bits(y) != ai.bits(fresh)) & rows)
        assert not len(bad), (f"{what} {tag}: {len(bad)} rows differ from the fresh plan's, first {bad[:5].tolist()}: "
                              f"{y[bad[:3]].tolist()} vs {fresh[bad[:3]].tolist()}")
        ai.assert_bound(y, rp, c["ref"], y0, *AB, f"{what} {tag}")

    b_built = info["device_bytes"]
    y_A = axpby(P)
    b0 = P.info()["device_bytes"]
    assert b0 - b_built == 0 if fused else b0 - b_built >= 8 * m, (what, b0 - b_built)
    same(y_A, axpby(FA), cA, "before the refresh")
    P.prepare_update(*((_dev(rp), _dev(col)) if device else (rp, col)))
    b1 = P.info()["device_bytes"]
    P.update_values(_dev(cB["val"]) if device else np.ascontiguousarray(cB["val"]))
    b2 = P.info()["device_bytes"]
    assert b2 - b1 == (0 if device else 8 * nnz), (what, b2 - b1)
    _same_layout(P.digest(), digest_B, what + " after update_values(B), holding the scratch")
    y_B = axpby(P)
    assert P.info()["device_bytes"] == b2, f"{what}: execute_axpby allocated again after the refresh"
    same(y_B, axpby(FB), cB, "after update_values(B)")
    stale = ai.bits(y_B) == ai.bits(y_A)
    live = np.diff(rp) > 0
    assert 2 * int((~stale & live).sum()) >= int(live.sum()), f"{what}: {int(stale[live].sum())} rows kept A's result"
    P.update_values(_dev(cA["val"]) if device else np.ascontiguousarray(cA["val"]))
    assert P.info()["device_bytes"] == b2
    same(axpby(P), y_A, cA, "after update_values(A)")
    for q in (P, FA, FB):
        q.destroy()


# ---- 9. memory accounting -----------------------------------------------------------
def _value_slots(info, nnz):
    """(value slots, value arrays) of a plan, from the layouts of
    include/spmv_hip.h: CSR nnz (rounded up to 256 in the row-group order)
    + 8, HYB / JDS the slots + 8 of the overflow, BIN its Mul entries + one
    batch of 512, every other format its stored slots."""
    f = info["format"]
    if f == "csr":
        return (nnz if info["csr_lanes"] == 0 else (nnz + 255) // 256 * 256) + 8, 1
    if f in ("hyb", "jds"):
        return info["stored_slots"] + 8, 2
    if f == "bin":
        return info["stored_slots"] + 512, 1
    return info["stored_slots"], 1


@pytest.mark.parametrize("fmt,kw", [("csr", {}), ("csr", {"csr_lanes": 4}), ("ell", {}), ("hyb", {"ell_width": 4}),
                                    ("ss", {}), ("dia", {}), ("coo", {}), ("css", {}), ("bin", {})])
def test_memory_accounting(fmt, kw):
    c0, c1 = si.case("banded", "spread"), si.case("banded", "cancel")
    m, n, rp, col = c1["m"], c1["n"], c1["rp"], c1["col"]
    nnz = len(col)
    P = _build(m, n, rp, col, c0["val"], fmt, kw, False)
    b0 = P.info()["device_bytes"]
    P.prepare_update(rp, col)
    b1 = P.info()["device_bytes"]
    slots, arrays = _value_slots(P.info(), nnz)
    assert 4 * nnz <= b1 - b0 <= 8 * slots + 4096 * arrays, (fmt, b1 - b0, slots)
    P.prepare_update(rp, col)
    assert P.info()["device_bytes"] == b1
    dv0, dv1 = _dev(c0["val"]), _dev(c1["val"])
    for v in (dv1, dv0, dv1):  # device values: no staging at all
        P.update_values(v)
        assert P.info()["device_bytes"] == b1
    P.update_values(c1["val"])  # the first host update allocates the staging buffer
    b2 = P.info()["device_bytes"]
    assert b2 - b1 == 8 * nnz
    for v in (c0["val"], c1["val"]):  # the second and the third do not
        P.update_values(v)
        assert P.info()["device_bytes"] == b2
    P.destroy()
