"""The transposed product y = A^T x on the GPU, by both routes: smvp_tjds_spmv_transposed (K8, from the TJDS arrays) and
smvp_csr_create_transposed (A^T as a CSR handle of its own).  Reference: tests/transposed.py -- the host converter's CSR
arrays of the swapped entries under the oracle's serial loop.  Every check is equality of bits (NaN = NaN) except the
transposed handle's default spmv at size, which goes by parity.check_y's bound for a row's term count.

y always lies in parity.guarded_y (NaN-filled, guards checked after every call).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import transposed as tr
from conftest import SAMPLES
from parity import check_guards, check_y, guarded_y

pytestmark = pytest.mark.gpu

TJDS_MODES = (sm.TJDS_MODE_ROW_GATHER, sm.TJDS_MODE_TWO_PHASE, sm.TJDS_MODE_ATOMIC)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load(name):
    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
    return m, n, coo


def k8(torch, T, x, stream=None):
    """A^T x through smvp_tjds_spmv_transposed into a guarded y; the host copy after the guard checks."""
    dx = x if hasattr(x, "is_cuda") else dev(torch, x)
    buf, dy = guarded_y(torch, T.cols)
    T.spmv_transposed(dx, dy, stream=stream)
    torch.cuda.synchronize()
    check_guards(buf, T.cols)
    return dy.cpu().numpy()


def spmm1(torch, At, x):
    """At x through smvp_csr_spmm with k = 1 (the serial loop's bits on every row) into a guarded y."""
    dx = x if hasattr(x, "is_cuda") else dev(torch, x)
    buf, dy = guarded_y(torch, At.rows)
    At.spmm(dx.view(At.cols, 1), dy.view(At.rows, 1))
    torch.cuda.synchronize()
    check_guards(buf, At.rows)
    return dy.cpu().numpy()


def spmv(torch, A, x):
    dx = x if hasattr(x, "is_cuda") else dev(torch, x)
    buf, dy = guarded_y(torch, A.rows)
    A.spmv(dx, dy)
    torch.cuda.synchronize()
    check_guards(buf, A.rows)
    return dy.cpu().numpy()


class _Raw:
    """A device address as an object torch.as_tensor can wrap (the CUDA array interface)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def arrays_of(torch, A):
    """(row_ptr, col_ind, val) of a CsrMatrix copied back from the addresses smvp_csr_device_arrays reports."""
    rp, ci, v = A.device_arrays()
    assert rp and ci and v
    out = [torch.as_tensor(_Raw(rp, A.rows + 1, "<i4"), device="cuda").cpu().numpy().copy()]
    for ptr, typestr, dtype in ((ci, "<i4", np.int32), (v, "<f8", np.float64)):
        out.append(torch.as_tensor(_Raw(ptr, A.nnz, typestr), device="cuda").cpu().numpy().copy() if A.nnz else np.zeros(0, dtype))
    return out


def assert_arrays(got, want, what=""):
    for name, g, w in zip(("row_ptr", "col_ind", "val"), got, want):
        assert g.dtype == w.dtype and g.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: %s differs" % (what, name)


def both_routes(torch, rows, cols, coo, x, what, tjds=True, csr=True, csr_arrays=None):
    """K8 on the TJDS of `coo` and the transposed handle of its CSR (or of csr_arrays): arrays and bits against the reference."""
    ref = tr.reference(coo, rows, cols, x)
    want = tr.transposed_csr(coo, cols)
    if tjds:
        T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
        tr.assert_bits(k8(torch, T, x), ref, what + ": K8")
        T.close()
    if csr:
        A = sm.CsrMatrix(rows, cols, *(csr_arrays or sm.csr_from_coo(coo, rows)))
        At = A.transposed()
        assert (At.rows, At.cols, At.nnz) == (cols, rows, len(coo))
        assert_arrays(arrays_of(torch, At), want, what)
        A.close()                                                     # the transposed handle outlives its source
        tr.assert_bits(spmm1(torch, At, x), ref, what + ": spmm k = 1 on the transposed handle")
        y = spmv(torch, At, x)
        if np.isfinite(x).all():
            scale = ob.csr_spmv(want[0], want[1], np.abs(want[2]), np.abs(x)) if cols else np.zeros(0)
            check_y(y, ref, scale, np.diff(want[0]))
        At.close()
    return ref


# ----------------------------------------------------------------------------------------------------------- 1. samples
@pytest.mark.parametrize("name", SAMPLES)
def test_transposed_sample_matrices_both_routes_every_mode(torch, name):
    m, n, coo = load(name)
    want = tr.transposed_csr(coo, n)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    A = sm.CsrMatrix(m, n, *sm.csr_from_coo(coo, m))
    At = A.transposed()
    assert (At.rows, At.cols, At.nnz) == (n, m, len(coo))
    assert At.get_kernel()[0] != sm.CSR_KERNEL_AUTO
    assert_arrays(arrays_of(torch, At), want, name)
    kname, alg = T.transposed_describe()
    assert kname == "tjds_transposed_columns"
    assert alg == 12.0 * len(coo) + 4.0 * (T._t.num_diag + 1) + 4.0 * n + 8.0 * m + 8.0 * n
    for operand in ("ones", "random"):
        x = np.ones(m) if operand == "ones" else np.random.default_rng(31).standard_normal(m)
        ref = ob.csr_spmv(want[0], want[1], want[2], x)
        for mode in TJDS_MODES:
            T.set_mode(mode)
            tr.assert_bits(k8(torch, T, x), ref, "%s %s mode %d" % (name, operand, mode))
        T.set_ref_quirks(True)
        tr.assert_bits(k8(torch, T, x), ref, "%s %s ref-quirks" % (name, operand))
        T.set_ref_quirks(False)
        T.set_mode(sm.TJDS_MODE_AUTO)
        via_csr = spmm1(torch, At, x)
        tr.assert_bits(via_csr, ref, "%s %s spmm k = 1" % (name, operand))
        tr.assert_bits(via_csr, k8(torch, T, x), "%s %s the two routes" % (name, operand))
    for h in (T, A, At):
        h.close()


# --------------------------------------------------------------------------------------- 2. forward product undisturbed
@pytest.mark.parametrize("mode", TJDS_MODES)
def test_forward_tjds_product_is_undisturbed(torch, mode):
    m, n, coo = load("memplus.mtx")
    rng = np.random.default_rng(32)
    x, xt = rng.standard_normal(n), rng.standard_normal(m)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    T.set_mode(mode)
    info = T.plan_info()
    T.set_x(dev(torch, x))

    def forward():
        buf, dy = guarded_y(torch, m)
        T.zero_y(dy)
        T.spmv(dy)
        torch.cuda.synchronize()
        check_guards(buf, m)
        return dy.cpu().numpy()

    y1 = forward()
    if mode == sm.TJDS_MODE_ATOMIC:                       # (its order of summation varies: the bound, not the bits)
        rp, ci, v = sm.csr_from_coo(coo, m)
        scale = ob.csr_spmv(rp, ci, np.abs(v), np.abs(x))
    tr.assert_bits(k8(torch, T, xt), tr.reference(coo, m, n, xt), "K8 between two forward products")
    y2 = forward()                                        # no new set_x
    if mode == sm.TJDS_MODE_ATOMIC:
        check_y(y2, ob.csr_spmv(rp, ci, v, x), scale, np.diff(rp))
        check_y(y1, ob.csr_spmv(rp, ci, v, x), scale, np.diff(rp))
    else:
        tr.assert_bits(y2, y1, "forward product after K8")
    assert T.plan_info() == info
    T.close()


def test_source_csr_handle_is_undisturbed_by_transposed(torch):
    import ceiling

    M = 1 << 16
    rp, ci, v = sm.synth_csr(sm.SYNTH_MEMPLUS_SHAPED, 12345, M, M)
    d_rp, d_ci, d_v = (dev(torch, a) for a in (rp, ci, v))
    sums = [ceiling.checksum(torch, a) for a in (d_rp, d_ci, d_v)]
    x = np.random.default_rng(33).standard_normal(M)
    A = sm.CsrMatrix(M, M, d_rp, d_ci, d_v)                 # adopted arrays: the call must leave them alone
    assert A.device_arrays() == (d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr())
    kernel, info = A.get_kernel(), A.plan_info()
    before = spmv(torch, A, x)
    At = A.transposed()
    after = spmv(torch, A, x)
    tr.assert_bits(after, before, "source spmv after transposed()")
    assert A.get_kernel() == kernel and A.plan_info() == info
    assert [ceiling.checksum(torch, a) for a in (d_rp, d_ci, d_v)] == sums
    assert set(At.device_arrays()).isdisjoint(A.device_arrays())
    coo = tr.coo_of_csr(rp, ci, v)
    assert_arrays(arrays_of(torch, At), tr.transposed_csr(coo, M), "memplus-shaped 2^16")
    A.close()
    del d_rp, d_ci, d_v
    tr.assert_bits(spmm1(torch, At, x), tr.reference(coo, M, M, x), "after the source is gone")
    At.close()


# ------------------------------------------------------------------------------------------------------- 3. edge cases
def coo_from_lists(rows, lists, rng):
    """COO (row-major storage order) from per-row column lists, seeded values."""
    r = np.repeat(np.arange(rows), [len(l) for l in lists])
    c = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists] + [np.zeros(0, np.int64)])
    return sm.make_coo(r, c, rng.uniform(-1, 1, len(c)))


def test_transposed_edge_cases(torch):
    rng = np.random.default_rng(34)
    empty = sm.make_coo([], [], [])
    # no rows (the CSR create call takes it; the transposed matrix has no columns)
    y = both_routes(torch, 0, 7, empty, np.zeros(0), "0 x 7", tjds=False)
    assert y.shape == (7,) and (y.view(np.int64) == 0).all()
    # no columns: y is empty
    both_routes(torch, 5, 0, empty, rng.standard_normal(5), "5 x 0", tjds=False)
    # no entries: every y +0.0, sign bit included
    for tjds in (True,):
        y = both_routes(torch, 9, 4, empty, -rng.random(9), "9 x 4 without entries", tjds=tjds)
        assert (y.view(np.int64) == 0).all()
    T = sm.TjdsMatrix(sm.tjds_from_coo(empty, 9, 4))
    assert (k8(torch, T, -np.ones(9)).view(np.int64) == 0).all()
    T.close()
    # empty columns between full ones
    lists = [sorted(3 * rng.choice(100, rng.integers(1, 40), replace=False)) for _ in range(200)]
    coo = coo_from_lists(200, lists, rng)
    y = both_routes(torch, 200, 300, coo, rng.standard_normal(200), "empty columns")
    assert (y.view(np.int64)[np.arange(300) % 3 != 0] == 0).all()
    # one column of 50 000 entries beside 3 000 short ones
    lists = [[0] + sorted(1 + rng.choice(3000, int(rng.integers(0, 4)), replace=False)) for _ in range(50000)]
    both_routes(torch, 50000, 3001, coo_from_lists(50000, lists, rng), rng.standard_normal(50000), "one long column")
    # one row; 1 x 1
    both_routes(torch, 1, 500, coo_from_lists(1, [sorted(rng.choice(500, 123, replace=False))], rng), rng.standard_normal(1), "one row")
    both_routes(torch, 1, 1, sm.make_coo([0], [0], [2.5]), np.array([-3.0]), "1 x 1")
    # M >> N and N >> M
    lists = [sorted(rng.choice(3, int(rng.integers(0, 3)), replace=False)) for _ in range(50000)]
    both_routes(torch, 50000, 3, coo_from_lists(50000, lists, rng), rng.standard_normal(50000), "tall")
    lists = [sorted(rng.choice(100000, int(rng.integers(0, 50)), replace=False)) for _ in range(100)]
    both_routes(torch, 100, 100000, coo_from_lists(100, lists, rng), rng.standard_normal(100), "wide")


def test_repeated_pairs_are_summed_in_storage_order(torch):
    # column 1 holds (2, 1) three times: 1e16 + 1 - 1e16 is 0 in storage order, 1 with the small value last
    coo = sm.make_coo([0, 2, 2, 2, 3], [0, 1, 1, 1, 1], [4.0, 1e16, 1.0, -1e16, 0.5])
    x = np.ones(4)
    ref = both_routes(torch, 4, 3, coo, x, "repeated pairs")
    tr.assert_bits(ref, np.array([4.0, 0.5, 0.0]), "the reference itself")
    other = tr.reference(coo[[0, 1, 3, 2, 4]], 4, 3, x)
    assert not tr.same_bits(other, ref), "the values must tell the orders apart"
    both_routes(torch, 4, 3, coo[[0, 1, 3, 2, 4]], x, "repeated pairs, the other order")


def test_csr_rows_with_descending_columns(torch):
    rng = np.random.default_rng(35)
    rows, cols = 300, 200
    lists = [sorted(rng.choice(cols, int(rng.integers(0, 60)), replace=False))[::-1] for _ in range(rows)]
    coo = coo_from_lists(rows, lists, rng)                  # storage order: descending columns inside every row
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    both_routes(torch, rows, cols, coo, rng.standard_normal(rows), "descending col_ind", tjds=False,
                csr_arrays=(rp, coo["col"].astype(np.int32), coo["val"].copy()))


def test_non_finite_operands_stay_in_the_columns_that_touch_them(torch):
    rng = np.random.default_rng(36)
    rows, cols = 64, 500
    lists = [sorted(rng.choice(cols // 2, int(rng.integers(0, 20)), replace=False)) for _ in range(rows)]   # columns < 250
    for r in range(8, rows):
        lists[r] = sorted(set(lists[r]) | set((250 + rng.choice(250, 30, replace=False)).tolist()))       # rows >= 8 reach columns >= 250 too
    coo = coo_from_lists(rows, lists, rng)
    x = rng.standard_normal(rows)
    x[0], x[1], x[2], x[3], x[4] = np.nan, np.inf, -np.inf, -0.0, np.inf
    y = both_routes(torch, rows, cols, coo, x, "non-finite x")
    assert not np.isfinite(y[:250]).all() and np.isfinite(y[250:]).all()


# --------------------------------------------------------------------------------------------------------------- 4. fuzz
@pytest.mark.parametrize("seed", range(25))
def test_transposed_fuzz_both_routes_and_twice_transposed(torch, seed):
    from test_gpu_parity import _fuzz_matrix

    rows, cols, rp, ci, v, _ = _fuzz_matrix(seed)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(rows) * 10.0 ** rng.integers(-3, 3, rows)
    ordered = tr.coo_of_csr(rp, ci, v)
    coo = ordered[rng.permutation(len(ordered))]
    ref = tr.reference(coo, rows, cols, x)
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, rows, cols))
    tr.assert_bits(k8(torch, T, x), ref, "fuzz %d: K8" % seed)
    T.close()
    A = sm.CsrMatrix(rows, cols, *sm.csr_from_coo(coo, rows))
    At = A.transposed()
    tr.assert_bits(spmm1(torch, At, x), ref, "fuzz %d: spmm k = 1" % seed)
    Att = At.transposed()
    assert (Att.rows, Att.cols, Att.nnz) == (rows, cols, len(coo))
    assert_arrays(arrays_of(torch, Att), sm.csr_from_coo(coo, rows), "fuzz %d: transposed twice" % seed)
    for h in (A, At, Att):
        h.close()


# ------------------------------------------------------------------------------------------------------ 5. graph capture
def test_k8_is_captured_as_the_first_call_on_a_fresh_handle(torch):
    m, n, coo = load("memplus.mtx")
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    dx = torch.zeros(m, dtype=torch.float64, device="cuda")
    buf, dy = guarded_y(torch, n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            T.spmv_transposed(dx, dy, stream=s)            # the handle's first call of any kind
    torch.cuda.synchronize()
    assert np.isnan(dy.cpu().numpy()).all(), "a captured call ran"
    rng = np.random.default_rng(37)
    for _ in range(3):
        x = rng.standard_normal(m)
        dx.copy_(torch.from_numpy(x))
        dy.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_guards(buf, n)
        tr.assert_bits(dy.cpu().numpy(), tr.reference(coo, m, n, x), "graph replay")
    del g
    runs = [k8(torch, T, x) for _ in range(3)]
    tr.assert_bits(runs[1], runs[0], "second plain run")
    tr.assert_bits(runs[2], runs[0], "third plain run")
    T.close()


def test_create_transposed_refuses_a_capturing_stream(torch):
    m, n, coo = load("ibm32.mtx")
    A = sm.CsrMatrix(m, n, *sm.csr_from_coo(coo, m))
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    refused, out = [], C.c_void_p(1)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            refused.append(sm.lib().smvp_csr_create_transposed(C.byref(out), A._h, s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert refused == [sm.ERR_INVALID] and not out.value
    assert "smvp_csr_create_transposed" in msg and "captur" in msg
    g.replay()                                               # the capture stayed valid
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16
    del g
    At = A.transposed(stream=s)                              # and outside a capture the same stream is fine
    assert_arrays(arrays_of(torch, At), tr.transposed_csr(coo, n), "on a side stream")
    At.close()
    A.close()


# -------------------------------------------------------------------------------------------------------------- 6. at size
def replicated(rp, ci, v, rows, cols, copies):
    """CSR arrays of kron(I_copies, A)."""
    nnz = int(rp[-1])
    big_rp = (np.arange(copies, dtype=np.int64)[:, None] * nnz + rp[None, :-1].astype(np.int64)).reshape(-1)
    big_rp = np.concatenate([big_rp, [copies * nnz]]).astype(np.int32)
    big_ci = (np.arange(copies, dtype=np.int64)[:, None] * cols + ci[None, :].astype(np.int64)).reshape(-1).astype(np.int32)
    return big_rp, big_ci, np.tile(v, copies)


def at_size(torch, rows, cols, rp, ci, v, t_arrays, x, what):
    """K8 == spmm k = 1 on the transposed handle == the oracle on the reference arrays t_arrays; the transposed handle is the
    handle smvp_csr_create makes from t_arrays (kernel, description, plan bytes) and its default spmv is inside check_y's bound."""
    from test_gpu_parity import _coo_to_device

    nnz = int(rp[-1])
    trp, tci, tv = t_arrays
    ref = ob.csr_spmv(trp, tci, tv, x)
    dx = dev(torch, x)
    A = sm.CsrMatrix(rows, cols, rp, ci, v)
    At = A.transposed()
    A.close()
    assert_arrays(arrays_of(torch, At), t_arrays, what)
    via_csr = spmm1(torch, At, dx)
    tr.assert_bits(via_csr, ref, what + ": spmm k = 1 on the transposed handle")
    Ah = sm.CsrMatrix(cols, rows, trp, tci, tv)
    assert At.get_kernel() == Ah.get_kernel(), what
    assert At.describe() == Ah.describe(), what
    assert At.plan_info()["plan_bytes"] == Ah.plan_info()["plan_bytes"] and At.launches() == Ah.launches(), what
    Ah.close()
    y = spmv(torch, At, dx)
    check_y(y, ref, ob.csr_spmv(trp, tci, np.abs(tv), np.abs(x)), np.diff(trp))
    At.close()
    d_coo = _coo_to_device(torch, tr.coo_of_csr(rp, ci, v))
    t = sm.tjds_from_coo_device(d_coo, rows, cols, nnz)
    del d_coo
    T = sm.TjdsMatrix(t)
    got = k8(torch, T, dx)
    T.close()
    tr.assert_bits(got, ref, what + ": K8")
    tr.assert_bits(got, via_csr, what + ": the two routes")


def test_transposed_memplus_replicated_944_times(torch):
    m, n, coo = load("memplus.mtx")
    copies = 944
    rp, ci, v = sm.csr_from_coo(coo, m)
    big = replicated(rp, ci, v, m, n, copies)
    t_big = replicated(*tr.transposed_csr(coo, n), n, m, copies)      # (I x A)^T = I x A^T
    x = np.random.default_rng(38).standard_normal(m * copies)
    at_size(torch, m * copies, n * copies, *big, t_big, x, "memplus x944")


def test_transposed_config4_shape_1m_rows(torch):
    M = 1_000_000
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 2024, M, M, param=32)
    x = np.random.default_rng(39).random(M)
    at_size(torch, M, M, rp, ci, v, tr.transposed_csr(tr.coo_of_csr(rp, ci, v), M), x, "config 4 at 1 M rows")


# --------------------------------------------------------------------------------------------------------------- 7. errors
def test_transposed_invalid_arguments_write_nothing(torch):
    m, n, coo = load("curtis54.mtx")
    coo = coo[coo["row"] < m - 4]                               # (rows != cols below: x and y differ in length)
    m -= 4
    T = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n))
    L = sm.lib()
    dx = torch.ones(m, dtype=torch.float64, device="cuda")
    buf, dy = guarded_y(torch, n)
    both = torch.full((m + n,), float("nan"), dtype=torch.float64, device="cuda")
    xp, yp, bp = dx.data_ptr(), dy.data_ptr(), both.data_ptr()
    cases = {"null x": (None, yp), "null y": (xp, None), "x is y": (yp, yp), "y inside x": (bp, bp + 8 * (m - 1)),
             "x inside y": (bp + 8 * (n - 1), bp)}
    torch.cuda.synchronize()
    for what, (x, y) in cases.items():
        rc = L.smvp_tjds_spmv_transposed(T._h, x, y, None)
        assert rc == sm.ERR_INVALID, (what, rc)
        assert "smvp_tjds_spmv_transposed" in L.smvp_last_error().decode()
    torch.cuda.synchronize()
    check_guards(buf, n)
    assert np.isnan(dy.cpu().numpy()).all(), "a refused call wrote y"
    assert torch.isnan(both).all()
    # adjacent, not overlapping: accepted
    assert L.smvp_tjds_spmv_transposed(T._h, bp, bp + 8 * m, None) == sm.OK
    both[:m] = 1.0
    assert L.smvp_tjds_spmv_transposed(T._h, bp, bp + 8 * m, None) == sm.OK
    torch.cuda.synchronize()
    tr.assert_bits(both[m:].cpu().numpy(), tr.reference(coo, m, n, np.ones(m)), "x and y side by side")
    # the binding's checks
    with pytest.raises(ValueError):
        T.spmv_transposed(dx[:-1], dy)
    with pytest.raises(ValueError):
        T.spmv_transposed(dx, dy.cpu())
    # a TJDS handle's inner CSR handle (the row-gather plan) is no plain CSR: both CSR calls refuse it
    inner = inner_csr_handle(T, m, n, len(coo))
    out = C.c_void_p(1)
    assert L.smvp_csr_create_transposed(C.byref(out), inner, None) == sm.ERR_UNSUPPORTED and not out.value
    assert "smvp_csr_create_transposed" in L.smvp_last_error().decode()
    rp, ci, v = C.c_void_p(7), C.c_void_p(7), C.c_void_p(7)
    assert L.smvp_csr_device_arrays(inner, C.byref(rp), C.byref(ci), C.byref(v)) == sm.ERR_UNSUPPORTED
    assert "smvp_csr_device_arrays" in L.smvp_last_error().decode()
    assert (rp.value, ci.value, v.value) == (7, 7, 7), "a refused call wrote its outputs"
    out = C.c_void_p(1)
    assert L.smvp_csr_create_transposed(C.byref(out), None, None) == sm.ERR_INVALID and not out.value
    T.close()


def inner_csr_handle(T, rows, cols, nnz):
    """The smvp_csr_t a TJDS handle in ROW_GATHER mode keeps inside (struct smvp_tjds::rg.csr, smvp_tjds.hip).  The C ABI does
    not hand it out, so it is read from the handle's memory: the x86-64 layout of the struct's head is {int device, rows,
    cols, nnz, num_diag; four pointers at 24; four bools at 56; a std::vector at 64; d_x_perm at 88; bool x_set at 96;
    int mode at 100; the three pointers of rg at 104; rg.csr at 128}.  Every field that can be checked is checked on both structs before
    the pointer is used, so a layout that has moved fails here instead of passing something else on."""
    base = T._h.value
    ints = [C.c_int.from_address(base + 4 * i).value for i in range(5)]
    assert ints == [0, rows, cols, nnz, T._t.num_diag], ints
    assert C.c_int.from_address(base + 100).value == sm.TJDS_MODE_ROW_GATHER
    rg = C.c_void_p.from_address(base + 128).value
    assert rg, "no row-gather plan"
    head = [C.c_int.from_address(rg + 4 * i).value for i in range(4)]       # smvp_csr: device, rows, cols, nnz
    assert head[0] == 0 and head[1] == rows and head[3] == nnz, head
    return C.c_void_p(rg)
