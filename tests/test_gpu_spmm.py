"""smvp_csr_spmm (K7) on the GPU: Y = A X for k vectors, every column bit for bit the serial loop (the oracle's csr_spmv).

Y always lies in a guarded buffer: GUARD words in front of and behind it (parity.check_guards), NaN in every slot the call
writes, GUARD in the padding columns k <= v < ldy, which must keep their bits.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
from conftest import REPORTS, SAMPLES
from parity import G, GUARD, check_guards

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 8, 16, 17, 40)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def guarded_Y(torch, rows, k, ldy):
    """(buffer, Y): Y = the first k columns of a rows x ldy row-major block inside buffer, NaN; padding and guards GUARD."""
    buf = torch.empty(rows * ldy + 2 * G, dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(int(GUARD))
    Y = buf[G:G + rows * ldy].view(rows, ldy)[:, :k]
    Y.fill_(float("nan"))
    return buf, Y


def check_Y_guards(buf, rows, k, ldy):
    check_guards(buf, rows * ldy)
    h = buf.cpu().numpy().view(np.int64)[G:G + rows * ldy].reshape(rows, ldy)
    assert (h[:, k:] == GUARD).all(), "a padding column k <= v < ldy was written"


def dev_X(torch, X, ldx):
    """X (cols x k, host) on the device with leading dimension ldx (a column slice of a wider array when ldx > k)."""
    cols, k = X.shape
    full = torch.full((cols, ldx), float("nan"), dtype=torch.float64, device="cuda")
    full[:, :k] = torch.from_numpy(np.ascontiguousarray(X))
    return full[:, :k]


def oracle(rp, ci, v, X):
    return np.stack([ob.csr_spmv(rp, ci, v, np.ascontiguousarray(X[:, c])) for c in range(X.shape[1])], axis=1).reshape(
        len(rp) - 1, X.shape[1])


def same_bits(a, b):
    """Bit-equal, except that any NaN equals any NaN (the host and the GPU make different NaN payloads)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def assert_bits(y, ref, what=""):
    ok = same_bits(y, ref)
    if not ok.all():
        r, c = np.argwhere(~ok)[0] if ok.ndim == 2 else (np.flatnonzero(~ok)[0], 0)
        raise AssertionError("%s: %d entries differ from the serial loop's bits; first (%d, %d): %r against %r" % (
            what, (~ok).sum(), r, c, np.asarray(y).reshape(ok.shape)[r, c] if ok.ndim == 2 else y[r],
            np.asarray(ref).reshape(ok.shape)[r, c] if ok.ndim == 2 else ref[r]))


def spmm(torch, A, X, k, ldx, ldy, stream=None):
    """A X[:, :k] through smvp_csr_spmm into a guarded Y; returns Y on the host after the guard checks."""
    dX = dev_X(torch, X[:, :k], ldx)
    buf, Y = guarded_Y(torch, A.rows, k, ldy)
    A.spmm(dX, Y, stream=stream)
    torch.cuda.synchronize()
    check_Y_guards(buf, A.rows, k, ldy)
    return Y.cpu().numpy()


def load(name):
    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
    rp, ci, v = sm.csr_from_coo(coo, m)
    return m, n, rp, ci, v


# ----------------------------------------------------------------------------------------------------------- 1. samples
@pytest.mark.parametrize("name", SAMPLES)
def test_spmm_sample_matrices_every_k_operand_and_leading_dimension(torch, name):
    m, n, rp, ci, v = load(name)
    A = sm.CsrMatrix(m, n, rp, ci, v)
    kmax = max(KS)
    for operand in ("ones", "random"):
        X = np.ones((n, kmax)) if operand == "ones" else np.random.default_rng(11).standard_normal((n, kmax))
        ref = oracle(rp, ci, v, X)
        for k in KS:
            for px, py in ((0, 0), (5, 5), (0, 5), (5, 0)):     # ldx, ldy in {k, k + 5}, mixed pairs included
                Y = spmm(torch, A, X, k, k + px, k + py)
                assert_bits(Y, ref[:, :k], "%s %s k=%d ldx=k+%d ldy=k+%d" % (name, operand, k, px, py))
    A.close()


# -------------------------------------------------------------------------------------------------- 2. committed reports
@pytest.mark.parametrize("name", SAMPLES)
def test_spmm_ones_prints_the_committed_report_on_every_row(torch, name):
    m, n, rp, ci, v = load(name)
    A = sm.CsrMatrix(m, n, rp, ci, v)
    Y = spmm(torch, A, np.ones((n, 8)), 8, 8, 8)
    A.close()
    want = ob.report_y_lines(ob.read_report("smvp-toolbox_report_CSR_%s.txt" % REPORTS[name][0]))
    for c in range(8):
        got = ob.fmt_g(Y[:, c])
        bad = [i for i in range(m) if got[i] != want[i]]
        assert not bad, "%s column %d: %d rows print differently, first %d: %s against %s" % (name, c, len(bad), bad[0],
                                                                                             got[bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------------- 3. edge cases
def csr_of(rows, cols, lists, rng):
    """CSR arrays from per-row column lists (values seeded)."""
    rp = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    ci = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return rp, ci, rng.uniform(-1, 1, len(ci))


def run_case(torch, rows, cols, rp, ci, v, X, ldx=None, ldy=None):
    k = X.shape[1]
    A = sm.CsrMatrix(rows, cols, rp, ci, v)
    Y = spmm(torch, A, X, k, ldx or k, ldy or k)
    A.close()
    ref = oracle(rp, ci, v, X) if rows else np.zeros((0, k))
    assert_bits(Y, ref, "rows=%d cols=%d k=%d" % (rows, cols, k))
    return Y


def test_spmm_edge_cases(torch):
    rng = np.random.default_rng(5)
    # no rows
    run_case(torch, 0, 5, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0), rng.random((5, 3)))
    # no entries: every row +0.0
    Y = run_case(torch, 9, 4, np.zeros(10, np.int32), np.zeros(0, np.int32), np.zeros(0), rng.random((4, 5)))
    assert (Y.view(np.int64) == 0).all()
    # empty rows between full ones
    lists = [sorted(rng.choice(300, rng.integers(1, 40), replace=False)) if r % 3 else [] for r in range(200)]
    run_case(torch, 200, 300, *csr_of(200, 300, lists, rng), rng.standard_normal((300, 6)))
    # one row of 50 000 entries among short ones
    lists = [sorted(rng.choice(60000, 5, replace=False)) for _ in range(5000)]
    lists[1234] = np.sort(rng.choice(60000, 50000, replace=False))
    run_case(torch, 5000, 60000, *csr_of(5000, 60000, lists, rng), rng.standard_normal((60000, 9)))
    # one column
    lists = [[0] * int(rng.integers(0, 2)) for _ in range(777)]
    run_case(torch, 777, 1, *csr_of(777, 1, lists, rng), rng.standard_normal((1, 4)))
    # k = 1, ldx = ldy = 1
    lists = [sorted(rng.choice(100, rng.integers(0, 50), replace=False)) for _ in range(100)]
    run_case(torch, 100, 100, *csr_of(100, 100, lists, rng), rng.standard_normal((100, 1)), 1, 1)
    # non-finite operands: inf, -inf and NaN where the serial loop puts them
    lists = [sorted(rng.choice(64, rng.integers(0, 20), replace=False)) for _ in range(500)]
    X = rng.standard_normal((64, 8))
    X[3, 0], X[10, 1], X[20, 2], X[20, 3], X[40, 4] = np.inf, -np.inf, np.nan, np.inf, np.nan
    Y = run_case(torch, 500, 64, *csr_of(500, 64, lists, rng), X)
    assert not np.isfinite(Y).all() and np.isfinite(Y[:, 5:]).all()


# ----------------------------------------------------------------------------------------------------- 4. independence
@pytest.fixture(scope="module")
def shaped():
    M = 1 << 16
    rp, ci, v = sm.synth_csr(sm.SYNTH_MEMPLUS_SHAPED, 12345, M, M)
    X = np.random.default_rng(7).standard_normal((M, 8))
    return M, rp, ci, v, X, oracle(rp, ci, v, X)


def test_spmm_is_the_same_under_every_spmv_plan_and_twice(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    A = sm.CsrMatrix(M, M, rp, ci, v)
    first = spmm(torch, A, X, 8, 8, 8)
    assert_bits(first, ref, "first call")
    assert_bits(spmm(torch, A, X, 8, 8, 8), first, "second call")
    for kernel, param in ((sm.CSR_KERNEL_STREAM, 0), (sm.CSR_KERNEL_COLSWEEP, 0), (sm.CSR_KERNEL_BINNED, 0),
                          (sm.CSR_KERNEL_VECTOR, 8)):
        A.set_kernel(kernel, param)
        assert_bits(spmm(torch, A, X, 8, 8, 8), first, "under SpMV plan %d" % kernel)
    A.close()


def test_spmv_is_unchanged_by_spmm_on_the_same_handle(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    x = torch.from_numpy(np.ascontiguousarray(X[:, 3])).cuda()

    def spmv(A):
        y = torch.full((M,), float("nan"), dtype=torch.float64, device="cuda")
        A.spmv(x, y)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    fresh = sm.CsrMatrix(M, M, rp, ci, v)
    want = spmv(fresh)
    fresh.close()
    A = sm.CsrMatrix(M, M, rp, ci, v)
    before = spmv(A)
    info = A.plan_info()
    spmm(torch, A, X, 8, 8, 8)
    assert A.plan_info() == info
    after = spmv(A)
    A.close()
    assert_bits(before, want, "spmv before spmm")
    assert_bits(after, want, "spmv after spmm")


def test_spmm_on_a_stream_of_its_own(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    A = sm.CsrMatrix(M, M, rp, ci, v)
    s = torch.cuda.Stream()
    dX = dev_X(torch, X, 8)
    buf, Y = guarded_Y(torch, M, 8, 8)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        A.spmm(dX, Y, stream=s)
    s.synchronize()
    check_Y_guards(buf, M, 8, 8)
    assert_bits(Y.cpu().numpy(), ref, "own stream")
    A.close()


def test_spmm_over_adopted_arrays_sees_val_changed_in_place(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    d_rp, d_ci, d_v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, v))
    A = sm.CsrMatrix(M, M, d_rp, d_ci, d_v)
    assert_bits(spmm(torch, A, X, 8, 8, 8), ref, "adopted")
    v2 = np.random.default_rng(8).uniform(-2, 2, len(v))
    d_v.copy_(torch.from_numpy(v2))
    torch.cuda.synchronize()
    assert_bits(spmm(torch, A, X, 8, 8, 8), oracle(rp, ci, v2, X), "after val changed in place")
    A.close()


# ------------------------------------------------------------------------------------------------------- 5. row blocks
def test_spmm_row_blocks_equal_the_whole_matrix(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    bounds = sm.partition_rows(rp, 5)
    for b in range(5):
        r0, r1 = int(bounds[b]), int(bounds[b + 1])
        e0, e1 = int(rp[r0]), int(rp[r1])
        B = sm.CsrMatrix(r1 - r0, M, (rp[r0:r1 + 1] - e0).astype(np.int32), ci[e0:e1], v[e0:e1], first_row=r0)
        assert_bits(spmm(torch, B, X, 8, 8, 8), ref[r0:r1], "row block %d" % b)
        B.close()


# -------------------------------------------------------------------------------------------------- 6. larger matrices
def test_spmm_memplus_shaped_2_21_rows_k16(torch):
    M = 1 << 21
    rp, ci, v = sm.synth_csr(sm.SYNTH_MEMPLUS_SHAPED, 4242, M, M)
    X = np.random.default_rng(9).standard_normal((M, 16))
    A = sm.CsrMatrix(M, M, rp, ci, v)
    assert_bits(spmm(torch, A, X, 16, 16, 16), oracle(rp, ci, v, X), "memplus-shaped 2^21")
    A.close()


def test_spmm_config4_first_2_20_rows_k8(torch):
    N = 10_000_000
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 12345, N, N, 32, row_end=1 << 20)
    X = np.random.default_rng(10).random((N, 8))
    A = sm.CsrMatrix(1 << 20, N, rp, ci, v)
    assert_bits(spmm(torch, A, X, 8, 8, 8), oracle(rp, ci, v, X), "config 4, first 2^20 rows")
    A.close()


# -------------------------------------------------------------------------------------------- 7. errors on a real handle
def test_spmm_invalid_arguments_write_nothing(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    A = sm.CsrMatrix(M, M, rp, ci, v)
    L = sm.lib()
    k = 4
    dX = dev_X(torch, X[:, :k], k)
    buf, Y = guarded_Y(torch, M, k, k)
    both = torch.full((2 * M * k,), float("nan"), dtype=torch.float64, device="cuda")
    xp, yp = dX.data_ptr(), Y.data_ptr()
    cases = {"k = 0": (0, xp, k, yp, k), "k < 0": (-3, xp, k, yp, k), "ldx < k": (k, xp, k - 1, yp, k),
             "ldy < k": (k, xp, k, yp, k - 1), "null X": (k, None, k, yp, k), "null Y": (k, xp, k, None, k),
             "X is Y": (k, yp, k, yp, k),
             "overlap": (k, both.data_ptr(), k, both.data_ptr() + 8 * (M * k - 1), k)}
    torch.cuda.synchronize()
    for what, (kk, x, ldx, y, ldy) in cases.items():
        rc = L.smvp_csr_spmm(A._h, kk, x, ldx, y, ldy, None)
        assert rc == sm.ERR_INVALID, (what, rc)
        assert "smvp_csr_spmm" in L.smvp_last_error().decode()
    torch.cuda.synchronize()
    check_Y_guards(buf, M, k, k)
    assert np.isnan(Y.cpu().numpy()).all(), "a refused call wrote Y"
    assert torch.isnan(both).all()
    assert A.spmm_describe(k)[2]["plan_bytes"] == 0      # nothing was built either
    A.close()


# ------------------------------------------------------------------------------------------------------ 8. graph capture
def test_spmm_capture_after_a_warm_call_and_refused_before(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    k, ldx, ldy = 8, 10, 11
    A = sm.CsrMatrix(M, M, rp, ci, v)
    dX = dev_X(torch, np.zeros((M, k)), ldx)
    buf, dY = guarded_Y(torch, M, k, ldy)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # before any call: refused at once, nothing enqueued, no plan half-built (dZ keeps the captured graph from being empty)
    refused = []
    with torch.cuda.stream(s):
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0, stream=s):
            dZ.add_(1.0)
            refused.append(sm.lib().smvp_csr_spmm(A._h, k, dX.data_ptr(), ldx, dY.data_ptr(), ldy, s.cuda_stream))
    del g0
    assert refused == [sm.ERR_INVALID]
    assert "capture" in sm.lib().smvp_last_error().decode()
    assert A.spmm_describe(k)[2]["plan_bytes"] == 0
    torch.cuda.synchronize()
    check_Y_guards(buf, M, k, ldy)
    assert np.isnan(dY.cpu().numpy()).all(), "a refused call wrote Y"
    # one warm call, then a capture replayed with new operands
    with torch.cuda.stream(s):
        A.spmm(dX, dY, stream=s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            A.spmm(dX, dY, stream=s)
    rng = np.random.default_rng(12)
    for _ in range(2):
        Xn = rng.standard_normal((M, k))
        dX.copy_(torch.from_numpy(Xn))
        dY.fill_(float("nan"))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check_Y_guards(buf, M, k, ldy)
        assert_bits(dY.cpu().numpy(), oracle(rp, ci, v, Xn), "graph replay")
    del g
    A.close()


# ------------------------------------------------------------------------------------------------------------ 9. describe
def test_spmm_describe(torch, shaped):
    M, rp, ci, v, X, ref = shaped
    A = sm.CsrMatrix(M, M, rp, ci, v)
    nnz = int(rp[-1])
    for k, name in ((1, "csr_spmm_rows<1>"), (8, "csr_spmm_rows<8>"),
                    (40, "csr_spmm_rows<16> + csr_spmm_rows<16> + csr_spmm_rows<8>")):
        got, alg, plan = A.spmm_describe(k)
        assert got == name
        assert alg == 12.0 * nnz + 4.0 * (M + 1) + 8.0 * k * (M + M)
        assert plan == {"plan_bytes": 0.0, "build_ms": 0.0}
    info = A.plan_info()
    spmm(torch, A, X, 8, 8, 8)
    plan = A.spmm_describe(8)[2]
    assert plan["plan_bytes"] > 0 and plan["build_ms"] > 0
    assert A.plan_info() == info
    with pytest.raises(sm.SmvpError):
        A.spmm_describe(0)
    # the largest k: the name stops at the buffer (255 characters), the bytes are the formula's
    got, alg, _ = A.spmm_describe(2 ** 31 - 1)
    assert got.startswith("csr_spmm_rows<16> + ") and len(got) == 255
    assert alg == 12.0 * nnz + 4.0 * (M + 1) + 8.0 * (2 ** 31 - 1) * (M + M)
    A.close()
