"""smvp_csr_spmm (K7) on the GPU: Y = A X for k vectors, every column bit for bit the serial loop (the oracle's csr_spmv).

Y always lies in a guarded buffer: GUARD words in front of and behind it (parity.check_guards), NaN in every slot the call
writes, GUARD in the padding columns k <= v < ldy, which must keep their bits.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import special_values as sv
import spmm_cases as sc
import transposed as tr
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


# ------------------------------------------------------------------------------------------------------- 10. ragged rows
ONE = "csr_spmm_rows<%d>"


def k7(torch, rows, cols, rp, ci, val, X, ldx=None, ldy=None):
    """A X through K7 on a fresh handle over the CSR arrays, and the oracle's serial loop on every column."""
    k = X.shape[1]
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    Y = spmm(torch, A, X, k, ldx or k, ldy or k)
    A.close()
    with np.errstate(invalid="ignore", over="ignore"):
        return Y, oracle(rp, ci, val, X)


@pytest.mark.parametrize("g", sc.GROUPS)
def test_spmm_ragged_rows_every_remainder_of_the_batch(torch, g):
    """k = G vectors and 3 * (64 / G) + 1 rows -- three full wavefronts' worth and one row more -- whose lengths run through
    0 ... 17: every remainder of the batch of 8, rows that end inside the first, second and third batch, empty rows, a partial last
    wavefront; neighbouring groups of a wavefront make a different number of trips around the hand-round.  Twice, the second run
    of lengths starting at 9, so that every length occurs for every G (13 rows at G = 16)."""
    seen = set()
    for start in sc.RAGGED_STARTS:
        rows, cols, rp, ci, val, X = sc.ragged(g, start)
        seen |= set(np.diff(rp).tolist())
        A = sm.CsrMatrix(rows, cols, rp, ci, val)
        assert A.spmm_describe(g)[0] == ONE % g
        Y = spmm(torch, A, X, g, g + 1, g + 2)
        A.close()
        sc.assert_bits(Y, oracle(rp, ci, val, X), "G=%d rows=%d lengths from %d" % (g, rows, start))
    assert seen == set(range(18)) and {l % sc.BATCH for l in seen} == set(range(sc.BATCH))


def test_spmm_a_slot_past_a_rows_end_never_multiplies(torch):
    """The last batch of a row re-reads the row's last entry in its unused slots and must leave them out (if (j + u < z)).  Every
    value is positive and X is +Inf in the column of the last entry of every third row, in the last vector: such a row sums to
    +Inf, and a kernel that multiplied the unused slots by 0.0 would add 0 * Inf = NaN to it.  Lengths 1 ... 17: every number of
    unused slots."""
    rows, cols, rp, ci, val, last_col = sc.slot_case()
    assert {int(l) % sc.BATCH for l in np.diff(rp)[::3]} == set(range(sc.BATCH))
    for k in (1, 2, 4, 8, 16):
        X = sc.slot_operand(k, last_col)
        Y, ref = k7(torch, rows, cols, rp, ci, val, X, k + 1, k + 2)
        sc.assert_bits(Y, ref, "k = %d" % k)
        sc.assert_slot_rows(Y, "k = %d" % k)


# ----------------------------------------------------------------------------------------------------- 11. special values
@pytest.mark.parametrize("name", sv.SMALL)
def test_spmm_scenarios_a_to_d(torch, name):
    """A: NaN / Inf in columns of X that no entry uses change no bit of Y.  B: a NaN / Inf in vector v of a used column changes
    vector v only, and there the class of a row is the serial loop's.  C: a stored 0.0 under an Inf gives NaN.  D: rows of -0.0
    products, zero operands and empty rows give +0.0."""
    rows, cols, rp, ci, u = sv.structure(name)
    o = sv.ordinary(rows, cols, rp, ci, u)
    val = o["val"]
    sv.assert_regime(name, "A", rows, cols, rp, ci, val, o["x_a"], u)
    sv.assert_regime(name, "B", rows, cols, rp, ci, val, o["x_b"])
    sv.assert_regime(name, "C", rows, cols, rp, ci, val, o["x_c"])
    keys = ("x", "x_a", "x_b", "x", "x_c", "x_a", "x")            # 7 vectors: a pass of G = 8 with one idle lane per group
    X = np.stack([o[key] for key in keys], axis=1)
    Y, ref = k7(torch, rows, cols, rp, ci, val, X, 9, 8)
    sc.assert_bits(Y, ref, name + ", A ... C")
    clean = Y[:, 0]
    assert np.isfinite(clean).all()
    for c, key in enumerate(keys):
        if key in ("x", "x_a"):                                  # unused columns poisoned, or a neighbour vector poisoned: no bit changes
            tr.assert_bits(Y[:, c], clean, "%s: vector %d (%s) beside poisoned vectors" % (name, c, key))
        else:
            sv.check_classes(Y[:, c], sv.row_classes(rp, ci, val, o[key]), "%s: vector %d (%s)" % (name, c, key))
        sv.check_no_negative_zero(Y[:, c], "%s: vector %d" % (name, c))
    # the poisoned vector alone (k = 1) and in a pass of its own (vector 16 of 17)
    for key in ("x_a", "x_b", "x_c"):
        Y1, ref1 = k7(torch, rows, cols, rp, ci, val, o[key].reshape(-1, 1), 1, 1)
        sc.assert_bits(Y1, ref1, "%s, %s alone" % (name, key))
        X17 = np.repeat(o["x"].reshape(-1, 1), 17, axis=1)
        X17[:, 16] = o[key]
        Y17, ref17 = k7(torch, rows, cols, rp, ci, val, X17)
        sc.assert_bits(Y17, ref17, "%s, %s as vector 16 of 17" % (name, key))
        for c in range(16):
            tr.assert_bits(Y17[:, c], clean, "%s: vector %d of 17 beside %s" % (name, c, key))
    # D
    for z in (np.zeros(cols), -np.zeros(cols)):
        sv.assert_regime(name, "D", rows, cols, rp, ci, val, z)
        Z = np.stack([z, -z, z], axis=1)
        Yz, refz = k7(torch, rows, cols, rp, ci, val, Z, 3, 4)
        sc.assert_bits(Yz, refz, name + ", D")
        assert (Yz.view(np.int64) == 0).all(), "%s, D: something other than +0.0" % name


@pytest.mark.parametrize("name", sv.SMALL)
def test_spmm_scenarios_e_f_and_g(torch, name):
    """E: subnormal products and sums are kept.  F: sums of +-2^1020 overflow where the serial loop's do.  G: products that round
    -- a kernel that fuses the multiply into the add differs from the serial loop in most rows."""
    rows, cols, rp, ci, u = sv.structure(name)
    for scenario, (val, x) in (("E", sv.subnormal(rows, cols, rp, ci)), ("F", sv.overflowing(rows, cols, rp, ci)),
                               ("G", sv.rounded(rows, cols, rp, ci))):
        if scenario == "G":
            sv.assert_regime(name, "G", rows, cols, rp, ci, val, x)
        X = np.stack([x, -x, 0.5 * x, x, 2.0 * x if scenario != "F" else x], axis=1)     # (exact scalings: the bits follow the oracle's)
        Y, ref = k7(torch, rows, cols, rp, ci, val, X, 6, 5)
        if scenario == "E" and int(rp[-1]) >= 100:
            assert np.count_nonzero(ref[:, 0]) > 0 and np.abs(ref[:, 0]).max() < 2.0 ** -1022
        for c in range(X.shape[1]):
            sv.assert_exact(Y[:, c], ref[:, c], "%s, %s, vector %d" % (name, scenario, c))


# -------------------------------------------------------------------------------------- 12. row counts at the launch edges
def test_spmm_row_counts_at_the_launch_edges(torch):
    """Row counts around 256 / G (a workgroup), 8 * 256 / G (one round of workgroups over the XCDs) and 4096 (a sorted block) for
    every G: a wrong `group`, a truncated last round or a block left out of the plan leaves rows NaN at some count and not at
    others.  One fresh handle per count serves every k: its plan is built by the first call."""
    for rows in sc.ROW_COUNTS:
        n, cols, rp, ci, val, X = sc.row_count_case(rows)
        ref = oracle(rp, ci, val, X)
        A = sm.CsrMatrix(rows, cols, rp, ci, val)
        for k in sc.ROW_COUNT_KS:
            sc.assert_bits(spmm(torch, A, X, k, k + 1, k + 2), ref[:, :k], "%d rows, k = %d" % (rows, k))
        A.close()


# --------------------------------------------------------------------------------------------------------------- 13. fuzz
@pytest.mark.parametrize("seed", sc.FUZZ_SEEDS)
def test_spmm_fuzz_random_shapes_k_and_leading_dimensions(torch, seed):
    """Random shapes across up to four sorted blocks, every style of row lengths, k = 1 ... 40 and padded leading dimensions:
    the serial loop's bits on every column, and the same bits from a second call on the same handle (the plan built by the
    first)."""
    rows, cols, rp, ci, val, k, ldx, ldy, X = sc.block_fuzz(seed)
    what = "fuzz %d: %d x %d, k=%d ldx=%d ldy=%d" % (seed, rows, cols, k, ldx, ldy)
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    first = spmm(torch, A, X, k, ldx, ldy)
    second = spmm(torch, A, X, k, ldx, ldy)
    A.close()
    sc.assert_bits(first, oracle(rp, ci, val, X), what)
    sc.assert_bits(second, first, what + ", second call")


# ------------------------------------------------------------------------------------------ 14. offsets past 2^32 elements
def test_spmm_offsets_into_x_and_y_beyond_2_32_elements(torch):
    """(long long)c * ldx and (long long)r * ldy at or past 2^32 elements: 2^22 columns (then rows) with a leading dimension of
    1030 are 2^32 + 2^24.6 elements, 34.6 GB -- the smallest operand with such an offset -- so the operands take turns: first a
    wide X under a matrix of 100 rows, then, X freed, a tall Y over a matrix of 100 columns.  k = 3 as a slice of the wide
    array.  Offsets kept in 32 bits, signed or unsigned, read or write somewhere else."""
    n = 1 << 22
    k, ld = 3, 1030
    first_past = -(-2 ** 32 // ld)                                  # the first index whose offset no longer fits 32 bits
    assert first_past < n - 1000
    rng = np.random.default_rng(72)
    # X: 100 rows of about 50 entries; a tenth of the entries past 2^32 / ld, one in the last column
    rows, per_row = 100, 50
    lists = []
    for r in range(rows):
        c = np.concatenate([rng.integers(0, n, per_row - 5), rng.integers(first_past, n, 5)])
        lists.append(np.unique(np.append(c, n - 1) if r == rows - 1 else c))
    rp, ci, val = csr_of(rows, n, lists, rng)
    c64 = ci.astype(np.int64)
    assert 4500 < len(ci) <= 5100 and (c64 > 1 << 21).sum() > 2000 and (c64 * ld >= 2 ** 31).sum() > 2000
    assert (c64 * ld >= 2 ** 32).sum() > 300 and c64.max() == n - 1
    Xh = rng.standard_normal((n, k))
    ref = oracle(rp, ci, val, Xh)
    A = sm.CsrMatrix(rows, n, rp, ci, val)
    Xfull = torch.full((n, ld), float("nan"), dtype=torch.float64, device="cuda")
    Xfull[:, :k] = torch.from_numpy(Xh)
    buf, Y = guarded_Y(torch, rows, k, k + 2)
    A.spmm(Xfull[:, :k], Y)
    torch.cuda.synchronize()
    A.close()
    del Xfull
    torch.cuda.empty_cache()
    check_Y_guards(buf, rows, k, k + 2)
    sc.assert_bits(Y.cpu().numpy(), ref, "X of 2^22 x 1030")
    del buf, Y
    # Y: 2^22 rows of 100 columns; some 20 000 rows hold entries, half of them past 2^21, more than 50 past 2^32 / ld
    cols = 100
    used = np.unique(np.concatenate([rng.choice(n, 20000, replace=False), [0, n - 1, (1 << 21) - 1, 1 << 21]]))
    r = np.concatenate([used, rng.choice(used, 80000)])
    c = rng.integers(0, cols, len(r))
    rp, ci, val = sm.csr_from_coo(sm.make_coo(r, c, rng.uniform(-1, 1, len(r))), n)
    assert (used > 1 << 21).sum() > 5000 and (used.astype(np.int64) * ld >= 2 ** 32).sum() > 50
    assert set(np.flatnonzero(np.diff(rp)).tolist()) == set(used.tolist()) and rp[-1] == len(r)
    Xh = rng.standard_normal((cols, k))
    ref = oracle(rp, ci, val, Xh)
    A = sm.CsrMatrix(n, cols, rp, ci, val)
    dX = dev_X(torch, Xh, k + 1)
    buf = torch.empty(n * ld + 2 * G, dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(int(GUARD))
    Yfull = buf[G:G + n * ld].view(n, ld)
    Y = Yfull[:, :k]
    Y.fill_(float("nan"))
    A.spmm(dX, Y)
    torch.cuda.synchronize()
    bits = buf.view(torch.int64)
    assert bool((bits[:G] == int(GUARD)).all()) and bool((bits[-G:] == int(GUARD)).all()), "wrote outside Y"
    for c0 in range(k, ld, 128):                                     # (in slabs: a mask of the whole block would be 4 GB)
        assert bool((Yfull[:, c0:c0 + 128].view(torch.int64) == int(GUARD)).all()), "a padding column k <= v < ldy was written"
    got = Y.cpu().numpy()
    A.close()
    del buf, bits, Yfull, Y
    torch.cuda.empty_cache()
    sc.assert_bits(got[used], ref[used], "rows that hold entries")
    assert (np.delete(got, used, axis=0).view(np.int64) == 0).all(), "a row without entries is not +0.0"
    sc.assert_bits(got, ref, "every row")
