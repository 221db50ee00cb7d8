"""GPU: BiCGSTAB on a handle (smvp_csr_bicgstab / smvp_tjds_bicgstab, kernel K13) against its numpy restatement
tests/bicgstab_method.py (test_bicgstab_host.py pins that to exact small cases and to the true residual).

No tolerance anywhere.  The header fixes the order of every addition of the dot, everything else is one rounded IEEE operation per
element, and the restatement's product argument is the SAME handle's single product: on every path whose product is the same from
run to run -- every CSR family, TJDS ROW_GATHER and TWO_PHASE -- steps, full, half, reason, rr, bb, both histories and every bit of
d_x have one right answer.  Comparisons are transposed.assert_bits on the uint64 views.  Every call goes through solve() below,
which gives d_x a guarded buffer, checks the guards, checks that d_b is unchanged, and checks that each history is filled exactly up
to its count and keeps a sentinel beyond."""
import ctypes as C
import functools

import numpy as np
import pytest

import bicgstab_method as bi
import cg_method as cg
import smvp_toolkit_amd as sm
from parity import check_guards, guarded_y
from test_gpu_parity import CSR_VARIANTS
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

AUTO = (sm.CSR_KERNEL_AUTO, 0)
PATHS = [("csr",) + kp for kp in [AUTO] + CSR_VARIANTS] + [("tjds", sm.TJDS_MODE_ROW_GATHER, 0), ("tjds", sm.TJDS_MODE_TWO_PHASE, 0)]
BOTH = [("csr",) + AUTO, ("tjds", sm.TJDS_MODE_ROW_GATHER, 0)]
SENTINEL = -12345.678
MAX_STEPS = 40
LARGE = (("nonsym", (1003,)), ("nonsym_long", ()), ("nonsym_shuffled", ()))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of bicgstab_method.py, built once and left unchanged."""
    M = getattr(bi, name)(*args)
    return M[0] if isinstance(M, tuple) else M


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def fn_of(H):
    return "smvp_csr_bicgstab" if isinstance(H, sm.CsrMatrix) else "smvp_tjds_bicgstab"


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, n)


# ----------------------------------------------------------------------------------- a handle and its single product, numpy to numpy
def handle(torch, M, fmt, a, b):
    """(handle, product): a CsrMatrix on kernel a / param b, or a TjdsMatrix in mode a; product(x) is one product of that handle,
    remembered by operand (the restatement asks for the same products again with every tol)."""
    if fmt == "csr":
        H = sm.CsrMatrix(M.n, M.n, *M.csr)
        if (a, b) != AUTO:
            H.set_kernel(a, b)
    else:
        H = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
        H.set_mode(a)
    seen = {}

    def product(x):
        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
        if key not in seen:
            dx = dev(torch, x)
            buf, dy = guarded_y(torch, M.n)
            if fmt == "csr":
                H.spmv(dx, dy)
            else:
                H.set_x(dx)
                H.zero_y(dy)
                H.spmv(dy)
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            seen[key] = dy.cpu().numpy()
        return seen[key].copy()

    return H, product


def solve(torch, H, n, b, x0, max_steps, tol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, full, half, reason, rr_each, ss_each, x, rr, bb): bicgstab_method.run's tuple, then the
    result block's two doubles.  alias: d_x is d_x0.  Nothing is synchronised after the call: it returns when the work is done.
    ss_each is filled for `steps` steps, or one fewer where rule A ended the run (then full = steps - 1 and half = 0): its count is
    read off the sentinel, and same() holds it to the restatement's.
    before: called in place of the leading torch.cuda.synchronize() with the call's device vectors (stream_order.solver_hook puts
    them in flight on `stream`)."""
    buf, dx = guarded_y(torch, n)
    d0 = None
    if x0 is not None and alias:
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
        d0 = dx
    elif x0 is not None:
        d0 = dev(torch, x0)
    db = dev(torch, b)
    o, r = sm.bicgstab_opts(max_steps, tol, every), sm.BicgstabResult()
    rr, ss = np.full(max_steps + 1, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx), C.byref(r), sm._p(rr),
                                     sm._p(ss), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    assert 0 <= r.full <= r.steps <= max_steps and r.steps - r.full in (0, 1) and r.half in (0, 1)
    assert not (r.half and r.full == r.steps), "a half update on top of the step's full one"
    assert (rr[r.full + 1:] == SENTINEL).all(), "rr_each was written beyond its filled elements"
    assert not (rr[:r.full + 1] == SENTINEL).any(), "an element of rr_each was not filled"
    nss = r.steps
    if r.steps > r.full and not r.half and ss[r.steps - 1] == SENTINEL:       # rule A: the last step has no ss
        nss -= 1
    assert (ss[nss:] == SENTINEL).all(), "ss_each was written beyond its filled elements"
    assert not (ss[:nss] == SENTINEL).any(), "an element of ss_each was not filled"
    return r.steps, r.full, r.half, r.reason, rr[:r.full + 1], ss[:nss], x, np.float64(r.rr), np.float64(r.bb)


def same(got, want, what, b=None):
    """steps, full, half, reason; both histories (their lengths too) and every bit of x; rr = ss of the last step after a half
    update, else rr_full; bb where b is given."""
    assert tuple(got[:4]) == tuple(want[:4]), "%s: (steps, full, half, reason) = %r, the restatement has %r" % (what, got[:4], want[:4])
    assert_bits(got[4], want[4], what + ": rr_each")
    assert_bits(got[5], want[5], what + ": ss_each")
    assert_bits(got[6], want[6], what + ": d_x")
    if len(got) > 7:
        assert_bits([got[7]], [want[5][-1] if want[2] else want[4][-1]], what + ": rr")
        if b is not None:
            assert_bits([got[8]], [bi.dot(b, b)], what + ": bb")


# ================================================================================================= 1. bits against run(), every path
@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name, args in LARGE:
        M = matrix(name, *args)
        H, product = handle(torch, M, fmt, a, b)
        rhs = bi.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            for tol in (0.0, 1e-10):
                what = "%s, %s %d %d, x0 %s, tol %g" % (name, fmt, a, b, "NULL" if x0 is None else "random", tol)
                want = bi.run(product, rhs, x0, MAX_STEPS, tol)
                got = solve(torch, H, M.n, rhs, x0, MAX_STEPS, tol)
                print("%s: steps %d, full %d, half %d, reason %d, rr %r" % (what, got[0], got[1], got[2], got[3], float(got[7])))
                same(got, want, what, rhs)
                if tol:
                    assert want[3] == bi.CONVERGED and want[0] < MAX_STEPS, "%s: the restatement did not converge" % what
        H.close()


def test_the_python_method_returns_the_trimmed_histories(torch):
    M = matrix("nonsym", 1003)
    rhs = bi.rhs(M.n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = bi.run(product, rhs, None, 100, 1e-10)
        dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
        r, rr, ss = H.bicgstab(dev(torch, rhs), dx)
        assert (r.steps, r.full, r.half, r.reason) == want[:4] and r.reason == sm.BICGSTAB_CONVERGED
        assert len(rr) == r.full + 1 and len(ss) == r.steps
        assert_bits(rr, want[4], "rr_each")
        assert_bits(ss, want[5], "ss_each")
        assert_bits([r.rr, r.bb], [want[5][-1] if r.half else want[4][-1], bi.dot(rhs, rhs)], "the result block")
        assert_bits(dx.cpu().numpy(), want[6], "d_x")
        with pytest.raises(ValueError):
            H.bicgstab(dev(torch, rhs).cpu(), dx)
        H.close()
    S = matrix("swap2")                                                               # rule A at step 1: no ss, and the method knows
    H = sm.CsrMatrix(2, 2, *S.csr)
    dx = torch.empty(2, dtype=torch.float64, device="cuda")
    r, rr, ss = H.bicgstab(dev(torch, [1.0, 0.0]), dx)
    assert (r.steps, r.full, r.half, r.reason) == (1, 0, 0, sm.BICGSTAB_BREAKDOWN) and len(rr) == 1 and len(ss) == 0
    H.close()
    E = matrix("identity", 5)                                                         # rule H at step 1: ss_1 = +0.0 is an element
    H = sm.CsrMatrix(5, 5, *E.csr)
    dx = torch.empty(5, dtype=torch.float64, device="cuda")
    r, rr, ss = H.bicgstab(dev(torch, bi.rhs(5)), dx)
    assert (r.steps, r.full, r.half, r.reason) == (1, 0, 1, sm.BICGSTAB_CONVERGED) and len(rr) == 1
    assert_bits(ss, [0.0], "ss_each")
    H.close()


# ===================================================================================================== 2. check_every changes nothing
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_nothing_depends_on_check_every(torch, fmt, a, b):
    M = matrix("nonsym", 1003)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    for x0 in (None, start_vector(M.n)):
        want = bi.run(product, rhs, x0, MAX_STEPS, 1e-10)
        assert want[3] == bi.CONVERGED and want[0] < MAX_STEPS
        for every in (1, 4, 7, MAX_STEPS + 5):
            same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, every), want,
                 "%s, x0 %s, check_every %d" % (fmt, "NULL" if x0 is None else "random", every), rhs)
    H.close()


# ============================================================================================================ 3. the grid's second trip
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_first_grid_trip(torch, fmt, a, b):
    """n = 2048 * 256 + 1: the last element is the second trip of lane 0 of workgroup 0 alone -- where the two-accumulator pass and
    the fused passes could drop the tail."""
    M = matrix("nonsym", bi.TRIP + 1)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = bi.run(product, rhs, None, 4, 0.0)
    assert want[:4] == (4, 4, 0, bi.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, None, 4, 0.0, 3), want, "nonsym(%d), %s" % (M.n, fmt), rhs)
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_unrolled_bodies(torch, fmt, a, b):
    """n = 8 * 2048 * 256 + 1: the smallest size at which the eight-deep body of the two-accumulator pass runs at all (the four-deep
    bodies of the passes that write run twice), followed by one tail trip of lane 0 of workgroup 0."""
    M = matrix("banded", 8 * bi.TRIP + 1)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = bi.run(product, rhs, None, 2, 0.0)
    assert want[:4] == (2, 2, 0, bi.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, None, 2, 0.0, 2), want, "banded(%d), %s" % (M.n, fmt), rhs)
    H.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wavefront_and_a_workgroup(torch, n):
    M = matrix("nonsym", n, 20300 + n)
    rhs = bi.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            same(solve(torch, H, n, rhs, x0, 20, 1e-10, 5), bi.run(product, rhs, x0, 20, 1e-10), "nonsym(%d), %s" % (n, fmt), rhs)
        H.close()


# ================================================================================================================ 4. the stop rules
def stop_cases():
    """(name, matrix, b, tol, (steps, full, half, reason), x or None): x is what d_x must hold where the case fixes it."""
    two = np.array([1.0, 0.0])
    b5 = bi.rhs(300, 5)
    yield "identity", matrix("identity", 300), b5, 0.0, (1, 0, 1, bi.CONVERGED), b5
    yield "minus_identity", matrix("minus_identity", 300), b5, 1e-10, (1, 0, 1, bi.CONVERGED), -b5
    yield "swap2 (rule A)", matrix("swap2"), two, 1e-10, (1, 0, 0, bi.BREAKDOWN), np.zeros(2)
    yield "rule T", matrix("rule_t"), bi.rule_t()[1], 1e-10, (1, 0, 1, bi.BREAKDOWN), np.array([-1.0, 0.0, 0.0])
    yield "rule B", matrix("rule_b"), bi.rule_b()[1], 1e-10, (1, 1, 0, bi.BREAKDOWN), np.array([-0.5, -0.5, 0.0])
    yield "a NaN matrix value", matrix("nan_value"), bi.rhs(300), 1e-10, (1, 0, 0, bi.NONFINITE), np.zeros(300)
    inf = bi.rhs(300)
    inf[17] = np.inf
    yield "inf in b", matrix("nonsym", 300), inf, 1e-10, (0, 0, 0, bi.NONFINITE), np.zeros(300)
    yield "bb overflows", matrix("nonsym", 300), np.full(300, 1e200), 1e-10, (0, 0, 0, bi.NONFINITE), np.zeros(300)
    yield "zero b", matrix("nonsym", 300), np.zeros(300), 1e-10, (0, 0, 0, bi.CONVERGED), np.zeros(300)
    yield "zero b, tol 0", matrix("nonsym", 300), np.zeros(300), 0.0, (0, 0, 0, bi.CONVERGED), np.zeros(300)
    yield "max_steps", matrix("nonsym", 300), bi.rhs(300), 1e-300, (10, 10, 0, bi.MAX_STEPS), None


def test_the_stop_rules_on_the_device(torch):
    for name, M, rhs, tol, expect, x in stop_cases():
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = bi.run(product, rhs, None, 10, tol)
            assert want[:4] == expect, "%s: the restatement gives %r" % (name, want[:4])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, None, 10, tol, every)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every))
                if x is not None:
                    assert_bits(got[6], x, name + ": d_x")
            H.close()
    M, x0 = matrix("swap2"), np.array([0.25, -3.0])                           # a breakdown leaves the caller's start vector in d_x
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        got = solve(torch, H, 2, np.array([1.0, 0.0]) + M.spmv(x0), x0, 10, 1e-10, 5)
        assert got[:4] == (1, 0, 0, bi.BREAKDOWN) and len(got[5]) == 0
        assert_bits(got[6], x0, "x_0 after a rule A breakdown at step 1")
        H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    for H in (A, T):
        o, r = sm.bicgstab_opts(5), sm.BicgstabResult()
        C.memset(C.byref(r), 0x5a, C.sizeof(r))
        b = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, C.byref(r), None, None, None) == sm.OK
        assert (r.steps, r.full, r.half, r.reason) == (0, 0, 0, bi.CONVERGED)
        assert_bits([r.rr, r.bb], [0.0, 0.0], "n = 0")
        H.close()


# ==================================================================================================================== 5. operands
def test_operands(torch):
    M = matrix("nonsym_long")
    rhs, x0 = bi.rhs(M.n), start_vector(M.n)
    side = torch.cuda.Stream()
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = bi.run(product, rhs, x0, MAX_STEPS, 1e-10)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10), want, fmt + ", separate vectors", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, alias=True), want, fmt + ", d_x is d_x0", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, stream=side), want, fmt + ", a stream of the caller's", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10), solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10)[:7], fmt + ", two runs")
        H.close()


# ====================================================================================================================== 6. refusals
def refused(torch, fn, h, n, o, result=True, b="own", x0=None, x="own"):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    r = sm.BicgstabResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, ss = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), C.byref(r) if result else None, sm._p(rr), sm._p(ss), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (ss == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def bad_opts():
    def o(**kw):
        v = sm.bicgstab_opts(5)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    return [None, o(struct_size=20), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf"))]


def test_invalid_arguments_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = matrix("nonsym", 63, 20300 + 63)
    rhs = bi.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.bicgstab_opts(5)
    n = M.n
    for fn, H, product, Wide in (("smvp_csr_bicgstab", A, pa, W), ("smvp_tjds_bicgstab", T, pt, WT)):
        assert refused(torch, fn, None, n, ok) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, H._h, n, o) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, n, ok, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=None) == sm.ERR_INVALID             # no d_b
        assert refused(torch, fn, Wide._h, 4, ok) == sm.ERR_INVALID                  # rows != cols
        assert refused(torch, fn, H._h, n, ok, x=None) == sm.ERR_INVALID             # no d_x
        both = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")    # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, x0=both[:n], x=both[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, x0=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_b is d_x
        assert refused(torch, fn, H._h, n, ok, b=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_b and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, b=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert (both.cpu().numpy() == SENTINEL).all()
        same(solve(torch, H, n, rhs, None, 5, 1e-10), bi.run(product, rhs, None, 5, 1e-10), fn + ": the handle after the refusals", rhs)
    for H in (A, T, W, WT):
        H.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = matrix("nonsym", 1003)
    t = sm.tjds_from_coo(M.coo, M.n, M.n)
    T = sm.TjdsMatrix(t)
    ok = sm.bicgstab_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_bicgstab", inner, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_bicgstab", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_bicgstab", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, bi.rhs(M.n), None, 5, 1e-10)[:4] == (5, 5, 0, bi.MAX_STEPS)
    T.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = matrix("nonsym", 63, 20300 + 63)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, rhs)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.bicgstab_opts(5), sm.BicgstabResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, ss = np.full(6, SENTINEL), np.full(5, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), C.byref(r), sm._p(rr),
                                                   sm._p(ss), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (ss == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, None, 5, 1e-10, stream=s), bi.run(product, rhs, None, 5, 1e-10), "outside a capture the same stream is fine")
    H.close()


# ========================================================================================================================= 7. state
def test_the_handles_state_afterwards(torch):
    M = matrix("nonsym_long")
    rhs = bi.rhs(M.n)
    x = start_vector(M.n, 4)
    for fmt, a, b in PATHS:
        H, product = handle(torch, M, fmt, a, b)
        name = H.describe()
        dx = dev(torch, x)
        before = []
        for _ in range(2):                                   # (the tile kernel's sweep direction may alternate: two products)
            buf, dy = guarded_y(torch, M.n)
            if fmt == "tjds":
                H.set_x(dx)
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            before.append(dy.cpu().numpy())
        first = solve(torch, H, M.n, rhs, None, 7, 1e-10, 2)
        assert H.describe() == name
        for want in before:
            buf, dy = guarded_y(torch, M.n)
            if fmt == "tjds":
                H.set_x(dx)                                  # the permuted operand is the last vector's: a fresh set_x, as the header says
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dy.cpu().numpy(), want, "%s %d %d: a product after the call" % (fmt, a, b))
        same(solve(torch, H, M.n, rhs, None, 7, 1e-10, 2), first[:7], "%s %d %d: the same call again" % (fmt, a, b))
        H.close()


# ================================================================================================ 8. not conjugate gradients again
def test_conjugate_gradients_fail_where_bicgstab_converges(torch):
    """nonsym(1003) is not symmetric.  BiCGSTAB converges on it; conjugate gradients, given as many products as BiCGSTAB used (two
    a step), end as their own restatement says they do -- a breakdown, or max_steps with the residual still above the threshold.
    (The matrix is diagonally dominant with a positive diagonal, so its symmetric part is positive definite and conjugate gradients
    do not break down on it: they crawl.  On the CPU they need 36 products where BiCGSTAB needs 28.)"""
    M = matrix("nonsym", 1003)
    rhs = bi.rhs(M.n)
    thr = (np.float64(1e-10) * np.float64(1e-10)) * cg.dot(rhs, rhs)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
        r, rr, ss = H.bicgstab(dev(torch, rhs), dx, max_steps=MAX_STEPS, tol=1e-10)
        assert r.reason == sm.BICGSTAB_CONVERGED and r.steps < MAX_STEPS and r.rr <= thr
        products = 2 * r.steps - r.half
        want = cg.run(product, rhs, None, products, 1e-10)
        r, rr, sigma = H.cg(dev(torch, rhs), dx, max_steps=products, tol=1e-10)
        print("%s: after %d products cg ends with steps %d, updates %d, reason %d, rr %r (thr %r)" % (
            fmt, products, r.steps, r.updates, r.reason, r.rr, float(thr)))
        assert (r.steps, r.updates, r.reason) == want[:3]
        assert r.reason == sm.CG_BREAKDOWN or (r.reason == sm.CG_MAX_STEPS and r.rr > thr)
        H.close()
