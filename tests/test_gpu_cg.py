"""GPU: the order-defined dot product (smvp_vector_dot) and conjugate gradients on a handle (smvp_csr_cg / smvp_tjds_cg, kernel
K12) against their numpy restatement tests/cg_method.py (test_cg_host.py pins that to hand-computed values and known answers).

No tolerance anywhere.  The header fixes the order of every addition of the dot, everything else is one rounded IEEE operation per
element, and the restatement's product argument is the SAME handle's single product: on every path whose product is the same from
run to run -- every CSR family, TJDS ROW_GATHER and TWO_PHASE -- steps, updates, reason, rr, bb, both histories and every bit of
d_x have one right answer.  Comparisons are transposed.assert_bits on the uint64 views.  Every call goes through solve() below,
which gives d_x a guarded buffer, checks the guards, and checks that the histories keep a sentinel beyond the filled elements."""
import ctypes as C
import functools

import numpy as np
import pytest

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
MAX_STEPS = 30


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of cg_method.py, built once and left unchanged."""
    return getattr(cg, name)(*args)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def fn_of(H):
    return "smvp_csr_cg" if isinstance(H, sm.CsrMatrix) else "smvp_tjds_cg"


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
    """One call through the C ABI -> (steps, updates, reason, rr_each, sigma_each, x, rr, bb): cg_method.run's tuple, then the
    result block's two doubles.  alias: d_x is d_x0.  Nothing is synchronised after the call: it returns when the work is done.
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
    o, r = sm.cg_opts(max_steps, tol, every), sm.CgResult()
    rr, sigma = np.full(max_steps + 1, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx), C.byref(r), sm._p(rr),
                                     sm._p(sigma), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    assert 0 <= r.updates <= r.steps <= max_steps and r.pad == 0
    assert (rr[r.updates + 1:] == SENTINEL).all() and (sigma[r.steps:] == SENTINEL).all(), "a history was written beyond its filled elements"
    assert not (rr[:r.updates + 1] == SENTINEL).any() and not (sigma[:r.steps] == SENTINEL).any(), "a history element was not filled"
    return r.steps, r.updates, r.reason, rr[:r.updates + 1], sigma[:r.steps], x, np.float64(r.rr), np.float64(r.bb)


def same(got, want, what, b=None):
    """steps, updates, reason; both histories and every bit of x; rr = rho_updates, and bb where b is given."""
    assert tuple(got[:3]) == tuple(want[:3]), "%s: (steps, updates, reason) = %r, the restatement has %r" % (what, got[:3], want[:3])
    assert_bits(got[3], want[3], what + ": rr_each")
    assert_bits(got[4], want[4], what + ": sigma_each")
    assert_bits(got[5], want[5], what + ": d_x")
    if len(got) > 6:
        assert_bits([got[6]], [want[3][-1]], what + ": rr")
        if b is not None:
            assert_bits([got[7]], [cg.dot(b, b)], what + ": bb")


# ================================================================================================================== 1. the dot
DOT_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 1003, 65537, cg.TRIP - 1, cg.TRIP, cg.TRIP + 1, 2 * cg.TRIP + 5, 8 * cg.TRIP + 1]


def dot_operands(n):
    """Both signs over six decades, signed zeros among them."""
    rng = np.random.default_rng(20273 + n)
    a = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
    b = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
    a[rng.random(n) < 0.02] = 0.0
    b[rng.random(n) < 0.02] = -0.0
    return a, b


@pytest.mark.parametrize("n", DOT_SIZES)
def test_vector_dot_is_the_restatements_bits(torch, n):
    a, b = dot_operands(n)
    want = cg.dot(a, b)
    da, db = dev(torch, a), dev(torch, b)
    got = sm.vector_dot(da, db)
    print("n = %d: library %r, restatement %r, np.dot %r" % (n, float(got), float(want), float(np.dot(a, b))))
    assert_bits([got], [want], "smvp_vector_dot, n = %d" % n)
    assert_bits([sm.vector_dot(da, db)], [want], "the same call again")
    assert_bits([sm.vector_dot(da, da)], [cg.dot(a, a)], "a vector with itself")
    assert_bits([sm.vector_dot(da, db, stream=torch.cuda.Stream())], [want], "on a stream of the caller's")
    assert_bits(da.cpu().numpy(), a, "d_a after the calls")


def test_vector_dot_where_the_order_shows(torch):
    """test_cg_host.py's hand-computed cases: a serial sum gives 1.0 for the first, a pairwise one 1 + 2U for the second."""
    u = 2.0 ** -53
    a = np.full(256, u)
    a[0] = 1.0
    assert sm.vector_dot(dev(torch, a), dev(torch, np.ones(256))) == 1.0 + 254 * u
    c = np.zeros(cg.TRIP + 1)
    c[0], c[1], c[cg.TRIP] = 1.0, u, u
    assert sm.vector_dot(dev(torch, c), dev(torch, np.ones(len(c)))) == 1.0
    assert_bits([sm.vector_dot(dev(torch, np.full(300, -0.0)), dev(torch, np.ones(300)))], [0.0], "negative zero terms")
    assert np.isnan(sm.vector_dot(dev(torch, np.array([1.0, np.inf])), dev(torch, np.array([1.0, 0.0]))))


def test_vector_dot_refusals(torch):
    out = C.c_double(-7.0)
    v = torch.ones(8, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            v.add_(1.0)
            rc = sm.lib().smvp_vector_dot(0, 8, sm._dev_ptr(v), sm._dev_ptr(v), C.byref(out), s.cuda_stream)
            msg = sm.lib().smvp_last_error().decode()
    assert rc == sm.ERR_INVALID and "captur" in msg and out.value == -7.0
    g.replay()
    torch.cuda.synchronize()
    assert v.cpu().numpy().tolist() == [2.0] * 8
    del g
    assert sm.vector_dot(v, v, stream=s) == 32.0


# ================================================================================================= 2. bits against run(), every path
@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name, args in (("spd", (1003,)), ("spd_long", ()), ("spd_shuffled", ())):
        M = matrix(name, *args)
        H, product = handle(torch, M, fmt, a, b)
        rhs = cg.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            for tol in (0.0, 1e-10):
                what = "%s, %s %d %d, x0 %s, tol %g" % (name, fmt, a, b, "NULL" if x0 is None else "random", tol)
                want = cg.run(product, rhs, x0, MAX_STEPS, tol)
                got = solve(torch, H, M.n, rhs, x0, MAX_STEPS, tol)
                print("%s: steps %d, updates %d, reason %d, rr %r" % (what, got[0], got[1], got[2], float(got[6])))
                same(got, want, what, rhs)
                if tol:
                    assert want[2] == cg.CONVERGED and want[0] < MAX_STEPS, "%s: the restatement did not converge" % what
        H.close()


def test_the_python_method_returns_the_trimmed_histories(torch):
    M = matrix("spd", 1003)
    rhs = cg.rhs(M.n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = cg.run(product, rhs, None, 100, 1e-10)
        dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
        r, rr, sigma = H.cg(dev(torch, rhs), dx)
        assert (r.steps, r.updates, r.reason) == want[:3] and r.reason == sm.CG_CONVERGED
        assert len(rr) == r.updates + 1 and len(sigma) == r.steps
        assert_bits(rr, want[3], "rr_each")
        assert_bits(sigma, want[4], "sigma_each")
        assert_bits([r.rr, r.bb], [want[3][-1], cg.dot(rhs, rhs)], "the result block")
        assert_bits(dx.cpu().numpy(), want[5], "d_x")
        with pytest.raises(ValueError):
            H.cg(dev(torch, rhs).cpu(), dx)
        H.close()


# ===================================================================================================== 3. check_every changes nothing
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_nothing_depends_on_check_every(torch, fmt, a, b):
    M = matrix("spd", 1003)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = cg.run(product, rhs, None, MAX_STEPS, 1e-10)
    assert want[2] == cg.CONVERGED and want[0] < MAX_STEPS
    for every in (1, 4, 7, MAX_STEPS + 5):
        same(solve(torch, H, M.n, rhs, None, MAX_STEPS, 1e-10, every), want, "%s, check_every %d" % (fmt, every), rhs)
    x0 = start_vector(M.n)
    want = cg.run(product, rhs, x0, MAX_STEPS, 1e-10)
    for every in (1, 7, MAX_STEPS + 5):
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, every), want, "%s, a start vector, check_every %d" % (fmt, every), rhs)
    H.close()


# ============================================================================================================ 4. the grid's second trip
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_first_grid_trip(torch, fmt, a, b):
    M = matrix("spd", cg.TRIP + 1)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = cg.run(product, rhs, None, 6, 0.0)
    assert want[:3] == (6, 6, cg.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, None, 6, 0.0, 4), want, "spd(%d), %s" % (M.n, fmt), rhs)
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_unrolled_bodies(torch, fmt, a, b):
    """n = 4 * 2048 * 256 + 1: the smallest size at which the four-deep bodies of the passes that write run at all, followed by one
    tail trip of lane 0 of workgroup 0.  (The dot's eight-deep body is DOT_SIZES' last size.)"""
    M = matrix("spd", 4 * cg.TRIP + 1)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = cg.run(product, rhs, None, 3, 0.0)
    assert want[:3] == (3, 3, cg.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, None, 3, 0.0, 2), want, "spd(%d), %s" % (M.n, fmt), rhs)
    H.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wavefront_and_a_workgroup(torch, n):
    M = matrix("spd", n, 20280 + n)
    rhs = cg.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            same(solve(torch, H, n, rhs, x0, 12, 1e-10, 5), cg.run(product, rhs, x0, 12, 1e-10), "spd(%d), %s" % (n, fmt), rhs)
        H.close()


# ================================================================================================================ 5. the stop rules
def stop_cases():
    two = np.array([1.0, 0.0])
    b5 = cg.rhs(300, 5)
    yield "identity", matrix("identity", 300), b5, 0.0, (1, 1, cg.CONVERGED)
    yield "zero b", matrix("spd", 300), np.zeros(300), 1e-10, (0, 0, cg.CONVERGED)
    yield "zero b, tol 0", matrix("spd", 300), np.zeros(300), 0.0, (0, 0, cg.CONVERGED)
    yield "minus_identity", matrix("minus_identity", 2), two, 1e-10, (1, 0, cg.BREAKDOWN)
    yield "minus_identity(300)", matrix("minus_identity", 300), b5, 1e-10, (1, 0, cg.BREAKDOWN)
    yield "swap2", matrix("swap2"), two, 1e-10, (1, 0, cg.BREAKDOWN)
    inf = cg.rhs(300)
    inf[17] = np.inf
    yield "inf in b", matrix("spd", 300), inf, 1e-10, (0, 0, cg.NONFINITE)
    yield "bb overflows", matrix("spd", 300), np.full(300, 1e200), 1e-10, (0, 0, cg.NONFINITE)
    yield "a NaN matrix value", matrix("nan_value"), cg.rhs(300), 1e-10, (1, 0, cg.NONFINITE)
    yield "max_steps", matrix("spd", 300), cg.rhs(300), 1e-300, (10, 10, cg.MAX_STEPS)


def test_the_stop_rules_on_the_device(torch):
    for name, M, rhs, tol, expect in stop_cases():
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = cg.run(product, rhs, None, 10, tol)
            assert want[:3] == expect, "%s: the restatement gives %r" % (name, want[:3])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, None, 10, tol, every)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every))
                if name == "identity":
                    assert_bits(got[5], rhs, "identity: x is b")
                    assert got[3][1] == 0.0
            H.close()
    M, x0 = matrix("swap2"), np.array([0.25, -3.0])                           # a breakdown leaves the caller's start vector in d_x
    H, product = handle(torch, M, "csr", *AUTO)
    got = solve(torch, H, 2, np.array([1.0, 0.0]) + M.spmv(x0), x0, 10, 1e-10, 5)
    assert got[:3] == (1, 0, cg.BREAKDOWN)
    assert_bits(got[5], x0, "x_0 after a breakdown at step 1")
    H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    for H in (A, T):
        o, r = sm.cg_opts(5), sm.CgResult()
        C.memset(C.byref(r), 0x5a, C.sizeof(r))
        b = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, C.byref(r), None, None, None) == sm.OK
        assert (r.steps, r.updates, r.reason) == (0, 0, cg.CONVERGED)
        assert_bits([r.rr, r.bb], [0.0, 0.0], "n = 0")
        H.close()


# ==================================================================================================================== 6. operands
def test_operands(torch):
    M = matrix("spd_long")
    rhs, x0 = cg.rhs(M.n), start_vector(M.n)
    side = torch.cuda.Stream()
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = cg.run(product, rhs, x0, MAX_STEPS, 1e-10)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10), want, fmt + ", separate vectors", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, alias=True), want, fmt + ", d_x is d_x0", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10, stream=side), want, fmt + ", a stream of the caller's", rhs)
        same(solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10), solve(torch, H, M.n, rhs, x0, MAX_STEPS, 1e-10)[:6], fmt + ", two runs")
        H.close()


# ====================================================================================================================== 7. refusals
def refused(torch, fn, h, n, o, result=True, b="own", x0=None, x="own"):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    r = sm.CgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, sigma = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), C.byref(r) if result else None, sm._p(rr), sm._p(sigma), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (sigma == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def bad_opts():
    def o(**kw):
        v = sm.cg_opts(5)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    return [None, o(struct_size=20), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf"))]


def test_invalid_arguments_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = matrix("spd", 63, 20280 + 63)
    rhs = cg.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.cg_opts(5)
    n = M.n
    for fn, H, product, Wide in (("smvp_csr_cg", A, pa, W), ("smvp_tjds_cg", T, pt, WT)):
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
        same(solve(torch, H, n, rhs, None, 5, 1e-10), cg.run(product, rhs, None, 5, 1e-10), fn + ": the handle after the refusals", rhs)
    for H in (A, T, W, WT):
        H.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = matrix("spd", 1003)
    t = sm.tjds_from_coo(M.coo, M.n, M.n)
    T = sm.TjdsMatrix(t)
    ok = sm.cg_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_cg", inner, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_cg", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_cg", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, cg.rhs(M.n), None, 5, 1e-10)[:3] == (5, 5, cg.MAX_STEPS)
    T.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = matrix("spd", 63, 20280 + 63)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, rhs)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.cg_opts(5), sm.CgResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, sigma = np.full(6, SENTINEL), np.full(5, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), C.byref(r), sm._p(rr),
                                                   sm._p(sigma), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (sigma == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, None, 5, 1e-10, stream=s), cg.run(product, rhs, None, 5, 1e-10), "outside a capture the same stream is fine")
    H.close()


# ========================================================================================================================= 8. state
def test_the_handles_state_afterwards(torch):
    M = matrix("spd_long")
    rhs = cg.rhs(M.n)
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
                H.set_x(dx)                                  # the permuted operand is the last direction's: a fresh set_x, as the header says
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dy.cpu().numpy(), want, "%s %d %d: a product after the call" % (fmt, a, b))
        same(solve(torch, H, M.n, rhs, None, 7, 1e-10, 2), first[:6], "%s %d %d: the same call again" % (fmt, a, b))
        H.close()
