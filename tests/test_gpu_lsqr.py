"""GPU: LSQR on a handle (smvp_csr_lsqr / smvp_tjds_lsqr, kernel K22) against its numpy restatement tests/lsqr_method.py
(test_lsqr_host.py pins that to hand-computed runs and to numpy.linalg.lstsq).

No tolerance anywhere.  The header fixes the order of every addition of the dot, the root is the correctly rounded one, everything
else is one rounded IEEE operation, and the restatement's two product arguments are the SAME handles' single products -- h's and
ht's for the CSR route, the forward and the transposed product of the one handle for TJDS: steps, updates, reason, the four norms,
both histories and every bit of d_x have one right answer.  Comparisons are transposed.assert_bits on the uint64 views.  Every call
goes through solve() below, which gives d_x a guarded buffer, checks the guards, checks that d_b is unchanged, and checks that each
history is filled exactly up to `updates` and keeps a sentinel beyond."""
import ctypes as C
import functools

import numpy as np
import pytest

import bicgstab_method as bi
import lsqr_method as lm
import smvp_toolkit_amd as sm
import stream_order as so
from parity import check_guards, guarded_y
from test_gpu_bicgstab import AUTO, BOTH, PATHS
from test_gpu_gmres import root_inputs
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
TRIP = lm.TRIP                                               # 2048 * 256: the elements of one trip of the full grid


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of lsqr_method.py, built once and left unchanged."""
    if name == "nonsym":
        return lm.of(bi.nonsym(*args))
    return getattr(lm, name)(*args)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, n)


# ------------------------------------------------------------------------ the handles of a route and their single products, numpy to numpy
class Route:
    """CSR: h on kernel a / param b and ht = h.transposed() on the same; TJDS: the one handle in mode a.  forward(x) and trans(u)
    are single products of those handles, remembered by operand (the restatement asks for the same products again)."""

    def __init__(self, torch, A, fmt, a, b, at=None):
        self.torch, self.fmt, self.m, self.n = torch, fmt, A.m, A.n
        if fmt == "csr":
            self.H = sm.CsrMatrix(A.m, A.n, *A.csr)
            self.HT = self.H.transposed() if A.nnz else sm.CsrMatrix(A.n, A.m, *A.transpose().csr)
            if (a, b) != AUTO:
                self.H.set_kernel(a, b)
            if (at or (a, b)) != AUTO:
                self.HT.set_kernel(*(at or (a, b)))
            self.fn, self.handles = "smvp_csr_lsqr", (self.H._h, self.HT._h)
        else:
            self.H, self.HT = sm.TjdsMatrix(sm.tjds_from_coo(A.coo, A.m, A.n)), None
            self.H.set_mode(a)
            self.fn, self.handles = "smvp_tjds_lsqr", (self.H._h,)
        self.seen = {}, {}

    def _product(self, which, x, rows):
        torch = self.torch
        key = np.ascontiguousarray(x, dtype=np.float64).tobytes()
        seen = self.seen[which]
        if key not in seen:
            dx = dev(torch, x)
            buf, dy = guarded_y(torch, rows)
            if self.fmt == "csr":
                (self.HT if which else self.H).spmv(dx, dy)
            elif which:
                self.H.spmv_transposed(dx, dy)
            else:
                self.H.set_x(dx)
                self.H.zero_y(dy)
                self.H.spmv(dy)
            torch.cuda.synchronize()
            check_guards(buf, rows)
            seen[key] = dy.cpu().numpy()
        return seen[key].copy()

    def forward(self, x):
        return self._product(0, x, self.m)

    def trans(self, u):
        return self._product(1, u, self.n)

    def close(self):
        for H in (self.HT, self.H):
            if H is not None:
                H.close()


def solve(torch, R, b, x0, max_steps, tol, atol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> lsqr_method.run's tuple.  alias: d_x is d_x0.  Nothing is synchronised after the call: it
    returns when the work is done.  before: called in place of the leading torch.cuda.synchronize() with the call's device vectors
    (stream_order.solver_hook puts them in flight on `stream`)."""
    buf, dx = guarded_y(torch, R.n)
    d0 = None
    if x0 is not None and alias:
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
        d0 = dx
    elif x0 is not None:
        d0 = dev(torch, x0)
    db = dev(torch, b)
    o, r = sm.lsqr_opts(max_steps, tol, atol, every), sm.LsqrResult()
    rn, arn = np.full(max_steps + 1, SENTINEL), np.full(max_steps + 1, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0)
    rc = getattr(sm.lib(), R.fn)(*R.handles, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx), C.byref(r), sm._p(rn),
                                 sm._p(arn), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, R.n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    assert 0 <= r.updates <= r.steps <= max_steps and r.steps - r.updates in (0, 1)
    for each, name in ((rn, "rnorm_each"), (arn, "arnorm_each")):
        assert (each[r.updates + 1:] == SENTINEL).all(), "%s was written beyond its filled elements" % name
        assert not (each[:r.updates + 1] == SENTINEL).any(), "an element of %s was not filled" % name
    return r.steps, r.updates, r.reason, rn[:r.updates + 1], arn[:r.updates + 1], x, (r.rnorm, r.arnorm, r.anorm, r.bnorm)


def restated(R, b, x0, max_steps, tol, atol):
    return lm.run(R.forward, R.trans, b, x0, max_steps, tol, atol)


def same(got, want, what):
    """steps, updates, reason; both histories (their lengths too), every bit of x and the result block's four norms."""
    assert tuple(got[:3]) == tuple(want[:3]), "%s: (steps, updates, reason) = %r, the restatement has %r" % (what, got[:3], want[:3])
    assert_bits(got[3], want[3], what + ": rnorm_each")
    assert_bits(got[4], want[4], what + ": arnorm_each")
    assert_bits(got[5], want[5], what + ": d_x")
    assert_bits(got[6], want[6], what + ": rnorm, arnorm, anorm, bnorm")
    assert_bits(got[6][:2], [want[3][-1], want[4][-1]], what + ": the result holds the last history elements")


def both(torch, R, b, x0, max_steps, tol, atol, what, every=10, **kw):
    want = restated(R, b, x0, max_steps, tol, atol)
    got = solve(torch, R, b, x0, max_steps, tol, atol, every, **kw)
    same(got, want, what)
    return got


# ==================================================================================================================== 1. the root
def test_the_root_is_the_correctly_rounded_one(torch):
    """One step of LSQR on the identity of 1, 2 or 3 rows at tol = atol = 0: bnorm = sqrt(dot(b, b)) is the root of the argument
    (held to smvp_vector_dot of b with itself), beta_1 the same root again, alpha_1, rho and anorm further ones, and bnorm, both
    histories, x and the result are the restatement's -- whose roots are numpy.sqrt's -- bit for bit."""
    routes = {n: Route(torch, lm.Rect(n, n, np.arange(n), np.arange(n), np.ones(n)), "csr", *AUTO) for n in (1, 2, 3)}
    for n, R in routes.items():                                                       # both products of these handles are the identity
        v = np.array([1.5, -2.25, 3.0][:n])
        assert_bits(R.forward(v), v, "the identity's product")
        assert_bits(R.trans(v), v, "its transpose's")
    count, roots = 0, set()
    for b in root_inputs():
        b = np.array(b, dtype=np.float64)
        R = routes[len(b)]
        want = lm.run(lambda v: v.copy(), lambda v: v.copy(), b, None, 1, 0.0, 0.0)
        arg = lm.dot(b, b)
        assert np.isfinite(arg) and arg > 0.0, "the argument %r is no argument" % arg
        db, dx = dev(torch, b), torch.empty(len(b), dtype=torch.float64, device="cuda")
        o, r = sm.lsqr_opts(1, 0.0, 0.0, 1), sm.LsqrResult()
        rn, arn = np.full(2, SENTINEL), np.full(2, SENTINEL)
        assert sm.lib().smvp_csr_lsqr(*R.handles, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), C.byref(r), sm._p(rn), sm._p(arn),
                                      None) == sm.OK
        what = "b = %r (dot(b, b) = %r, its root %r)" % (b.tolist(), float(arg), float(np.sqrt(arg)))
        assert_bits([sm.vector_dot(db, db)], [arg], what + ": smvp_vector_dot")
        assert_bits([r.bnorm], [np.sqrt(arg)], what + ": bnorm")
        got = (r.steps, r.updates, r.reason, rn[:r.updates + 1], arn[:r.updates + 1], dx.cpu().numpy(), (r.rnorm, r.arnorm, r.anorm, r.bnorm))
        same(got, want, what)
        count += 1
        roots.add(float(arg))
    print("%d runs, %d different arguments of the first root" % (count, len(roots)))
    assert count > 2500 and len(roots) > 2500
    for R in routes.values():
        R.close()


# ================================================================================================================ 2. every path
@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    """h and ht on the same plan family (TJDS: the mode and K8): a tall inconsistent system to its LEAST_SQUARES end, a wide one to
    CONVERGED, and 1003 x 517 -- more than one workgroup in both loops, odd sizes -- from an x0."""
    for name, args, x0, want_reason in (("tall", (257, 131), None, lm.LEAST_SQUARES), ("wide", (131, 257), None, lm.CONVERGED),
                                        ("tall", (1003, 517), start_vector(517), lm.LEAST_SQUARES)):
        A = matrix(name, *args)
        R = Route(torch, A, fmt, a, b)
        got = both(torch, R, lm.rhs(A.m), x0, 60, 1e-10, 1e-10, "%s%r, %s %d %d" % (name, args, fmt, a, b), every=7)
        assert got[2] == want_reason and got[0] > 5
        R.close()


def test_h_and_ht_on_different_plans(torch):
    A = matrix("tall", 1003, 517)
    for plan_h, plan_t in (((sm.CSR_KERNEL_VECTOR, 4), (sm.CSR_KERNEL_COLSWEEP, 0)), ((sm.CSR_KERNEL_BINNED, 3), (sm.CSR_KERNEL_STREAM, 256))):
        R = Route(torch, A, "csr", *plan_h, at=plan_t)
        kernels = R.H.get_kernel(), R.HT.get_kernel()
        both(torch, R, lm.rhs(1003), None, 12, 0.0, 0.0, "h on %r, ht on %r" % (plan_h, plan_t), every=5)
        assert (R.H.get_kernel(), R.HT.get_kernel()) == kernels, "a plan was changed"
        R.close()


# ================================================================================================================== 3. the shapes
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_smallest_shapes(torch, fmt, a, b):
    cases = (("1 x 1", lm.dense_rect([[2.0]]), [6.0]), ("1 x 5", lm.dense_rect([[1.0, -2.0, 0.5, 3.0, 0.25]]), [1.75]),
             ("5 x 1", lm.dense_rect([[1.0], [-2.0], [0.5], [3.0], [0.25]]), [1.0, 0.5, -0.25, 2.0, 3.0]),
             ("2 x 2 diagonal", lm.dense_rect([[2.0, 0.0], [0.0, 2.0]]), [3.0, 4.0]))
    for name, A, rhs in cases:
        R = Route(torch, A, fmt, a, b)
        for x0 in (None, start_vector(A.n)):
            both(torch, R, np.array(rhs), x0, 10, 1e-12, 1e-12, "%s, %s" % (name, fmt), every=2)
        R.close()
    # the hand-computed runs of test_lsqr_host.py, on the device: these products are exact
    R = Route(torch, cases[0][1], fmt, a, b)
    got = solve(torch, R, np.array([6.0]), None, 10, 0.0, 0.0)
    assert got[:3] == (1, 1, lm.CONVERGED)
    assert_bits(got[5], [3.0], "1 x 1: x")
    assert_bits(got[6], [0.0, 0.0, 2.0, 6.0], "1 x 1: the result")
    R.close()
    R = Route(torch, cases[3][1], fmt, a, b)                                            # a zero beta in mid-run: the step completes x
    got = solve(torch, R, np.array([3.0, 4.0]), None, 10, 0.0, 0.0)
    assert got[:3] == (1, 1, lm.CONVERGED)
    assert_bits(got[3], [5.0, 0.0], "diag(2, 2): rnorm_each")
    assert_bits(got[5], [1.5, 2.0], "diag(2, 2): x")
    R.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
@pytest.mark.parametrize("shape", ["tall", "wide"])
def test_one_element_past_the_first_grid_trip(torch, fmt, a, b, shape):
    """M = 2048 * 256 + 1 with N = 257, and the transpose's shape: the M-loop, then the N-loop, takes its second trip for one
    element, the unrolled body never runs in the other loop, and the dots have lanes with two terms.  Five steps at tol = atol = 0;
    at most three entries a row."""
    A = matrix("tall", TRIP + 1, 257) if shape == "tall" else matrix("wide", 257, TRIP + 1, 20301, 2)
    assert int(np.diff(A.row_ptr).max()) <= 3
    R = Route(torch, A, fmt, a, b)
    got = both(torch, R, lm.rhs(A.m), start_vector(A.n) if shape == "wide" else None, 5, 0.0, 0.0, "%s %d x %d, %s" % (shape, A.m, A.n, fmt),
               every=2)
    assert got[:3] == (5, 5, lm.MAX_STEPS)
    R.close()


def test_matrices_without_rows_or_columns(torch):
    """M == 0 or N == 0: SMVP_OK, nothing done, every norm +0.0; with M == 0 < N d_x holds x_0."""
    for m, n in ((0, 0), (0, 4), (3, 0)):
        A = lm.Rect(m, n, [], [], [])
        for fmt, a, b in BOTH:
            R = Route(torch, A, fmt, a, b)
            for x0 in (None, start_vector(n)):
                got = solve(torch, R, np.ones(max(m, 1)), x0 if n else None, 5, 1e-10, 1e-10)    # (d_b may not be NULL)
                assert got[:3] == (0, 0, lm.CONVERGED)
                assert_bits(got[3], [0.0], "rnorm_each")
                assert_bits(got[4], [0.0], "arnorm_each")
                assert_bits(got[6], np.zeros(4), "%d x %d: the norms" % (m, n))
                assert_bits(got[5], np.zeros(n) if x0 is None else x0, "%d x %d: x = x_0" % (m, n))
            R.close()


# ============================================================================================================== 4. the behaviour
def all_the_same(torch, R, A, rhs, x0, max_steps, tol, atol, what):
    want = restated(R, rhs, x0, max_steps, tol, atol)
    for every in sorted({1, 3, 10, max_steps}):
        same(solve(torch, R, rhs, x0, max_steps, tol, atol, every), want, "%s, check_every %d" % (what, every))
    return want


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_nothing_depends_on_check_every(torch, fmt, a, b):
    """Stops at a looked step, between two looks and at max_steps, by each of the rules; the close of a step rides in the next
    step's pass U or is launched on its own at a look: the same bits."""
    A = matrix("tall", 1003, 517)
    R = Route(torch, A, fmt, a, b)
    rhs = lm.rhs(A.m)
    reasons = set()
    for x0, max_steps, tol, atol in ((None, 40, 1e-10, 1e-10), (start_vector(A.n), 40, 0.0, 1e-6), (None, 7, 0.0, 0.0), (None, 1, 0.0, 0.0),
                                     (None, 30, 0.0, 1e-3)):
        reasons.add(all_the_same(torch, R, A, rhs, x0, max_steps, tol, atol, "tall(1003, 517), %s, max_steps %d" % (fmt, max_steps))[2])
    consistent = R.forward(start_vector(A.n, 3))
    for max_steps, tol in ((40, 1e-10), (40, 1e-4), (12, 1e-9)):
        reasons.add(all_the_same(torch, R, A, consistent, None, max_steps, tol, 0.0, "consistent, %s, max_steps %d" % (fmt, max_steps))[2])
    assert reasons == {lm.CONVERGED, lm.LEAST_SQUARES, lm.MAX_STEPS}
    R.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_stop_rules_on_the_device(torch, fmt, a, b):
    """All four reasons; step 0's rules; NaN and Inf in b; rule N in mid-run, which leaves x at the last finite step."""
    A = matrix("tall", 257, 131)
    R = Route(torch, A, fmt, a, b)
    rhs = lm.rhs(A.m)
    x0 = start_vector(A.n)
    taken = set()
    for bad in (np.nan, np.inf, -np.inf):
        c = rhs.copy()
        c[100] = bad
        for start in (None, x0):
            got = both(torch, R, c, start, 10, 1e-10, 1e-10, "%r in b, %s" % (bad, fmt), every=3)
            assert got[:3] == (0, 0, lm.NONFINITE)
            assert_bits(got[5], np.zeros(A.n) if start is None else x0, "x stays x_0")
    assert both(torch, R, np.full(A.m, 1e200), None, 10, 1e-10, 1e-10, "the square overflows")[:3] == (0, 0, lm.NONFINITE)
    got = both(torch, R, np.zeros(A.m), None, 10, 0.0, 0.0, "b = 0")
    assert got[:3] == (0, 0, lm.CONVERGED)
    assert_bits(got[6], np.zeros(4), "b = 0: every norm +0.0")
    assert both(torch, R, rhs, None, 10, 1e30, 0.0, "a huge tol")[:3] == (0, 0, lm.CONVERGED)
    taken.add(both(torch, R, rhs, None, 1, 0.0, 0.0, "max_steps = 1")[2])
    taken.add(both(torch, R, rhs, None, 60, 1e-10, 1e-10, "to the end")[2])
    taken.add(both(torch, R, R.forward(x0), None, 60, 1e-10, 0.0, "consistent")[2])
    R.close()
    # b orthogonal to range(A): LEAST_SQUARES at step 0, x = x_0
    Z = Route(torch, lm.dense_rect([[1.0], [0.0]]), fmt, a, b)
    for rhs2, start, want in (([0.0, 5.0], None, 0.0), ([7.0, 5.0], [7.0], 7.0)):
        got = both(torch, Z, np.array(rhs2), None if start is None else np.array(start), 5, 0.0, 0.0, "b orthogonal to the range")
        assert got[:3] == (0, 0, lm.LEAST_SQUARES)
        assert_bits(got[5], [want], "x = x_0")
        assert_bits(got[6][:3], [5.0, 0.0, 0.0], "rnorm, arnorm, anorm")
    Z.close()
    # values of 5e153: A2 overflows in the third step (test_lsqr_host.py): rule N, x stays x_2
    T = matrix("tall", 40, 17)
    rows, cols, vals = (np.array(T.coo[f]) for f in ("row", "col", "val"))
    N = Route(torch, lm.Rect(40, 17, rows, cols, vals * 5e153), fmt, a, b)
    for every in (1, 2, 10):
        got = both(torch, N, lm.rhs(40), None, 10, 1e-10, 1e-10, "rule N in mid-run, check_every %d" % every, every=every)
        assert got[2] == lm.NONFINITE and got[1] == got[0] - 1 >= 1 and np.isfinite(got[5]).all()
    taken.add(got[2])
    N.close()
    assert taken == {lm.MAX_STEPS, lm.LEAST_SQUARES, lm.CONVERGED, lm.NONFINITE}


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_x_aliased_to_x0_and_the_rank_deficient_matrix(torch, fmt, a, b):
    A = matrix("rank_deficient", 257, 131)
    R = Route(torch, A, fmt, a, b)
    rhs, x0 = lm.rhs(A.m), start_vector(A.n)
    want = restated(R, rhs, x0, 60, 1e-10, 1e-10)
    assert want[2] == lm.LEAST_SQUARES
    same(solve(torch, R, rhs, x0, 60, 1e-10, 1e-10, 4, alias=True), want, "d_x is d_x0, %s" % fmt)
    same(solve(torch, R, rhs, x0, 60, 1e-10, 1e-10, 4), want, "d_x and d_x0 apart, %s" % fmt)
    R.close()


# ==================================================================================================== 5. streams, state, refusals
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_stream_of_the_callers_with_the_operands_still_in_flight(torch, fmt, a, b):
    A = matrix("tall", 1003, 517)
    R = Route(torch, A, fmt, a, b)
    rhs, x0 = lm.rhs(A.m), start_vector(A.n)
    side = torch.cuda.Stream()
    want = restated(R, rhs, x0, 60, 1e-10, 1e-10)
    seen = []
    got = solve(torch, R, rhs, x0, 60, 1e-10, 1e-10, 3, stream=side, before=so.solver_hook(torch, side, seen))
    assert seen and all(event.query() for event, _ in seen), "the call returned before the work on its stream had finished"
    same(got, want, "%s, everything in flight" % fmt)
    same(solve(torch, R, rhs, None, 9, 0.0, 0.0, 4, stream=side), restated(R, rhs, None, 9, 0.0, 0.0), fmt + ", a stream of the caller's")
    R.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    A = matrix("tall", 257, 131)
    R = Route(torch, A, fmt, a, b)
    rhs = lm.rhs(A.m)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((A.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, rhs)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.lsqr_opts(5), sm.LsqrResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rn, arn = np.full(6, SENTINEL), np.full(6, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), R.fn)(*R.handles, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), C.byref(r), sm._p(rn),
                                               sm._p(arn), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rn == SENTINEL).all() and (arn == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, R, rhs, None, 5, 1e-10, 1e-10, stream=s), restated(R, rhs, None, 5, 1e-10, 1e-10),
         "outside a capture the same stream is fine")
    R.close()


def test_the_state_of_the_handles_afterwards(torch):
    """Both CSR handles keep their plans and give their earlier bits; a TJDS handle gives its earlier bits after a fresh set_x, and
    its transposed product needs nothing."""
    A = matrix("tall", 1003, 517)
    rhs = lm.rhs(A.m)
    x, u = start_vector(A.n, 4), start_vector(A.m, 5)
    for fmt, a, b in PATHS:
        R = Route(torch, A, fmt, a, b)
        names = R.H.describe(), R.HT.describe() if R.HT else None
        dx, du = dev(torch, x), dev(torch, u)

        def look():
            out = []
            for _ in range(2):                               # (the tile kernel's sweep direction may alternate: two products)
                buf, dy = guarded_y(torch, A.m)
                if fmt == "tjds":
                    R.H.set_x(dx)                            # the permuted operand is the last vh's: a fresh set_x, as the header says
                R.H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
                buf_t, dt = guarded_y(torch, A.n)
                if fmt == "csr":
                    R.HT.spmv(du, dt)
                else:
                    R.H.spmv_transposed(du, dt)
                torch.cuda.synchronize()
                check_guards(buf, A.m)
                check_guards(buf_t, A.n)
                out += [dy.cpu().numpy(), dt.cpu().numpy()]
            return out

        before = look()
        first = solve(torch, R, rhs, None, 7, 0.0, 0.0, 2)
        assert (R.H.describe(), R.HT.describe() if R.HT else None) == names
        for got, want in zip(look(), before):
            assert_bits(got, want, "%s %d %d: a product after the call" % (fmt, a, b))
        same(solve(torch, R, rhs, None, 7, 0.0, 0.0, 2), first, "%s %d %d: the same call again" % (fmt, a, b))
        R.close()


def refused(torch, fn, handles, n, o, result=True, b="own", x0=None, x="own", m=1):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(m, 1))) if isinstance(b, str) else b
    r = sm.LsqrResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rn, arn = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(*handles, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), C.byref(r) if result else None, sm._p(rn), sm._p(arn), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rn == SENTINEL).all() and (arn == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def bad_opts():
    def o(**kw):
        v = sm.lsqr_opts(5)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    return [None, o(struct_size=24), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf")), o(atol=-1e-300), o(atol=float("nan")), o(atol=float("inf"))]


def test_invalid_arguments_a_mismatched_ht_and_overlaps_are_refused_and_nothing_is_written(torch):
    A = matrix("tall", 63, 40)
    rhs = lm.rhs(63)
    Rc, Rt = Route(torch, A, "csr", *AUTO), Route(torch, A, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    ok = sm.lsqr_opts(5)
    m, n = A.m, A.n
    for R in (Rc, Rt):
        fn, hs = R.fn, R.handles
        assert refused(torch, fn, (None,) + hs[1:], n, ok, m=m) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, hs, n, o, m=m) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, hs, n, ok, result=False, m=m) == sm.ERR_INVALID
        assert refused(torch, fn, hs, n, ok, b=None, m=m) == sm.ERR_INVALID           # no d_b
        assert refused(torch, fn, hs, n, ok, x=None, m=m) == sm.ERR_INVALID           # no d_x
        both_ = torch.full((m + n + 1,), SENTINEL, dtype=torch.float64, device="cuda")   # d_x0 and d_x one element apart
        assert refused(torch, fn, hs, n, ok, x0=both_[:n], x=both_[1:n + 1], m=m) == sm.ERR_INVALID
        assert refused(torch, fn, hs, n, ok, x0=both_[1:n + 1], x=both_[:n], m=m) == sm.ERR_INVALID
        assert refused(torch, fn, hs, n, ok, b=both_[:m], x=both_[:n], m=m) == sm.ERR_INVALID      # d_x inside d_b
        assert refused(torch, fn, hs, n, ok, b=both_[n - 1:n - 1 + m], x=both_[:n], m=m) == sm.ERR_INVALID     # one element shared
        assert b"d_b and d_x overlap" in sm.lib().smvp_last_error()
        assert (both_.cpu().numpy() == SENTINEL).all()
    # ht: missing, the wrong shape (h itself, and the transpose of a narrower matrix), the wrong number of entries
    assert refused(torch, Rc.fn, (Rc.H._h, None), n, ok, m=m) == sm.ERR_INVALID
    assert refused(torch, Rc.fn, (Rc.H._h, Rc.H._h), n, ok, m=m) == sm.ERR_INVALID
    assert b"the transpose of h" in sm.lib().smvp_last_error()
    narrow = Route(torch, matrix("tall", 63, 39), "csr", *AUTO)
    assert refused(torch, Rc.fn, (Rc.H._h, narrow.HT._h), n, ok, m=m) == sm.ERR_INVALID
    rows, cols, vals = (np.array(A.coo[f]) for f in ("row", "col", "val"))
    fewer = Route(torch, lm.Rect(63, 40, rows[:-1], cols[:-1], vals[:-1]), "csr", *AUTO)
    assert refused(torch, Rc.fn, (Rc.H._h, fewer.HT._h), n, ok, m=m) == sm.ERR_INVALID
    assert b"entries" in sm.lib().smvp_last_error()
    for R in (Rc, Rt):
        same(solve(torch, R, rhs, None, 5, 1e-10, 1e-10), restated(R, rhs, None, 5, 1e-10, 1e-10), R.fn + ": the handles after the refusals")
    for R in (Rc, Rt, narrow, fewer):
        R.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    A = matrix("tall", 1003, 517)
    R = Route(torch, A, "csr", *AUTO)
    T = sm.TjdsMatrix(sm.tjds_from_coo(A.coo, A.m, A.n))
    ok = sm.lsqr_opts(5)
    inner = inner_csr_handle(T, A.m, A.n, A.nnz)                                      # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_lsqr", (inner, R.HT._h), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    TT = sm.TjdsMatrix(sm.tjds_from_coo(A.transpose().coo, A.n, A.m))
    assert refused(torch, "smvp_csr_lsqr", (R.H._h, inner_csr_handle(TT, A.n, A.m, A.nnz)), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    block = sm.CsrMatrix(A.m, A.n, *A.csr, first_row=3)                               # a row block of a taller matrix
    assert refused(torch, "smvp_csr_lsqr", (block._h, R.HT._h), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    assert b"row block" in sm.lib().smvp_last_error()
    block_t = sm.CsrMatrix(A.n, A.m, *A.transpose().csr, first_row=3)
    assert refused(torch, "smvp_csr_lsqr", (R.H._h, block_t._h), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_lsqr", (T._h,), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_lsqr", (T._h,), A.n, ok, m=A.m) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    for H in (block, block_t, TT, T):
        H.close()
    assert solve(torch, R, lm.rhs(A.m), None, 2, 0.0, 0.0)[:3] == (2, 2, lm.MAX_STEPS)
    R.close()


# ===================================================================================== 6. library against library, the Python methods
def two_a_row(n, seed=20303):
    """n x n, not symmetric: a diagonal in [1, 2] and one small entry a row at a random other column.  A row's two products add up
    to the same bits in either order, so every forward product agrees; a column may hold many entries."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    j = (i + rng.integers(1, n, n)) % n
    return lm.Rect(n, n, np.concatenate([i, i]), np.concatenate([i, j]), np.concatenate([rng.uniform(1.0, 2.0, n), rng.uniform(-0.3, 0.3, n)]))


def test_the_tjds_route_and_the_csr_route_agree_where_their_products_do(torch):
    """A square matrix from one COO list, at = transposed(): wherever every product the two routes ran has the same bits, so has
    everything LSQR returns.  With two entries a row every forward product has one right answer, and K8 sums a column in the
    serial order, which is the column sweep's on ht: those pairs of plans must agree, so the check is not empty."""
    A = two_a_row(257)
    rhs = lm.rhs(257)
    T = Route(torch, A, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    want_t = restated(T, rhs, None, 60, 1e-10, 1e-10)
    got_t = solve(torch, T, rhs, None, 60, 1e-10, 1e-10, 7)
    same(got_t, want_t, "tjds")
    assert got_t[0] > 5
    sweep = (sm.CSR_KERNEL_COLSWEEP, 0)
    agreed = []
    for plan, at in ((AUTO, sweep), (sweep, sweep), ((sm.CSR_KERNEL_VECTOR, 2), sweep), (AUTO, AUTO), ((sm.CSR_KERNEL_BINNED, 3), (sm.CSR_KERNEL_VECTOR, 8))):
        R = Route(torch, A, "csr", *plan, at=at)
        got = solve(torch, R, rhs, None, 60, 1e-10, 1e-10, 7)
        same(got, restated(R, rhs, None, 60, 1e-10, 1e-10), "csr %r, ht %r" % (plan, at))
        products = all(R.seen[w].keys() == T.seen[w].keys() and all((R.seen[w][k].view(np.int64) == T.seen[w][k].view(np.int64)).all()
                                                                    for k in R.seen[w]) for w in (0, 1))
        if products:
            same(got, got_t, "csr %r, ht %r against tjds" % (plan, at))
            agreed.append((plan, at))
        R.close()
    print("the routes' products agreed on %r" % agreed)
    assert (sweep, sweep) in agreed
    T.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_whole_use_through_the_python_methods(torch, fmt, a, b):
    A, rhs = lm.named("tall(257, 131), inconsistent")
    R = Route(torch, A, fmt, a, b)
    db = dev(torch, rhs)
    dx = torch.empty(A.n, dtype=torch.float64, device="cuda")
    want = restated(R, rhs, None, 100, 1e-10, 1e-10)
    kw = dict(at=R.HT) if fmt == "csr" else {}
    for extra in (kw, {}):                                                            # at given; at = None builds and closes its own
        dx.fill_(SENTINEL)
        r, rn, arn = R.H.lsqr(db, dx, check_every=4, **extra)
        assert (r.steps, r.updates, r.reason) == want[:3] and r.reason == sm.LSQR_LEAST_SQUARES
        assert_bits(rn, want[3], "rnorm_each")
        assert_bits(arn, want[4], "arnorm_each")
        assert_bits([r.rnorm, r.arnorm, r.anorm, r.bnorm], want[6], "the result block")
        assert_bits(dx.cpu().numpy(), want[5], "d_x")
    x0 = dev(torch, start_vector(A.n))
    r, rn, arn = R.H.lsqr(db, x0, x0=x0, max_steps=300, tol=1e-12, atol=1e-12, check_every=1000, stream=torch.cuda.Stream(), **kw)
    want = restated(R, rhs, start_vector(A.n), 300, 1e-12, 1e-12)
    assert (r.steps, r.updates, r.reason) == want[:3]
    assert_bits(x0.cpu().numpy(), want[5], "x0 given and aliased")
    best = np.linalg.lstsq(A.dense(), rhs, rcond=None)[0]
    assert np.linalg.norm(x0.cpu().numpy() - best) <= 1e-9 * np.linalg.norm(best)
    with pytest.raises(ValueError):
        R.H.lsqr(db.cpu(), dx, **kw)
    if fmt == "csr":
        with pytest.raises(ValueError):
            R.H.lsqr(db, dx, at=R.HT._h)
        with pytest.raises(sm.SmvpError):
            R.H.lsqr(db, dx, at=R.H)                                                  # h is no transpose of itself: 257 x 131
    with pytest.raises(sm.SmvpError):
        R.H.lsqr(db, dx, max_steps=0, **kw)
    R.close()
