"""GPU: the diagonal of a handle (smvp_csr_diagonal / smvp_tjds_diagonal) and conjugate gradients with a diagonal preconditioner
(smvp_csr_pcg / smvp_tjds_pcg), kernel K14, against their numpy restatement tests/pcg_method.py (test_pcg_host.py pins that to
hand-computed values and known answers).

No tolerance anywhere.  A diagonal element is a sum in storage order from +0.0; the header fixes the order of every addition of the
dot, everything else -- the division r_i / m_i included -- is one rounded IEEE operation per element, and the restatement's product
argument is the SAME handle's single product (test_gpu_cg.handle): on every path whose product is the same from run to run, steps,
updates, reason, rr, rz, bb, the three histories and every bit of d_x have one right answer.  Comparisons are
transposed.assert_bits on the uint64 views.  Every solver call goes through solve() below, which gives d_x a guarded buffer, checks
the guards, checks that d_b and d_m come back unchanged and that the histories keep a sentinel beyond the filled elements."""
import ctypes as C
import functools

import numpy as np
import pytest

import cg_method as cg
import oracle_binding as ob
import pcg_method as pcg
import smvp_toolkit_amd as sm
import test_gpu_cg as k12
from conftest import SAMPLES
from parity import check_guards, guarded_y
from test_gpu_cg import AUTO, BOTH, PATHS, SENTINEL, dev, handle, start_vector
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

MAX_STEPS = 30
TOL = 1e-8


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of cg_method.py and pcg_method.py, built once and left unchanged; "scaled" is scaled(spd(n), 2)."""
    if name == "scaled":
        return pcg.scaled(cg.spd(*args), 2)
    return getattr(pcg if hasattr(pcg, name) else cg, name)(*args)


@functools.lru_cache(maxsize=None)
def jacobi(name, *args):
    """The restatement's diagonal of matrix(name, *args): computed once, shared, left unchanged."""
    return pcg.diagonal(matrix(name, *args))


def fn_of(H, what="pcg"):
    return "smvp_%s_%s" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds", what)


# =========================================================================================================== 1. the diagonal
@functools.lru_cache(maxsize=None)
def diagonal_case(i):
    """(Case, the restatement's diagonal): the cases of pcg_method.diag_cases(), then the five golden samples."""
    cases = pcg.diag_cases()
    if i < len(cases):
        M = cases[i]
    else:
        name = SAMPLES[i - len(cases)]
        tc, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
        M = pcg.Case(name, m, n, coo["row"], coo["col"], coo["val"])
    return M, pcg.diagonal(M)


def make(M, fmt):
    return sm.CsrMatrix(M.rows, M.cols, *M.csr) if fmt == "csr" else sm.TjdsMatrix(M.tjds)


def diagonal_of(torch, H, rows, stream=None):
    """One call into a guarded buffer poisoned with NaN: every element is written, nothing beside them."""
    buf, d = guarded_y(torch, rows)
    assert H.diagonal(d, stream=stream) is d
    torch.cuda.synchronize()
    check_guards(buf, rows)
    return d.cpu().numpy()


def products(torch, H, fmt, M, dx):
    """Two products of the handle (the tile kernel's sweep direction may alternate)."""
    out = []
    for _ in range(2):
        buf, dy = guarded_y(torch, M.rows)
        if fmt == "tjds":
            H.set_x(dx)
            H.zero_y(dy)
            H.spmv(dy)
        else:
            H.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, M.rows)
        out.append(dy.cpu().numpy())
    return out


@pytest.mark.parametrize("fmt", ["csr", "tjds"])
@pytest.mark.parametrize("i", range(len(pcg.diag_cases()) + len(SAMPLES)))
def test_the_diagonal_is_the_restatements_bits(torch, i, fmt):
    M, want = diagonal_case(i)
    H = make(M, fmt)
    got = diagonal_of(torch, H, M.rows)                                              # the first call on the handle: no plan, no set_x
    print("%s, %s: %d x %d, %d entries, %d elements not zero" % (M.name, fmt, M.rows, M.cols, M.nnz, np.count_nonzero(got)))
    assert_bits(got, want, "%s, %s" % (M.name, fmt))
    assert not np.signbit(got[got == 0.0]).any(), "a -0.0 in the diagonal"
    assert_bits(diagonal_of(torch, H, M.rows), got, "the same call again")
    assert_bits(diagonal_of(torch, H, M.rows, stream=torch.cuda.Stream()), got, "on a stream of the caller's")
    dx = dev(torch, np.random.default_rng(5).uniform(-1.0, 1.0, max(M.cols, 1)))[:M.cols]
    before = products(torch, H, fmt, M, dx)
    assert_bits(diagonal_of(torch, H, M.rows), got, "after products")
    for a, b in zip(products(torch, H, fmt, M, dx), before):                         # the handle's state is left alone
        assert_bits(a, b, "%s, %s: a product after the call" % (M.name, fmt))
    H.close()


def test_the_diagonal_of_a_row_block_lies_at_first_row_plus_r(torch):
    M = matrix("spd", 1003)
    row_ptr, col_ind, val = M.csr
    lo, hi = 100, 400
    block = (row_ptr[lo:hi + 1] - row_ptr[lo]).astype(np.int32)
    cols_, vals_ = col_ind[row_ptr[lo]:row_ptr[hi]], val[row_ptr[lo]:row_ptr[hi]]
    H = sm.CsrMatrix(hi - lo, M.n, block, cols_, vals_, first_row=lo)
    want = pcg.diagonal_csr(hi - lo, M.n, block, cols_, vals_, first_row=lo)
    assert_bits(want, jacobi("spd", 1003)[lo:hi], "the restatement: rows 100 .. 399 of the whole diagonal")
    assert_bits(diagonal_of(torch, H, hi - lo), want, "a row block with first_row = 100")
    H.close()
    H = sm.CsrMatrix(hi - lo, M.n, block, cols_, vals_)                              # the same arrays as a matrix of their own
    assert_bits(diagonal_of(torch, H, hi - lo), pcg.diagonal_csr(hi - lo, M.n, block, cols_, vals_), "first_row = 0")
    H.close()
    H = sm.CsrMatrix(hi - lo, M.n, block, cols_, vals_, first_row=M.n - 100)         # rows whose diagonal lies beyond the last column
    want = pcg.diagonal_csr(hi - lo, M.n, block, cols_, vals_, first_row=M.n - 100)
    assert (want[100:] == 0.0).all()
    assert_bits(diagonal_of(torch, H, hi - lo), want, "first_row + r >= cols reads +0.0")
    H.close()


@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_the_diagonal_is_captured_as_a_handles_first_call(torch, fmt):
    M, want = diagonal_case(1)
    H = make(M, fmt)
    buf, d = guarded_y(torch, M.rows)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc = getattr(sm.lib(), fn_of(H, "diagonal"))(H._h, sm._dev_ptr(d), s.cuda_stream)
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    d.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    check_guards(buf, M.rows)
    assert_bits(d.cpu().numpy(), want, "%s: the replayed capture" % fmt)
    del g
    H.close()


def adopted(torch, M, fmt):
    """(handle, the device tensor of its values): a handle over device arrays it adopts in place."""
    if fmt == "csr":
        rp, ci, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in M.csr)
        return sm.CsrMatrix(M.rows, M.cols, rp, ci, v), v
    t = sm.TjdsArrays()
    t.rows, t.cols, t.nnz, t.num_diag = M.tjds.rows, M.tjds.cols, M.tjds.nnz, M.tjds.num_diag
    pad = np.concatenate([M.tjds.start_pos[:t.num_diag + 1], [M.tjds.start_pos[t.num_diag]]]).astype(np.int32)
    t.perm = torch.from_numpy(np.ascontiguousarray(M.tjds.perm, dtype=np.int32)).cuda()
    t.start_pos = torch.from_numpy(pad).cuda()
    t.row_ind = torch.from_numpy(np.ascontiguousarray(M.tjds.row_ind, dtype=np.int32)).cuda()
    t.val = torch.from_numpy(np.ascontiguousarray(M.tjds.val, dtype=np.float64)).cuda()
    return sm.TjdsMatrix(t), t.val


@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_adopted_values_changed_in_place_are_seen(torch, fmt):
    M, want = diagonal_case(1)
    H, v = adopted(torch, M, fmt)
    assert_bits(diagonal_of(torch, H, M.rows), want, "%s: adopted arrays" % fmt)
    v.mul_(-3.0)                                                                     # exact for one entry; repeats are not in this case
    torch.cuda.synchronize()
    assert_bits(diagonal_of(torch, H, M.rows), want * -3.0 + 0.0, "%s: the values changed in place" % fmt)
    H.close()


def test_diagonal_refusals(torch):
    M, want = diagonal_case(1)
    A, T = make(M, "csr"), make(M, "tjds")
    for H in (A, T):
        assert getattr(sm.lib(), fn_of(H, "diagonal"))(H._h, None, None) == sm.ERR_INVALID
        assert b"null d_diag" in sm.lib().smvp_last_error()
        with pytest.raises(ValueError):
            H.diagonal(torch.zeros(M.rows + 1, dtype=torch.float64, device="cuda"))
        with pytest.raises(ValueError):
            H.diagonal(torch.zeros(M.rows, dtype=torch.float32, device="cuda"))
    d = torch.full((M.rows,), SENTINEL, dtype=torch.float64, device="cuda")
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_x(dev(torch, np.ones(M.cols)))
    T.spmv(torch.empty(M.rows, dtype=torch.float64, device="cuda"))                  # (the row-gather plan and its inner handle exist)
    inner = inner_csr_handle(T, M.rows, M.cols, M.nnz)                               # a CSR handle that is not plain CSR
    assert sm.lib().smvp_csr_diagonal(inner, sm._dev_ptr(d), None) == sm.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == SENTINEL).all()
    E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    ET = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    assert sm.lib().smvp_csr_diagonal(E._h, None, None) == sm.OK and sm.lib().smvp_tjds_diagonal(ET._h, None, None) == sm.OK
    for H in (A, T, E, ET):
        H.close()


# ======================================================================================================= 2. the solver's calls
def solve(torch, H, n, b, m, x0, max_steps, tol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, updates, reason, rr_each, rz_each, sigma_each, x, rr, rz, bb): pcg_method.run's tuple,
    then the result block's three doubles.  alias: d_x is d_x0.  Nothing is synchronised after the call: it returns when the work
    is done.
    before: called in place of the leading torch.cuda.synchronize() with the call's device vectors (stream_order.solver_hook puts
    them in flight on `stream`)."""
    buf, dx = guarded_y(torch, n)
    d0 = None
    if x0 is not None and alias:
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
        d0 = dx
    elif x0 is not None:
        d0 = dev(torch, x0)
    db, dm = dev(torch, b), dev(torch, m)
    o, r = sm.cg_opts(max_steps, tol, every), sm.PcgResult()
    rr, rz, sigma = np.full(max_steps + 1, SENTINEL), np.full(max_steps + 1, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0, m=dm)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx), sm._dev_ptr(dm), C.byref(r),
                                     sm._p(rr), sm._p(rz), sm._p(sigma), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    assert_bits(dm.cpu().numpy(), m, "d_m after the call")
    assert 0 <= r.updates <= r.steps <= max_steps and r.pad == 0
    for h, filled, name in ((rr, r.updates + 1, "rr_each"), (rz, r.updates + 1, "rz_each"), (sigma, r.steps, "sigma_each")):
        assert (h[filled:] == SENTINEL).all(), name + " was written beyond its filled elements"
        assert not (h[:filled] == SENTINEL).any(), "an element of %s was not filled" % name
    return (r.steps, r.updates, r.reason, rr[:r.updates + 1], rz[:r.updates + 1], sigma[:r.steps], x, np.float64(r.rr), np.float64(r.rz),
            np.float64(r.bb))


def same(got, want, what, b=None):
    """steps, updates, reason; the three histories and every bit of x; rr and rz of the last update, and bb where b is given."""
    assert tuple(got[:3]) == tuple(want[:3]), "%s: (steps, updates, reason) = %r, the restatement has %r" % (what, got[:3], want[:3])
    for i, name in ((3, "rr_each"), (4, "rz_each"), (5, "sigma_each"), (6, "d_x")):
        assert_bits(got[i], want[i], "%s: %s" % (what, name))
    if len(got) > 7:
        assert_bits([got[7], got[8]], [want[3][-1], want[4][-1]], what + ": rr, rz")
        if b is not None:
            assert_bits([got[9]], [cg.dot(b, b)], what + ": bb")


# ================================================================================================= 3. bits against run(), every path
SYSTEMS = (("scaled", (1003,)), ("spd_long", ()), ("spd_shuffled", ()))


@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name, args in SYSTEMS:
        M = matrix(name, *args)
        m = jacobi(name, *args)
        H, product = handle(torch, M, fmt, a, b)
        rhs, x0 = cg.rhs(M.n), start_vector(M.n)
        want = {None: pcg.run(product, rhs, None, m, MAX_STEPS, TOL), "x0": pcg.run(product, rhs, x0, m, MAX_STEPS, TOL)}
        for key, every, alias in ((None, 1, False), (None, 7, False), ("x0", 7, False), ("x0", 1000, True), ("x0", 1, True)):
            what = "%s, %s %d %d, x0 %s%s, check_every %d" % (name, fmt, a, b, key, ", d_x is d_x0" if alias else "", every)
            got = solve(torch, H, M.n, rhs, m, x0 if key else None, MAX_STEPS, TOL, every, alias=alias)
            same(got, want[key], what, rhs)
        w = want[None]
        print("%s, %s %d %d: steps %d, updates %d, reason %d, rr %r, rz %r" % (name, fmt, a, b, w[0], w[1], w[2], float(w[3][-1]), float(w[4][-1])))
        assert w[2] == pcg.CONVERGED and w[0] < MAX_STEPS, "%s: the restatement did not converge" % name
        same(solve(torch, H, M.n, rhs, m, None, 6, 0.0, 4), pcg.run(product, rhs, None, m, 6, 0.0), name + ", tol 0", rhs)
        H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_diagonal_kernel_feeds_the_solver(torch, fmt, a, b):
    """The whole use: diagonal() into a device vector, pcg() on it, through the Python methods."""
    M = matrix("scaled", 1003)
    H, product = handle(torch, M, fmt, a, b)
    rhs = cg.rhs(M.n)
    dm = H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda"))
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    r, rr, rz, sigma = H.pcg(dev(torch, rhs), dx, dm, max_steps=60, tol=TOL)
    want = pcg.run(product, rhs, None, jacobi("scaled", 1003), 60, TOL)
    assert (r.steps, r.updates, r.reason) == want[:3] and r.reason == sm.CG_CONVERGED and r.steps <= 30
    assert len(rr) == len(rz) == r.updates + 1 and len(sigma) == r.steps
    assert_bits(rr, want[3], "rr_each")
    assert_bits(rz, want[4], "rz_each")
    assert_bits(sigma, want[5], "sigma_each")
    assert_bits([r.rr, r.rz, r.bb], [want[3][-1], want[4][-1], cg.dot(rhs, rhs)], "the result block")
    assert_bits(dx.cpu().numpy(), want[6], "d_x")
    plain = H.cg(dev(torch, rhs), torch.empty_like(dx), max_steps=60, tol=TOL)[0]
    assert plain.reason == sm.CG_MAX_STEPS                                           # what the preconditioner is for
    with pytest.raises(ValueError):
        H.pcg(dev(torch, rhs), dx, dm.cpu())
    H.close()


# ====================================================================================== 4. m = ones is smvp_*_cg on the GPU, bit for bit
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_an_all_ones_preconditioner_is_the_librarys_cg(torch, fmt, a, b):
    for name, args in (("spd", (1003,)), ("spd_long", ()), ("spd_shuffled", ())):
        M = matrix(name, *args)
        H, product = handle(torch, M, fmt, a, b)
        rhs = cg.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            for tol in (0.0, 1e-10):
                plain = k12.solve(torch, H, M.n, rhs, x0, MAX_STEPS, tol)
                got = solve(torch, H, M.n, rhs, np.ones(M.n), x0, MAX_STEPS, tol)
                what = "%s, %s, x0 %s, tol %g" % (name, fmt, "NULL" if x0 is None else "random", tol)
                assert got[:3] == plain[:3], what
                assert_bits(got[3], plain[3], what + ": rr_each")
                assert_bits(got[4], plain[3], what + ": rz_each is rr_each")
                assert_bits(got[5], plain[4], what + ": sigma_each")
                assert_bits(got[6], plain[5], what + ": d_x")
                assert_bits([got[7], got[8], got[9]], [plain[6], plain[6], plain[7]], what + ": rr, rz, bb")
        H.close()


# ==================================================================================================================== 5. sizes
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_sizes_around_a_workgroup(torch, n):
    M = matrix("spd", n, 20280 + n)
    m = jacobi("spd", n, 20280 + n)
    rhs = cg.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            same(solve(torch, H, n, rhs, m, x0, 12, 1e-10, 5), pcg.run(product, rhs, x0, m, 12, 1e-10), "spd(%d), %s" % (n, fmt), rhs)
        H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_first_grid_trip(torch, fmt, a, b):
    M = matrix("tridiagonal", cg.TRIP + 1)
    m = jacobi("tridiagonal", cg.TRIP + 1)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = pcg.run(product, rhs, None, m, 4, 0.0)
    assert want[:3] == (4, 4, pcg.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, m, None, 4, 0.0, 3), want, "tridiagonal(%d), %s" % (M.n, fmt), rhs)
    assert_bits(diagonal_of(torch, H, M.n), m, "the diagonal kernel at this size")
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_unrolled_bodies(torch, fmt, a, b):
    """n = 4 * 2048 * 256 + 1: the smallest size at which the four-deep bodies of the passes that write run at all, followed by one
    tail trip of lane 0 of workgroup 0."""
    M = matrix("tridiagonal", 4 * cg.TRIP + 1)
    m = jacobi("tridiagonal", 4 * cg.TRIP + 1)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    want = pcg.run(product, rhs, None, m, 3, 0.0)
    assert want[:3] == (3, 3, pcg.MAX_STEPS)
    same(solve(torch, H, M.n, rhs, m, None, 3, 0.0, 2), want, "tridiagonal(%d), %s" % (M.n, fmt), rhs)
    H.close()


# ================================================================================================================ 6. the stop rules
def stop_cases():
    b5 = cg.rhs(300, 5)
    ones = np.ones(300)
    zero_in_m = ones.copy()
    zero_in_m[17] = 0.0
    yield "a zero in m", matrix("spd", 300), cg.rhs(300), zero_in_m, 1e-10, (0, 0, pcg.NONFINITE)
    yield "m = -ones", matrix("spd", 300), cg.rhs(300), -ones, 1e-10, (0, 0, pcg.BREAKDOWN)
    yield "minus_identity, m = ones", matrix("minus_identity", 300), b5, ones, 1e-10, (1, 0, pcg.BREAKDOWN)
    yield "rho turns negative", matrix("identity", 2), np.array([2.0, 1.0]), np.array([1.0, -1.0]), 1e-10, (1, 1, pcg.BREAKDOWN)
    yield "max_steps", matrix("spd", 300), cg.rhs(300), jacobi("spd", 300), 1e-300, (10, 10, pcg.MAX_STEPS)
    yield "zero b", matrix("spd", 300), np.zeros(300), jacobi("spd", 300), 1e-10, (0, 0, pcg.CONVERGED)
    yield "zero b, tol 0", matrix("spd", 300), np.zeros(300), jacobi("spd", 300), 0.0, (0, 0, pcg.CONVERGED)
    yield "a NaN matrix value", matrix("nan_value"), cg.rhs(300), ones, 1e-10, (1, 0, pcg.NONFINITE)
    inf = cg.rhs(300)
    inf[17] = np.inf
    yield "inf in b", matrix("spd", 300), inf, jacobi("spd", 300), 1e-10, (0, 0, pcg.NONFINITE)
    yield "bb overflows", matrix("spd", 300), np.full(300, 1e200), jacobi("spd", 300), 1e-10, (0, 0, pcg.NONFINITE)
    yield "identity, m = 1/2", matrix("identity", 300), b5, np.full(300, 0.5), 0.0, (1, 1, pcg.CONVERGED)


def test_the_stop_rules_on_the_device(torch):
    for name, M, rhs, m, tol, expect in stop_cases():
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = pcg.run(product, rhs, None, m, 10, tol)
            assert want[:3] == expect, "%s: the restatement gives %r" % (name, want[:3])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, m, None, 10, tol, every)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every))
                if name.startswith("identity"):
                    assert_bits(got[6], rhs, "identity: x is b")
            H.close()
    M, x0 = matrix("minus_identity", 2), np.array([0.25, -3.0])                      # rule A leaves the caller's start vector in d_x
    H, product = handle(torch, M, "csr", *AUTO)
    got = solve(torch, H, 2, np.array([1.0, 0.0]) + M.spmv(x0), np.ones(2), x0, 10, 1e-10, 5)
    assert got[:3] == (1, 0, pcg.BREAKDOWN)
    assert_bits(got[6], x0, "x_0 after a breakdown at step 1")
    H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    for H in (A, T):
        o, r = sm.cg_opts(5), sm.PcgResult()
        C.memset(C.byref(r), 0x5a, C.sizeof(r))
        b = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, sm._dev_ptr(b), C.byref(r), None, None, None,
                                           None) == sm.OK
        assert (r.steps, r.updates, r.reason, r.pad) == (0, 0, pcg.CONVERGED, 0)
        assert_bits([r.rr, r.rz, r.bb], [0.0, 0.0, 0.0], "n = 0")
        H.close()


# ==================================================================================================================== 7. operands
def test_operands(torch):
    M = matrix("spd_long")
    m = jacobi("spd_long")
    rhs, x0 = cg.rhs(M.n), start_vector(M.n)
    side = torch.cuda.Stream()
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = pcg.run(product, rhs, x0, m, MAX_STEPS, 1e-10)
        same(solve(torch, H, M.n, rhs, m, x0, MAX_STEPS, 1e-10), want, fmt + ", separate vectors", rhs)
        same(solve(torch, H, M.n, rhs, m, x0, MAX_STEPS, 1e-10, alias=True), want, fmt + ", d_x is d_x0", rhs)
        same(solve(torch, H, M.n, rhs, m, x0, MAX_STEPS, 1e-10, stream=side), want, fmt + ", a stream of the caller's", rhs)
        same(solve(torch, H, M.n, rhs, m, x0, MAX_STEPS, 1e-10), solve(torch, H, M.n, rhs, m, x0, MAX_STEPS, 1e-10)[:7], fmt + ", two runs")
        both = dev(torch, rhs)                                                       # d_m may be d_b: both are only read
        o, r = sm.cg_opts(MAX_STEPS, 1e-10, 10), sm.PcgResult()
        dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
        assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(both), None, sm._dev_ptr(dx), sm._dev_ptr(both), C.byref(r), None,
                                           None, None, None) == sm.OK                # (all three histories may be NULL)
        ref = pcg.run(product, rhs, None, rhs, MAX_STEPS, 1e-10)
        assert (r.steps, r.updates, r.reason) == ref[:3]
        assert_bits(dx.cpu().numpy(), ref[6], fmt + ": d_m is d_b")
        H.close()


# ====================================================================================================================== 8. refusals
def refused(torch, fn, h, n, o, result=True, b="own", x0=None, x="own", m="own"):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    dm = dev(torch, np.ones(max(n, 1))) if isinstance(m, str) else m
    r = sm.PcgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, rz, sigma = np.full(8, SENTINEL), np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), sm._dev_ptr(dm), C.byref(r) if result else None, sm._p(rr),
                               sm._p(rz), sm._p(sigma), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all(), \
        "%s wrote its outputs although it refused" % fn
    return rc


def test_invalid_arguments_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = matrix("spd", 63, 20280 + 63)
    m = jacobi("spd", 63, 20280 + 63)
    rhs = cg.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.cg_opts(5)
    n = M.n
    for fn, H, product, Wide in (("smvp_csr_pcg", A, pa, W), ("smvp_tjds_pcg", T, pt, WT)):
        assert refused(torch, fn, None, n, ok) == sm.ERR_INVALID
        for o in k12.bad_opts():
            assert refused(torch, fn, H._h, n, o) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, n, ok, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=None) == sm.ERR_INVALID             # no d_b
        assert refused(torch, fn, H._h, n, ok, m=None) == sm.ERR_INVALID             # no d_m
        assert refused(torch, fn, Wide._h, 4, ok) == sm.ERR_INVALID                  # rows != cols
        assert refused(torch, fn, H._h, n, ok, x=None) == sm.ERR_INVALID             # no d_x
        both = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")    # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, x0=both[:n], x=both[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, x0=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_b is d_x
        assert refused(torch, fn, H._h, n, ok, b=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_b and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, b=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, m=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_m is d_x
        assert refused(torch, fn, H._h, n, ok, m=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_m and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, m=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert (both.cpu().numpy() == SENTINEL).all()
        same(solve(torch, H, n, rhs, m, None, 5, 1e-10), pcg.run(product, rhs, None, m, 5, 1e-10), fn + ": the handle after the refusals", rhs)
    for H in (A, T, W, WT):
        H.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = matrix("spd", 1003)
    t = sm.tjds_from_coo(M.coo, M.n, M.n)
    T = sm.TjdsMatrix(t)
    ok = sm.cg_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_pcg", inner, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_pcg", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_pcg", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, cg.rhs(M.n), jacobi("spd", 1003), None, 2, 1e-10)[:3] == (2, 2, pcg.MAX_STEPS)
    T.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = matrix("spd", 63, 20280 + 63)
    m = jacobi("spd", 63, 20280 + 63)
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db, dm = dev(torch, rhs), dev(torch, m)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.cg_opts(5), sm.PcgResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, rz, sigma = np.full(6, SENTINEL), np.full(6, SENTINEL), np.full(5, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), sm._dev_ptr(dm), C.byref(r),
                                                   sm._p(rr), sm._p(rz), sm._p(sigma), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, m, None, 5, 1e-10, stream=s), pcg.run(product, rhs, None, m, 5, 1e-10),
         "outside a capture the same stream is fine")
    H.close()


# ========================================================================================================================= 9. state
def test_the_handles_state_afterwards(torch):
    M = matrix("spd_long")
    m = jacobi("spd_long")
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
        first = solve(torch, H, M.n, rhs, m, None, 7, 1e-10, 2)
        assert H.describe() == name
        for want in before:
            buf, dy = guarded_y(torch, M.n)
            if fmt == "tjds":
                H.set_x(dx)                                  # the permuted operand is the last direction's: a fresh set_x, as the header says
            H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dy.cpu().numpy(), want, "%s %d %d: a product after the call" % (fmt, a, b))
        same(solve(torch, H, M.n, rhs, m, None, 7, 1e-10, 2), first[:7], "%s %d %d: the same call again" % (fmt, a, b))
        H.close()
