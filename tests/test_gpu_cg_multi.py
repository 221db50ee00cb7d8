"""GPU: conjugate gradients for k right-hand sides on a handle (smvp_csr_cg_multi / smvp_tjds_cg_multi, kernel K20) against the
restatement tests/cg_multi_method.py: cg_method.run / pcg_method.run per column around the oracle's serial loop per column
(test_cg_multi_host.py pins that on the CPU).

No tolerance anywhere.  The header defines column v of every output as the one-vector run on column v of the operands, with the
block product's column -- the serial loop, whatever the handle's plan or mode -- as q: steps, updates, reason, the result block,
the three histories and every bit of X have one right answer.  Comparisons are transposed.assert_bits on the uint64 views.  Every
call goes through solve() below, which gives X (and, wide, B and X0) a guarded buffer whose padding columns hold a sentinel, checks
guards and padding, and hands back the flat histories whole: same() holds them to the restatement's filled elements AND to the
sentinel everywhere else."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import cg_method as cg
import cg_multi_method as cm
import pcg_method as pcg
import power_iteration as pi
import smvp_toolkit_amd as sm
import stream_order as so
from parity import G, GUARD, check_guards, guarded_y
from test_gpu_parity import CSR_VARIANTS
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

AUTO = (sm.CSR_KERNEL_AUTO, 0)
MAIN = [("csr",) + AUTO, ("tjds", sm.TJDS_MODE_ROW_GATHER, 0), ("tjds", sm.TJDS_MODE_TWO_PHASE, 0), ("tjds", sm.TJDS_MODE_ATOMIC, 0)]
BOTH = MAIN[:2]
KS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 33)           # every group width, an idle remainder, passes of 16 + 16 + 1
KMAX = max(KS)
SENTINEL = -12345.678
MAX_STEPS, TOL = 30, 1e-10
MATRICES = (("spd", (1003,)), ("spd_long", ()), ("spd_shuffled", ()))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "smvp-toolkit_amd")
COUNTED = os.path.join(PKG, "lib", "libsmvp_amd_counted.so")
LIMIT_S = 240


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def matrix(name, *args):
    """The matrices of cg_method.py, built once and left unchanged."""
    return getattr(cg, name)(*args)


@functools.lru_cache(maxsize=None)
def rhs_block(n, k=KMAX):
    return np.random.default_rng(20300 + n).uniform(-1.0, 1.0, (n, k))


@functools.lru_cache(maxsize=None)
def start_block(n, k=KMAX):
    return np.random.default_rng(20301 + n).uniform(-2.0, 2.0, (n, k))


@functools.lru_cache(maxsize=None)
def jacobi(name, *args):
    return pcg.diagonal(matrix(name, *args))


@functools.lru_cache(maxsize=None)
def restated(name, args, fmt, with_m, with_x0, k=KMAX, max_steps=MAX_STEPS, tol=TOL):
    """The restatement's runs of the first k columns of rhs_block / start_block on a cg_method matrix: computed once, shared by
    every test that needs them, and left unchanged.  Column v's run depends on nothing but column v."""
    M = matrix(name, *args)
    return cm.run(cm.product_of(M, fmt), rhs_block(M.n)[:, :k], start_block(M.n)[:, :k] if with_x0 else None,
                  jacobi(name, *args) if with_m else None, max_steps, tol)


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def fn_of(H):
    return "smvp_csr_cg_multi" if isinstance(H, sm.CsrMatrix) else "smvp_tjds_cg_multi"


def handle(M, fmt, a, b):
    """A CsrMatrix on kernel a / param b, or a TjdsMatrix in mode a."""
    if fmt == "csr":
        H = sm.CsrMatrix(M.n, M.n, *M.csr)
        if (a, b) != AUTO:
            H.set_kernel(a, b)
        return H
    H = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    H.set_mode(a)
    return H


# ----------------------------------------------------------------------------------------------------------- guarded operands
def guarded_block(torch, n, k, ld, off, fill=float("nan")):
    """(buffer, V): V = columns off .. off + k - 1 of an n x ld row-major block inside buffer, holding `fill`; the padding columns
    and G doubles on either side hold GUARD."""
    buf = torch.empty(n * ld + 2 * G, dtype=torch.float64, device="cuda")
    buf.view(torch.int64).fill_(int(GUARD))
    V = buf[G:G + n * ld].view(n, ld)[:, off:off + k]
    V.fill_(fill)
    return buf, V


def check_block_guards(buf, n, k, ld, off, what):
    check_guards(buf, n * ld)
    h = buf.cpu().numpy().view(np.int64)[G:G + n * ld].reshape(n, ld)
    assert (h[:, :off] == GUARD).all() and (h[:, off + k:] == GUARD).all(), "a padding column of %s was written" % what


class Got:
    """What one call handed back: results (k PcgResult), the flat histories whole, X on the host."""


def solve(torch, H, B, X0=None, m=None, max_steps=MAX_STEPS, tol=TOL, every=10, stream=None, alias=False, wide=False, before=None):
    """One call through the C ABI.  wide: X, B and X0 are column slices of arrays 3, 4 and 5 columns wider, each with a leading
    dimension and an offset of its own; else ld = k.  alias: d_X is d_X0.  Nothing is synchronised after the call: it returns when
    the work is done.  before: called in place of the leading torch.cuda.synchronize() with the call's device operands
    (stream_order.solver_hook puts them in flight on `stream`)."""
    n, k = B.shape
    (ldx, offx), (ldb, offb), (ld0, off0) = ((k + 3, 1), (k + 4, 2), (k + 5, 3)) if wide else ((k, 0),) * 3
    bufx, dX = guarded_block(torch, n, k, ldx, offx)
    buf0 = d0 = None
    if X0 is not None and alias:
        dX.copy_(torch.from_numpy(np.ascontiguousarray(X0, dtype=np.float64)))
        d0 = dX
    elif X0 is not None:
        buf0, d0 = guarded_block(torch, n, k, ld0, off0)
        d0.copy_(torch.from_numpy(np.ascontiguousarray(X0, dtype=np.float64)))
    bufb, dB = guarded_block(torch, n, k, ldb, offb)
    dB.copy_(torch.from_numpy(np.ascontiguousarray(B, dtype=np.float64)))
    dm = dev(torch, m) if m is not None else None
    o, r = sm.cg_opts(max_steps, tol, every), (sm.PcgResult * k)()
    C.memset(r, 0x5a, C.sizeof(r))
    g = Got()
    g.max_steps, g.k = max_steps, k
    g.rr, g.rz, g.sigma = np.full(k * (max_steps + 1), SENTINEL), np.full(k * (max_steps + 1), SENTINEL), np.full(k * max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dX, b=dB, x0=None if alias else d0, m=dm)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), k, sm._dev_ptr(dB), ldb, sm._dev_ptr(d0), ldx if alias else ld0, sm._dev_ptr(dX), ldx,
                                     sm._dev_ptr(dm), r, sm._p(g.rr), sm._p(g.rz), sm._p(g.sigma), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    g.X = dX.cpu().numpy()
    check_block_guards(bufx, n, k, ldx, offx, "X")
    check_block_guards(bufb, n, k, ldb, offb, "B")
    assert_bits(dB.cpu().numpy().ravel(), np.asarray(B).ravel(), "d_B after the call")
    if buf0 is not None:
        check_block_guards(buf0, n, k, ld0, off0, "X0")
        assert_bits(d0.cpu().numpy().ravel(), np.asarray(X0).ravel(), "d_X0 after the call")
    if dm is not None:
        assert_bits(dm.cpu().numpy(), m, "d_m after the call")
    g.results = list(r)
    for v, b in enumerate(g.results):
        assert 0 <= b.updates <= b.steps <= max_steps and b.pad == 0, "column %d: steps %d, updates %d, pad %d" % (v, b.steps, b.updates, b.pad)
    return g


def same(got, want, what, B=None, with_m=False):
    """Every column's steps, updates and reason; the three flat histories whole -- the restatement's filled elements and the
    sentinel beyond them, all of rz_each the sentinel without an m --; every bit of X; the result blocks."""
    assert len(want) == got.k
    outcome = [(b.steps, b.updates, b.reason) for b in got.results]
    assert outcome == cm.outcomes(want), "%s: (steps, updates, reason) = %r, the restatement has %r" % (what, outcome, cm.outcomes(want))
    rr, rz, sigma = cm.flat_histories(want, got.max_steps, SENTINEL)
    assert_bits(got.rr, rr, what + ": rr_each")
    assert_bits(got.rz, rz if with_m else np.full(len(rz), SENTINEL), what + ": rz_each")
    assert_bits(got.sigma, sigma, what + ": sigma_each")
    assert_bits(got.X.ravel(), cm.solution(want).ravel(), what + ": d_X")
    for v, b in enumerate(got.results):
        assert_bits([b.rr, b.rz], [want[v][3][-1], want[v][4][-1]], "%s: rr and rz of column %d" % (what, v))
        if B is not None:
            assert_bits([b.bb], [cg.dot(B[:, v], B[:, v])], "%s: bb of column %d" % (what, v))


def column(got, v):
    """Everything the call said about column v, the sentinel tails of its histories included."""
    s, b = got.max_steps, got.results[v]
    return ((b.steps, b.updates, b.reason), np.array([b.rr, b.rz, b.bb]), got.rr[v * (s + 1):(v + 1) * (s + 1)],
            got.rz[v * (s + 1):(v + 1) * (s + 1)], got.sigma[v * s:(v + 1) * s], got.X[:, v])


def same_column(a, b, what):
    assert a[0] == b[0], "%s: (steps, updates, reason) %r against %r" % (what, a[0], b[0])
    for x, y, name in zip(a[1:], b[1:], ("the result block", "rr_each", "rz_each", "sigma_each", "X")):
        assert_bits(x, y, "%s: %s" % (what, name))


# ============================================================================================================ 1. restatement parity
# (m, X0, alias, wide): plain and Jacobi; without an X0, with one, with X aliasing it; ld = k and column slices of wider arrays
COMBOS = [(with_m, x0, wide) for with_m in (False, True) for x0 in ("none", "own", "alias") for wide in (False, True)]


def run_combo(torch, H, name, args, fmt, k, combo, every=10):
    with_m, x0, wide = combo
    M = matrix(name, *args)
    B = rhs_block(M.n)[:, :k]
    X0 = start_block(M.n)[:, :k] if x0 != "none" else None
    want = restated(name, args, fmt, with_m, x0 != "none")[:k]
    what = "%s, k = %d, %s, x0 %s, %s" % (name, k, "jacobi" if with_m else "plain", x0, "column slices" if wide else "ld = k")
    got = solve(torch, H, B, X0, jacobi(name, *args) if with_m else None, every=every, alias=x0 == "alias", wide=wide)
    same(got, want, what, B, with_m)
    return want


@pytest.mark.parametrize("fmt,a,b", MAIN)
def test_every_number_is_the_restatements(torch, fmt, a, b):
    """A covering design, not the full product of matrices x k x combinations (1080 calls a path): every k runs on every matrix with
    four of the twelve combinations, chosen so that every (k, combination) pair runs on exactly one of the three matrices and every
    (matrix, combination) pair with at least three values of k.  A call's cost is the same on each matrix, so nothing cheap is
    picked; what is given up is the triple interaction of matrix, k and combination."""
    for j, (name, args) in enumerate(MATRICES):
        H = handle(matrix(name, *args), fmt, a, b)
        for i, k in enumerate(KS):
            for c, combo in enumerate(COMBOS):
                if (c + i + j) % 3 == 0:
                    want = run_combo(torch, H, name, args, fmt, k, combo)
                    assert all(r[2] == cm.CONVERGED and r[0] < MAX_STEPS for r in want), "%s: the restatement did not converge" % name
        H.close()


@pytest.mark.parametrize("a,b", CSR_VARIANTS)
def test_the_bits_do_not_depend_on_the_spmv_plan(torch, a, b):
    """The SpMV plan never enters K20's code path, so each plan gets a sample and not MAIN's design: on every matrix an idle
    remainder (3), a full group (16), 16 + 1 and 16 + 16 + 1, each with another combination."""
    for j, (name, args) in enumerate(MATRICES):
        H = handle(matrix(name, *args), "csr", a, b)
        before = H.describe()
        for i, k in enumerate((3, 16, 17, 33)):
            run_combo(torch, H, name, args, "csr", k, COMBOS[(2 * j + 5 * i + 1) % len(COMBOS)])
        assert H.describe() == before, "the call changed the handle's SpMV plan"
        H.close()


def test_the_python_method(torch):
    name, args = MATRICES[0]
    M = matrix(name, *args)
    B, X0, m = rhs_block(M.n)[:, :5], start_block(M.n)[:, :5], jacobi(name, *args)
    for fmt, a, b in BOTH:
        H = handle(M, fmt, a, b)
        wideB = torch.full((M.n, 9), float("nan"), dtype=torch.float64, device="cuda")
        wideB[:, 2:7] = dev(torch, B)
        X = dev(torch, X0)
        results, rr, rz, sigma = H.cg_multi(wideB[:, 2:7], X, m=dev(torch, m), X0=X, max_steps=MAX_STEPS, tol=TOL, check_every=7)
        want = restated(name, args, fmt, True, True)[:5]
        assert [(r.steps, r.updates, r.reason) for r in results] == cm.outcomes(want)
        assert rr.shape == (5, MAX_STEPS + 1) and rz.shape == (5, MAX_STEPS + 1) and sigma.shape == (5, MAX_STEPS)
        wrr, wrz, wsigma = cm.flat_histories(want, MAX_STEPS, np.nan)
        assert_bits(rr.ravel(), wrr, "rr_each")
        assert_bits(rz.ravel(), wrz, "rz_each")
        assert_bits(sigma.ravel(), wsigma, "sigma_each")
        assert_bits(X.cpu().numpy().ravel(), cm.solution(want).ravel(), "X")
        out = H.cg_multi(dev(torch, B), X)
        assert out[2] is None and len(out[0]) == 5
        with pytest.raises(ValueError):
            H.cg_multi(dev(torch, B).cpu(), X)
        with pytest.raises(ValueError):
            H.cg_multi(dev(torch, B).t().contiguous().t(), X)                 # column-major: out of scope
        H.close()


# =================================================================================================== 2. every way out, in one block
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_every_way_out_mixed_in_one_block(torch, fmt, a, b):
    M, B = cm.signed_diagonal(), cm.mixed_block()
    H = handle(M, fmt, a, b)
    for m, expect in ((None, cm.MIXED_PLAIN), (np.abs(cm.signed_diagonal_values()), cm.MIXED_JACOBI)):
        want = cm.run(cm.product_of(M, fmt), B, None, m, cm.MIXED_STEPS, cm.MIXED_TOL)
        assert cm.outcomes(want) == expect, "the restatement's block does not cover what it is here for: %r" % cm.outcomes(want)
        assert {r[2] for r in want} >= {cm.CONVERGED, cm.BREAKDOWN, cm.NONFINITE}
        if m is None:
            assert {r[2] for r in want} == {cm.CONVERGED, cm.MAX_STEPS, cm.BREAKDOWN, cm.NONFINITE}
        gots = []
        for every in (1, 2, 1000):
            for wide in (False, True):
                got = solve(torch, H, B, None, m, cm.MIXED_STEPS, cm.MIXED_TOL, every, wide=wide)
                same(got, want, "%s, %s, check_every %d" % (fmt, "plain" if m is None else "jacobi", every), None, m is not None)
                gots.append(got)
        for got in gots[1:]:
            for v in range(6):
                same_column(column(got, v), column(gots[0], v), "column %d under another check_every" % v)
    H.close()


# ========================================================================================================= 3. column independence
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_columns_numbers_depend_on_nothing_beside_it(torch, fmt, a, b):
    name, args = MATRICES[0]
    M = matrix(name, *args)
    n = M.n
    H = handle(M, fmt, a, b)
    b0, b1, x0 = rhs_block(n)[:, 0], rhs_block(n)[:, 1], start_block(n)[:, 0]
    nan, zero = np.full(n, np.nan), np.zeros(n)
    for m in (None, jacobi(name, *args)):
        for with_x0 in (False, True):
            alone = column(solve(torch, H, b0[:, None], x0[:, None] if with_x0 else None, m), 0)
            want = restated(name, args, fmt, m is not None, with_x0)[0]
            assert alone[0] == tuple(want[:3])
            for cols, at in (([b1, b0], 1), ([nan, b0, zero], 1), ([b0, nan], 0), ([zero, b1, nan, b1, b0], 4),
                             ([b1] * 16 + [b0], 16), ([nan] * 15 + [b0, b1], 15)):
                B = np.stack(cols, axis=1)
                X0 = np.stack([x0] * len(cols), axis=1) if with_x0 else None
                got = solve(torch, H, B, X0, m, wide=at % 2 == 1)
                same_column(column(got, at), alone, "%s, %d columns, at position %d" % (fmt, len(cols), at))
                for v, c in enumerate(cols):
                    if c is nan:
                        assert (got.results[v].steps, got.results[v].updates, got.results[v].reason) == (0, 0, cm.NONFINITE)
                    if c is zero and not with_x0:
                        assert (got.results[v].steps, got.results[v].reason) == (0, cm.CONVERGED) and not got.X[:, v].any()
    H.close()


# ================================================================================================ 4. cross-check against tested code
def test_k_calls_of_the_one_vector_solvers_give_the_same_bits(torch):
    name, args = MATRICES[0]
    M = matrix(name, *args)
    n, k = M.n, 5
    assert M.terms.max() <= 32, "the default kernel is the serial loop on rows of at most 32 entries only"
    H = handle(M, "csr", *AUTO)
    B, X0, m = rhs_block(n)[:, :k], start_block(n)[:, :k], jacobi(name, *args)
    # the handle's single product IS the oracle's serial loop on every operand the runs multiply
    used = []
    serial = cm.csr_product(M)

    def recording(x):
        used.append(np.array(x, copy=True))
        return serial(x)
    for with_m in (False, True):
        cm.run(recording, B[:, :2], X0[:, :2], m if with_m else None, MAX_STEPS, TOL)
    assert len(used) > 20
    for x in used:
        buf, dy = guarded_y(torch, n)
        H.spmv(dev(torch, x), dy)
        torch.cuda.synchronize()
        check_guards(buf, n)
        assert_bits(dy.cpu().numpy(), serial(x), "smvp_csr_spmv against the serial loop")
    for with_m in (False, True):
        for with_x0 in (False, True):
            got = solve(torch, H, B, X0 if with_x0 else None, m if with_m else None, every=4)
            for v in range(k):
                dx = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
                d0 = dev(torch, X0[:, v]) if with_x0 else None
                if with_m:
                    r, rr, rz, sigma = H.pcg(dev(torch, B[:, v]), dx, dev(torch, m), x0=d0, max_steps=MAX_STEPS, tol=TOL, check_every=3)
                else:
                    r, rr, sigma = H.cg(dev(torch, B[:, v]), dx, x0=d0, max_steps=MAX_STEPS, tol=TOL, check_every=3)
                    rz = None
                what = "column %d against smvp_csr_%s" % (v, "pcg" if with_m else "cg")
                mine = column(got, v)
                assert mine[0] == (r.steps, r.updates, r.reason), what
                assert_bits(mine[1], [r.rr, r.rz if with_m else r.rr, r.bb], what + ": the result block")
                assert_bits(mine[2][:r.updates + 1], rr, what + ": rr_each")
                if with_m:
                    assert_bits(mine[3][:r.updates + 1], rz, what + ": rz_each")
                assert_bits(mine[4][:r.steps], sigma, what + ": sigma_each")
                assert_bits(mine[5], dx.cpu().numpy(), what + ": x")
    # m all ones: every number is the plain run's, and rz_each is rr_each
    plain, ones = solve(torch, H, B, X0), solve(torch, H, B, X0, np.ones(n))
    for v in range(k):
        p, o = column(plain, v), column(ones, v)
        same_column(p[:3] + (p[2],) + p[4:], o, "m = ones against no m, column %d" % v)
        assert (p[3] == SENTINEL).all()
    H.close()


# ==================================================================================================== 5. sizes at the passes' edges
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_sizes_around_a_workgroup(torch, n):
    M = matrix("spd", n, 20280 + n)
    m = pcg.diagonal(M)
    for fmt, a, b in BOTH:
        H = handle(M, fmt, a, b)
        product = cm.product_of(M, fmt)
        for k in (1, 3, 16):
            B, X0 = rhs_block(n, 16)[:, :k], start_block(n, 16)[:, :k]
            for mm, x0, wide in ((None, X0, False), (m, None, True), (m, X0, False)):
                want = cm.run(product, B, x0, mm, 12, TOL)
                got = solve(torch, H, B, x0, mm, 12, TOL, 5, wide=wide, alias=x0 is not None and k == 3)
                same(got, want, "spd(%d), %s, k = %d" % (n, fmt, k), B, mm is not None)
        H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_row_past_the_first_grid_trip(torch, fmt, a, b):
    M = matrix("spd", cg.TRIP + 1)
    B, X0 = rhs_block(M.n, 3), start_block(M.n, 3)
    H = handle(M, fmt, a, b)
    want = cm.run(cm.product_of(M, fmt), B, X0, None, 3, 0.0)
    assert cm.outcomes(want) == [(3, 3, cm.MAX_STEPS)] * 3
    same(solve(torch, H, B, X0, None, 3, 0.0, 2, wide=True), want, "spd(%d), %s" % (M.n, fmt), B)
    H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    for H in (A, T):
        for dm in (None, torch.ones(1, dtype=torch.float64, device="cuda")):
            o, r = sm.cg_opts(5), (sm.PcgResult * 3)()
            C.memset(r, 0x5a, C.sizeof(r))
            b = torch.zeros(3, dtype=torch.float64, device="cuda")
            rr, rz, sigma = np.full(18, SENTINEL), np.full(18, SENTINEL), np.full(15, SENTINEL)
            rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), 3, sm._dev_ptr(b), 3, None, 0, None, 3, sm._dev_ptr(dm), r, sm._p(rr), sm._p(rz),
                                             sm._p(sigma), None)
            assert rc == sm.OK, sm.lib().smvp_last_error().decode()
            for blk in r:
                assert (blk.steps, blk.updates, blk.reason, blk.pad) == (0, 0, cm.CONVERGED, 0)
                assert_bits([blk.rr, blk.rz, blk.bb], [0.0, 0.0, 0.0], "n = 0")
            assert (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all()
        H.close()


# ========================================================================================================================= 6. state
@pytest.mark.parametrize("a,b", [AUTO, (sm.CSR_KERNEL_STREAM, 256), (sm.CSR_KERNEL_VECTOR, 8), (sm.CSR_KERNEL_COLSWEEP, 0),
                                 (sm.CSR_KERNEL_BINNED, 1)])
def test_a_csr_handles_products_are_the_same_before_and_after(torch, a, b):
    name, args = MATRICES[1]
    M = matrix(name, *args)
    H = handle(M, "csr", a, b)
    dx = dev(torch, cg.rhs(M.n, 4))
    products = []
    for _ in range(4):                                       # (the tile kernel's sweep direction may alternate: two products each)
        if len(products) == 2:
            plan = H.describe()
            run_combo(torch, H, name, args, "csr", 4, COMBOS[3])
            run_combo(torch, H, name, args, "csr", 4, COMBOS[3])
            assert H.describe() == plan
        buf, dy = guarded_y(torch, M.n)
        H.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        products.append(dy.cpu().numpy())
    assert_bits(products[2], products[0], "the first product after the calls")
    assert_bits(products[3], products[1], "the second product after the calls")
    H.close()


@pytest.mark.parametrize("mode", [sm.TJDS_MODE_ROW_GATHER, sm.TJDS_MODE_TWO_PHASE])
def test_a_set_x_spmv_pair_straddling_the_call_is_undisturbed(torch, mode):
    name, args = MATRICES[2]
    M = matrix(name, *args)
    H = handle(M, "tjds", mode, 0)
    dx = dev(torch, cg.rhs(M.n, 4))

    def spmv():
        buf, dy = guarded_y(torch, M.n)
        H.zero_y(dy)
        H.spmv(dy)
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        return dy.cpu().numpy()
    H.set_x(dx)
    want = spmv()
    H.set_x(dx)
    run_combo(torch, H, name, args, "tjds", 5, COMBOS[2])     # between set_x and spmv: the first call, which builds the plan
    assert_bits(spmv(), want, "set_x, cg_multi, spmv")
    run_combo(torch, H, name, args, "tjds", 5, COMBOS[9])
    assert_bits(spmv(), want, "no new set_x after another call")
    H.close()


def test_adopted_values_changed_in_place_are_seen_by_the_next_call(torch):
    from test_gpu_adopted import coo_to_device

    M = matrix("spd", 257, 20280 + 257)
    rows, cols, vals = (np.array(M.coo[f]) for f in ("row", "col", "val"))
    M3 = pi.Matrix(M.n, rows, cols, 3.0 * vals)              # 3 A: the same structure, still symmetric positive definite
    B, X0 = rhs_block(M.n, 16)[:, :4], start_block(M.n, 16)[:, :4]
    rp, ci, val = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in M.csr)
    A = sm.CsrMatrix(M.n, M.n, rp, ci, val)
    t = sm.tjds_from_coo_device(coo_to_device(torch, M.coo), M.n, M.n, len(M.coo))
    T = sm.TjdsMatrix(t)
    for H, fmt, values in ((A, "csr", val), (T, "tjds", t.val)):
        same(solve(torch, H, B, X0, None, 12, TOL), cm.run(cm.product_of(M, fmt), B, X0, None, 12, TOL), fmt + ", adopted", B)
        values.mul_(3.0)                                     # in place; no call on the handle before the next solve
        torch.cuda.synchronize()
        same(solve(torch, H, B, X0, None, 12, TOL), cm.run(cm.product_of(M3, fmt), B, X0, None, 12, TOL), fmt + ", val scaled in place", B)
        H.close()


# ====================================================================================================================== 7. refusals
def refused(torch, fn, h, n, k, o, results=True, B="own", ldb=None, X0=None, ldx0=0, X="own", ldx=None, m=None):
    """The status of one call that must be refused: the guarded X, the result blocks and the histories come back untouched."""
    rows = max(n, 1)
    bufx, dX = guarded_block(torch, rows, max(k, 1), max(k, 1) + 2, 1, SENTINEL)
    dB = torch.ones((rows, max(k, 1)), dtype=torch.float64, device="cuda") if isinstance(B, str) else B
    r = (sm.PcgResult * max(k, 1))()
    C.memset(r, 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, rz, sigma = np.full(8 * max(k, 1), SENTINEL), np.full(8 * max(k, 1), SENTINEL), np.full(8 * max(k, 1), SENTINEL)
    torch.cuda.synchronize()
    own = isinstance(X, str)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, k, sm._dev_ptr(dB), max(k, 1) if ldb is None else ldb,
                               sm._dev_ptr(X0), ldx0, sm._dev_ptr(dX if own else X), (max(k, 1) + 2 if own else max(k, 1)) if ldx is None else ldx,
                               sm._dev_ptr(m), r if results else None, sm._p(rr), sm._p(rz), sm._p(sigma), None)
    msg = sm.lib().smvp_last_error().decode()
    torch.cuda.synchronize()
    assert (dX.cpu().numpy() == SENTINEL).all(), "%s wrote d_X although it refused" % fn
    check_block_guards(bufx, rows, max(k, 1), max(k, 1) + 2, 1, "X")
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all(), \
        "%s wrote its outputs although it refused" % fn
    return rc, msg, dX


def bad_opts():
    def o(**kw):
        v = sm.cg_opts(5)
        for f, x in kw.items():
            setattr(v, f, x)
        return v
    return [None, o(struct_size=20), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf"))]


def test_every_refusal_returns_its_code_and_writes_nothing(torch):
    M = matrix("spd", 63, 20280 + 63)
    n, k = M.n, 3
    A, T = handle(M, "csr", *AUTO), handle(M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                        # 3 x 4
    W, WT = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3)), sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.cg_opts(5)
    INV = sm.ERR_INVALID
    for fn, H, Wide in (("smvp_csr_cg_multi", A, W), ("smvp_tjds_cg_multi", T, WT)):
        h = H._h
        assert refused(torch, fn, None, n, k, ok)[0] == INV
        for o in bad_opts():
            assert refused(torch, fn, h, n, k, o)[0] == INV, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, h, n, k, ok, results=False)[0] == INV
        assert refused(torch, fn, h, n, k, ok, B=None)[0] == INV                      # no d_B
        assert refused(torch, fn, Wide._h, 4, k, ok)[0] == INV                        # rows != cols
        assert refused(torch, fn, h, n, k, ok, X=None)[0] == INV                      # no d_X
        for bad_k in (0, -1):
            assert refused(torch, fn, h, n, bad_k, ok)[0] == INV
        x0 = torch.zeros((n, k), dtype=torch.float64, device="cuda")
        assert refused(torch, fn, h, n, k, ok, ldb=k - 1)[0] == INV                   # a leading dimension below k, each in turn
        assert refused(torch, fn, h, n, k, ok, ldx=k - 1)[0] == INV
        assert refused(torch, fn, h, n, k, ok, X0=x0, ldx0=k - 1)[0] == INV
        both = torch.full((n * (k + 1) + k,), SENTINEL, dtype=torch.float64, device="cuda")
        lo, hi = both[:n * k].view(n, k), both[1:n * k + 1].view(n, k)                # two blocks one element apart
        for args in (dict(X0=lo, ldx0=k, X=hi), dict(X0=hi, ldx0=k, X=lo), dict(B=lo, X=lo), dict(B=lo, X=hi), dict(B=hi, X=lo),
                     dict(X0=lo, ldx0=k + 1, X=lo),                                   # the same pointer under another leading dimension
                     dict(m=both[:n], X=lo), dict(m=both[n * k - 1:n * k - 1 + n], X=lo), dict(m=both[k:k + n], X=lo, ldx=k + 1)):
            assert refused(torch, fn, h, n, k, ok, **args)[0] == INV, sorted(args)
        assert (both.cpu().numpy() == SENTINEL).all()
        # a column slice beside X in the same wide array does not overlap it byte for byte, but its rows interleave with X's: the
        # byte RANGES meet, which is what is refused (as smvp_csr_spmm refuses it)
        two = torch.full((n, 2 * k), SENTINEL, dtype=torch.float64, device="cuda")
        assert refused(torch, fn, h, n, k, ok, B=two[:, :k], ldb=2 * k, X=two[:, k:], ldx=2 * k)[0] == INV
        assert (two.cpu().numpy() == SENTINEL).all()
    T2 = handle(matrix("spd", 1003), "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    Mbig = matrix("spd", 1003)
    inner = inner_csr_handle(T2, Mbig.n, Mbig.n, Mbig.nnz)                             # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_cg_multi", inner, Mbig.n, k, ok)[0] == sm.ERR_UNSUPPORTED
    # TJDS is accepted in every mode, ATOMIC and ref-quirks included: the block product's bits depend on neither
    name, args = MATRICES[0]
    T2.set_mode(sm.TJDS_MODE_ATOMIC)
    run_combo(torch, T2, name, args, "tjds", 3, COMBOS[4])
    T2.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T2.set_ref_quirks(True)
    run_combo(torch, T2, name, args, "tjds", 3, COMBOS[7])
    T2.set_ref_quirks(False)
    # and the handles work after the refusals
    B = rhs_block(n, 16)[:, :k]
    for H, fmt in ((A, "csr"), (T, "tjds")):
        same(solve(torch, H, B, None, None, 5, TOL), cm.run(cm.product_of(M, fmt), B, None, None, 5, TOL), fmt + ": after the refusals", B)
    for H in (A, T, W, WT, T2):
        H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = matrix("spd", 63, 20280 + 63)
    H = handle(M, fmt, a, b)
    B = rhs_block(M.n, 16)[:, :3]
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dX = torch.full((M.n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    dB, dm = dev(torch, B), dev(torch, np.ones(M.n))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.cg_opts(5), (sm.PcgResult * 3)(), []
    C.memset(r, 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, rz, sigma = np.full(18, SENTINEL), np.full(18, SENTINEL), np.full(15, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            for m in (None, dm):
                got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), 3, sm._dev_ptr(dB), 3, None, 0, sm._dev_ptr(dX), 3, sm._dev_ptr(m), r,
                                                       sm._p(rr), sm._p(rz), sm._p(sigma), s.cuda_stream))
                got.append("captur" in sm.lib().smvp_last_error().decode())
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID, True] * 2
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dX.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, B, None, None, 5, TOL, stream=s), cm.run(cm.product_of(M, fmt), B, None, None, 5, TOL),
         "outside a capture the same stream is fine", B)
    H.close()


# ================================================================================================================== 8. stream order
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_stream_of_the_callers_with_the_operands_still_in_flight(torch, fmt, a, b):
    name, args = MATRICES[0]
    M = matrix(name, *args)
    k = 5
    B, X0, m = rhs_block(M.n)[:, :k], start_block(M.n)[:, :k], jacobi(name, *args)
    side = torch.cuda.Stream()
    H = handle(M, fmt, a, b)
    seen = []
    got = solve(torch, H, B, X0, m, every=3, stream=side, wide=True, before=so.solver_hook(torch, side, seen))
    assert seen and all(event.query() for event, _ in seen), "the call returned before the work on its stream had finished"
    same(got, restated(name, args, fmt, True, True)[:k], "jacobi, %s, everything in flight" % fmt, B, True)
    same(solve(torch, H, B, None, None, every=4, stream=side), restated(name, args, fmt, False, False)[:k], fmt + ", plain, a stream of the caller's", B)
    H.close()


# =================================================================================== 9. resources and fresh memory, in a child process
SCRIPT = os.path.join(ROOT, "tests", "cg_multi_scenarios.py")
_crashed = []


@pytest.mark.parametrize("group", ["resources", "fresh"])
def test_the_call_gives_back_what_it_took_and_reads_no_fresh_memory(group):
    """tests/cg_multi_scenarios.py against lib/libsmvp_amd_counted.so, one child per group under one time limit, nothing retried: a
    successful call, every refusal and each obtaining call of the workspace failing in turn leave the counters where they were; the
    same solves with the fill off and under both fill patterns give the same bits.  After an error of the device the child runs
    nothing more, and no further group is started."""
    assert not _crashed, "not started: the group %r ended in a crash or at its time limit" % _crashed[0]
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    env = dict(os.environ, SMVP_LIB_PATH=COUNTED)
    try:
        p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired as e:
        _crashed.append(group)
        seen = e.stdout or ""
        seen = seen.decode(errors="replace") if isinstance(seen, bytes) else seen
        raise AssertionError("group %s did not finish in %d s\n%s" % (group, LIMIT_S, seen[-3000:]))
    if p.returncode not in (0, 1, 2):
        _crashed.append(group)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
