"""GPU: restarted GMRES on a handle (smvp_csr_gmres / smvp_tjds_gmres, kernel K19) against its numpy restatement
tests/gmres_method.py (test_gmres_host.py pins that to hand-computed runs, to the true residual and to its step counts).

No tolerance anywhere.  The header fixes the order of every addition of the dot, the two roots are the correctly rounded IEEE
root, yhat = M^-1 y is K18's, everything else is one rounded IEEE operation, and the restatement's product argument is the SAME
handle's single product (test_gpu_bicgstab.handle): steps, cycles, columns, reason, rr, bb, both histories and every bit of d_x
have one right answer.  Comparisons are transposed.assert_bits on the uint64 views.  Every solver call goes through solve() below,
which gives d_x a guarded buffer, checks the guards, checks that d_b and d_m come back unchanged and that the histories keep a
sentinel beyond the filled elements.  The serial substitution in Python is the reference, so n stays at about 3000 at the most
wherever a plan is used."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bicgstab_method as bi
import gmres_method as gm
import pbicgstab_method as pb
import power_iteration as pi
import smvp_toolkit_amd as sm
import stream_order as so
import test_gpu_bicgstab as k13
import test_gpu_pbicgstab as k18
import trsv_method as trsv
from conftest import ROOT
from parity import check_guards, guarded_y
from test_gpu_bicgstab import AUTO, BOTH, PATHS, SENTINEL, dev, handle, start_vector
from test_gpu_resources import COUNTED, LIMIT_S, PKG
from test_gpu_transposed import inner_csr_handle
from test_gmres_host import STEPS_ON_CONVDIFF
from transposed import assert_bits

pytestmark = pytest.mark.gpu

CHUNK = 4                                                    # kGmChunk of csrc/smvp_gmres.hip: coefficients a lane accumulates at a time
TOL = 1e-8
banded = functools.lru_cache(maxsize=None)(bi.banded)        # built once and left unchanged


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class NoPlans:
    first = second = m = None
    triples = (None, None, None)

    def close(self):
        pass


PLAIN = NoPlans()


def fn_of(H):
    return "smvp_%s_gmres" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds")


def entries(max_steps, restart):
    return max_steps + 1, -(-max_steps // restart) + 1


def solve(torch, H, n, b, P, x0, restart, max_steps, tol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, cycles, columns, reason, rr_each, restart_each, x, rr, bb): gmres_method.run_rr's
    tuple, then bb.  P: anything with first, second (TrsvPlans or None) and m (numpy or None).  alias: d_x is d_x0.  Nothing is
    synchronised after the call: it returns when the work is done.  rr_each is filled for steps + 1 elements, or one fewer where
    rule S1 ended the run: its count is read off the sentinel, and same() holds it to the restatement's.
    before: called in place of the leading torch.cuda.synchronize() with the call's device vectors (stream_order.solver_hook puts
    them in flight on `stream`)."""
    buf, dx = guarded_y(torch, n)
    d0 = None
    if x0 is not None and alias:
        dx.copy_(torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)))
        d0 = dx
    elif x0 is not None:
        d0 = dev(torch, x0)
    db, dm = dev(torch, b), (dev(torch, P.m) if P.m is not None else None)
    o, r = sm.gmres_opts(max_steps, tol, every, restart), sm.GmresResult()
    nrr, ntr = entries(max_steps, restart)
    rr, tr = np.full(nrr, SENTINEL), np.full(ntr, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0, m=dm)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx),
                                     P.first._t if P.first is not None else None, sm._dev_ptr(dm),
                                     P.second._t if P.second is not None else None, C.byref(r), sm._p(rr), sm._p(tr),
                                     sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    if dm is not None:
        assert_bits(dm.cpu().numpy(), P.m, "d_m after the call")
    assert 0 <= r.steps <= max_steps and 1 <= r.cycles <= ntr - 1 and 0 <= r.columns <= min(restart, max_steps)
    filled = r.steps + 1
    if r.steps > 0 and rr[r.steps] == SENTINEL:              # rule S1: the last step has no rr
        filled -= 1
    assert (rr[filled:] == SENTINEL).all(), "rr_each was written beyond its filled elements"
    assert not (rr[:filled] == SENTINEL).any(), "an element of rr_each was not filled"
    assert (tr[r.cycles:] == SENTINEL).all(), "restart_each was written beyond its filled elements"
    assert not (tr[:r.cycles] == SENTINEL).any(), "an element of restart_each was not filled"
    assert not np.signbit(np.concatenate([rr[:filled], tr[:r.cycles], [r.bb]])).any(), "a squared norm is -0.0 or negative"
    return r.steps, r.cycles, r.columns, r.reason, rr[:filled], tr[:r.cycles], x, np.float64(r.rr), np.float64(r.bb)


def restated(product, b, P, x0, restart, max_steps, tol):
    return gm.run_rr(product, b, x0, *P.triples, restart, max_steps, tol)


def same(got, want, what, b=None):
    """steps, cycles, columns, reason; both histories (their lengths too), every bit of x and the result block's rr; bb where b
    is given.  want: gmres_method.run_rr's tuple."""
    assert tuple(got[:4]) == tuple(want[:4]), "%s: (steps, cycles, columns, reason) = %r, the restatement has %r" % (what, got[:4], want[:4])
    assert_bits(got[4], want[4], what + ": rr_each")
    assert_bits(got[5], want[5], what + ": restart_each")
    assert_bits(got[6], want[6], what + ": d_x")
    if len(got) > 7 and len(want) > 7:
        assert_bits([got[7]], [want[7]], what + ": rr")
    if len(got) > 8 and b is not None:
        assert_bits([got[8]], [bi.dot(b, b)], what + ": bb")


def both(torch, H, product, n, b, P, x0, restart, max_steps, tol, what, every=10, **kw):
    want = restated(product, b, P, x0, restart, max_steps, tol)
    got = solve(torch, H, n, b, P, x0, restart, max_steps, tol, every, **kw)
    same(got, want, what, b)
    return want


# ========================================================================================================== 1. the root, first
def identity_handle(n):
    return sm.CsrMatrix(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def root_inputs():
    """Vectors b of 1, 2 or 3 elements whose tr_0 = dot(b, b) is the root's argument: subnormal arguments, arguments near overflow,
    squares of random numbers of every binade parity (a rounded square is the hardest argument: its root is within an ulp of a
    tie-free double), and exact squares +- 1 ulp: (2^26 + 1)^2 + 1 as two elements, (2^26 + 1)^2 - 1 = 2^52 + 2^26 + 2^26 as
    three, both scaled by powers of four."""
    rng = np.random.default_rng(1900)
    for t in rng.uniform(1.0, 4.0, 1500):
        yield [t]
    for t in rng.uniform(1.0, 4.0, 400) * 2.0 ** rng.integers(-500, 500, 400):
        yield [t]
    for t in rng.uniform(1.0, 2.0, 300) * 2.0 ** rng.integers(-537, -512, 300):       # t * t is subnormal, and not zero
        yield [t]
    for t in rng.uniform(1.0, 1.4, 300) * 2.0 ** 511:                                 # t * t up to 1.96 * 2^1022
        yield [t]
    yield [2.0 ** -537]                                                               # the smallest subnormal
    yield [np.sqrt(np.finfo(np.float64).max) * (1 - 2.0 ** -52)]
    for e in range(-40, 41, 4):
        s = 2.0 ** e
        yield [(2.0 ** 26 + 1) * s, s]
        yield [2.0 ** 26 * s, 2.0 ** 13 * s, 2.0 ** 13 * s]
        yield [(2.0 ** 26 + 3) * s, s]


def test_the_root_is_the_correctly_rounded_one(torch):
    """One step of GMRES on the identity with restart = 1 and tol = 0: restart_each[0] = dot(b, b) is the argument (held to
    smvp_vector_dot of b with itself and to numpy's product), beta = sqrt(tr_0) divides b, and rr_each[1], x and the result are the
    restatement's -- whose roots are numpy.sqrt's -- bit for bit.  h_2 and d are two more roots per run."""
    handles = {n: identity_handle(n) for n in (1, 2, 3)}
    for n, H in handles.items():                                                      # the product of these handles is the identity
        v = np.array([1.5, -2.25, 3.0][:n])
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        H.spmv(dev(torch, v), y)
        assert_bits(y.cpu().numpy(), v, "the identity's product")
    count, roots = 0, set()
    for b in root_inputs():
        b = np.array(b, dtype=np.float64)
        n = len(b)
        want = gm.run_rr(lambda v: v.copy(), b, None, None, None, None, 1, 1, 0.0)
        assert np.isfinite(want[5][0]) and want[5][0] > 0.0, "the argument %r is no argument" % want[5][0]
        db, dx = dev(torch, b), torch.empty(n, dtype=torch.float64, device="cuda")
        o, r = sm.gmres_opts(1, 0.0, 1, 1), sm.GmresResult()
        rr, tr = np.full(2, SENTINEL), np.full(2, SENTINEL)
        assert sm.lib().smvp_csr_gmres(handles[n]._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), None, None, None, C.byref(r),
                                       sm._p(rr), sm._p(tr), None) == sm.OK
        what = "b = %r (tr_0 = %r, its root %r)" % (b.tolist(), float(want[5][0]), float(np.sqrt(want[5][0])))
        assert_bits([sm.vector_dot(db, db)], want[5], what + ": smvp_vector_dot")
        got = (r.steps, r.cycles, r.columns, r.reason, rr[:r.steps + 1], tr[:r.cycles], dx.cpu().numpy(), np.float64(r.rr))
        same(got, want, what)
        count += 1
        roots.add(float(want[5][0]))
    print("%d runs, %d different arguments of the first root" % (count, len(roots)))
    assert count > 2500 and len(roots) > 2500
    for H in handles.values():
        H.close()


# ============================================================================================================ 2. the coefficients
@pytest.mark.parametrize("n", [1, 255, 256, 257, 700])
def test_the_coefficients_of_the_first_steps(torch, n):
    """restart 1: every step is a cycle of one column, so rr_each[1] and x hold h_1 = dot(v_1, w) + dot(v_1, w'), h_2 and the root
    of their squares and nothing else."""
    M = k13.matrix("nonsym", n, 20300 + n)
    rhs = bi.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            for steps in (1, 3):
                both(torch, H, product, n, rhs, PLAIN, x0, 1, steps, 0.0, "nonsym(%d), %s, %d steps" % (n, fmt, steps), every=2)
        H.close()


# ================================================================================================= 3. bits against run(), every path
@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name, args in k13.LARGE:
        M = k13.matrix(name, *args)
        H, product = handle(torch, M, fmt, a, b)
        rhs, x0 = bi.rhs(M.n), start_vector(M.n)
        for start, every, alias in ((None, 7, False), (x0, 3, False), (x0, 1000, True)):
            what = "%s, %s %d %d, x0 %s%s" % (name, fmt, a, b, "NULL" if start is None else "random", ", d_x is d_x0" if alias else "")
            want = both(torch, H, product, M.n, rhs, PLAIN, start, 5, 60, 1e-10, what, every, alias=alias)
            assert want[3] == gm.CONVERGED and want[1] > 1, "%s: the restatement did not converge after a restart" % what
        H.close()


# =================================================================================================================== 4. the restart
@pytest.mark.parametrize("restart", sorted({1, 2, 5, 30, 64, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1}))
def test_every_width_of_the_multi_dot(torch, restart):
    """max_steps = 2 * restart + 1 at tol 0 (restart 64: 64 steps, the widest multi-dot and every chunk tail on the way): two
    whole cycles and the first column of a third; then the run to convergence."""
    M = k13.matrix("nonsym", 1003)
    rhs = bi.rhs(M.n)
    steps = 64 if restart == 64 else 2 * restart + 1
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = both(torch, H, product, M.n, rhs, PLAIN, None, restart, steps, 0.0, "restart %d, %s, tol 0" % (restart, fmt), every=7)
        assert want[0] == steps or want[3] == gm.CONVERGED
        want = both(torch, H, product, M.n, rhs, PLAIN, start_vector(M.n), restart, 80, 1e-10, "restart %d, %s" % (restart, fmt), every=4)
        assert want[3] == gm.CONVERGED
        H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_lanes_that_take_more_than_one_slot(torch, fmt, a, b):
    """n = 256 * 2048 + 300: one restart, two trips per lane and a ragged last trip -- the smallest n at which the slot map of the
    multi-dot, of the updates and of the close can go wrong."""
    n = bi.TRIP + 300
    M = banded(n)
    rhs = bi.rhs(n)
    H, product = handle(torch, M, fmt, a, b)
    want = both(torch, H, product, n, rhs, PLAIN, None, 3, 4, 0.0, "banded(%d), %s" % (n, fmt), every=3)
    assert want[:4] == (4, 2, 1, gm.MAX_STEPS)
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_past_the_unrolled_bodies(torch, fmt, a, b):
    """n = 4 * 2048 * 256 + 1: the four-deep bodies of the updates and of the close, the two-deep body of the multi-dot twice, and
    one element over."""
    n = 4 * bi.TRIP + 1
    M = banded(n)
    rhs = bi.rhs(n)
    H, product = handle(torch, M, fmt, a, b)
    m = 1.0 / (2.0 + (np.arange(n) % 7) / 8.0)
    P = type("P", (), dict(first=None, second=None, m=m, triples=(None, m, None)))
    want = both(torch, H, product, n, rhs, P, None, 2, 3, 0.0, "banded(%d), %s, Jacobi" % (n, fmt), every=2)
    assert want[:4] == (3, 2, 1, gm.MAX_STEPS)
    H.close()


# ============================================================================================================ 5. the preconditioners
@pytest.mark.parametrize("kind", ["plain", "jacobi", "sgs", "ilu0"])
def test_every_preconditioner_on_convdiff_and_the_pinned_step_counts(torch, kind):
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    rhs = bi.rhs(M.n)
    P = PLAIN if kind == "plain" else k18.plans_of(torch, kind, Cs)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = both(torch, H, product, M.n, rhs, P, None, 30, 400, TOL, "convdiff(32, 0.5) with %s, %s" % (kind, fmt), every=7)
        probe = start_vector(M.n, 3)
        serial = product(probe).tobytes() == M.spmv(probe).tobytes() and product(rhs).tobytes() == M.spmv(rhs).tobytes()
        print("convdiff(32, 0.5) with %s, %s: steps %d, cycles %d, columns %d; the product's bits are the serial loop's: %s" % (
            kind, fmt, want[0], want[1], want[2], serial))
        assert want[3] == gm.CONVERGED
        if serial:
            assert want[0] == STEPS_ON_CONVDIFF[kind]
        if kind in ("sgs", "ilu0"):
            same(solve(torch, H, M.n, rhs, P, start_vector(M.n), 5, 100, TOL, 3, alias=True),
                 restated(product, rhs, P, start_vector(M.n), 5, 100, TOL), "%s, restart 5, x0 aliased, %s" % (kind, fmt), rhs)
        H.close()
    P.close()


def test_a_lone_lower_plan_and_the_other_systems(torch):
    for name, kind in (("nonsym_shuffled", "lower"), ("nonsym(1003), coalesced", "ilu0"), ("nonsym_long", "jacobi")):
        M, Cs = pb.case_of(name)
        P = k18.plans_of(torch, kind, Cs)
        rhs = bi.rhs(M.n)
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = both(torch, H, product, M.n, rhs, P, None, 3, 60, 1e-10, "%s with %s, %s" % (name, kind, fmt), every=4)
            assert want[3] == gm.CONVERGED
            H.close()
        P.close()


def test_identity_plans_and_an_m_of_ones_are_the_plain_run(torch):
    M = k13.matrix("nonsym_long")
    E = identity_handle(M.n)
    ident = type("P", (), dict(first=E.trsv_plan(sm.TRSV_LOWER, sm.TRSV_DIAG_STORED), second=E.trsv_plan(sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT),
                               m=None))
    ones = type("P", (), dict(first=None, second=None, m=np.ones(M.n)))
    rhs = bi.rhs(M.n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(M.n)):
            plain = solve(torch, H, M.n, rhs, PLAIN, x0, 4, 30, 1e-10, 3)
            assert plain[0] > 4
            for what, P in (("identity plans", ident), ("m of ones", ones)):
                same(solve(torch, H, M.n, rhs, P, x0, 4, 30, 1e-10, 3), plain, "%s, %s" % (fmt, what), rhs)
        H.close()
    ident.first.close()
    ident.second.close()
    E.close()


# ===================================================================================================== 6. check_every changes nothing
EVERY = (1, 3, 7, 1000)


def all_the_same(torch, H, product, M, rhs, P, x0, restart, max_steps, tol, what):
    want = restated(product, rhs, P, x0, restart, max_steps, tol)
    for every in EVERY:
        same(solve(torch, H, M.n, rhs, P, x0, restart, max_steps, tol, every), want, "%s, check_every %d" % (what, every), rhs)
    return want


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_nothing_depends_on_check_every(torch, fmt, a, b):
    M = k13.matrix("nonsym", 1003)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    # stops in mid-cycle; among them one whose stop step no check_every above looks at and that is no cycle's end
    unlooked = []
    for restart in (5, 6, 7, 9):
        for x0 in (None, start_vector(M.n)):
            want = all_the_same(torch, H, product, M, rhs, PLAIN, x0, restart, 80, 1e-10, "%s, restart %d" % (fmt, restart))
            assert want[3] == gm.CONVERGED
            if want[0] % 3 and want[0] % 7 and want[0] % restart:
                unlooked.append((restart, want[0]))
    print("%s: (restart, stop step) no check_every but 1 looks at, and no cycle's end: %r" % (fmt, unlooked))
    assert unlooked
    # a stop exactly at a cycle's end: by max_steps, and by convergence in the cycle's last column
    want = all_the_same(torch, H, product, M, rhs, PLAIN, None, 4, 8, 0.0, fmt + ", max_steps at a cycle's end")
    assert want[:4] == (8, 2, 4, gm.MAX_STEPS)
    full = restated(product, rhs, PLAIN, None, 64, 64, 1e-10)
    assert full[3] == gm.CONVERGED and full[1] == 1
    want = all_the_same(torch, H, product, M, rhs, PLAIN, None, full[0], 64, 1e-10, fmt + ", converged in a cycle's last column")
    assert want[:4] == (full[0], 1, full[0], gm.CONVERGED)
    # a stop by the start rule of cycle 1: a threshold between the last estimate of cycle 0 and the true residual after it
    found, bb = None, bi.dot(rhs, rhs)
    for restart in range(16, 2, -1):                                                  # (late in the run the two are 1e-10 apart, not an ulp)
        free = restated(product, rhs, PLAIN, None, restart, 2 * restart, 0.0)
        lo, hi = (free[5][1], free[4][restart]) if free[1] > 1 else (1.0, 0.0)
        if not lo < hi:
            continue
        tol = np.sqrt(((lo + hi) / 2) / bb)
        if lo <= (tol * tol) * bb < hi:
            found = restart, float(tol)
            break
    assert found, "no restart whose tr_1 lies below rr_restart"
    restart, tol = found
    want = all_the_same(torch, H, product, M, rhs, PLAIN, None, restart, 2 * restart, tol, fmt + ", the start rule of cycle 1")
    assert want[:4] == (restart, 2, 0, gm.CONVERGED) and len(want[4]) == restart + 1 and len(want[5]) == 2
    H.close()


def test_check_every_with_plans(torch):
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    P = k18.plans_of(torch, "ilu0", Cs)
    rhs = bi.rhs(M.n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = all_the_same(torch, H, product, M, rhs, P, start_vector(M.n), 4, 60, TOL, fmt + ", ILU(0), restart 4")
        assert want[3] == gm.CONVERGED and want[1] > 1
        H.close()
    P.close()


# ================================================================================================================ 7. the stop rules
def test_the_stop_rules_on_the_device(torch):
    inf = bi.rhs(300)
    inf[17] = np.inf
    A = k13.matrix("nonsym", 300)
    zero = pi.Matrix(3, [0], [0], [0.0])
    b4 = np.array([2.0, -2.0, 2.0, 2.0])
    cases = (("identity", k13.matrix("identity", 4), b4, 30, 10, 0.0, (1, 1, 1, gm.CONVERGED), b4),
             ("the zero matrix", zero, np.array([1.0, 2.0, 3.0]), 5, 10, 1e-10, (1, 1, 0, gm.BREAKDOWN), np.zeros(3)),
             ("the rotation, one step", bi.dense3([[0, -1], [1, 0]]), np.array([1.0, 0.0]), 2, 1, 1e-10, (1, 1, 1, gm.MAX_STEPS), np.zeros(2)),
             ("the rotation", bi.dense3([[0, -1], [1, 0]]), np.array([1.0, 0.0]), 2, 10, 1e-10, (2, 1, 2, gm.CONVERGED), np.array([0.0, -1.0])),
             ("the rotation, restart 1", bi.dense3([[0, -1], [1, 0]]), np.array([1.0, 0.0]), 1, 3, 1e-10, (3, 3, 1, gm.MAX_STEPS), np.zeros(2)),
             ("a NaN matrix value", k13.matrix("nan_value"), bi.rhs(300), 5, 10, 1e-10, (1, 1, 0, gm.NONFINITE), np.zeros(300)),
             ("inf in b", A, inf, 5, 10, 1e-10, (0, 1, 0, gm.NONFINITE), np.zeros(300)),
             ("bb overflows", A, np.full(300, 1e200), 5, 10, 1e-10, (0, 1, 0, gm.NONFINITE), np.zeros(300)),
             ("zero b, tol 0", A, np.zeros(300), 5, 10, 0.0, (0, 1, 0, gm.CONVERGED), np.zeros(300)),
             ("max_steps in mid-cycle", A, bi.rhs(300), 5, 7, 1e-300, (7, 2, 2, gm.MAX_STEPS), None))
    for name, M, rhs, restart, max_steps, tol, expect, x in cases:
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = restated(product, rhs, PLAIN, None, restart, max_steps, tol)
            assert want[:4] == expect, "%s: the restatement gives %r" % (name, want[:4])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, PLAIN, None, restart, max_steps, tol, every)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every), rhs if np.isfinite(rhs).all() else None)
                if x is not None:
                    assert_bits(got[6], x, name + ": d_x")
            H.close()
    x0 = start_vector(300)                                                            # a NaN in the first product leaves the start vector
    P = type("P", (), dict(first=None, second=None, m=pb.nan_m(300), triples=(None, pb.nan_m(300), None)))
    for fmt, a, b in BOTH:
        H, product = handle(torch, A, fmt, a, b)
        got = solve(torch, H, 300, bi.rhs(300), P, x0, 5, 10, 1e-10, 5)
        assert got[:4] == (1, 1, 0, gm.NONFINITE) and len(got[4]) == 1
        assert_bits(got[6], x0, "x_0 after NONFINITE by rule S1 at step 1")
        H.close()


def test_nonfinite_after_finite_columns_leaves_x_at_the_last_finite_columns(torch):
    """An m whose one huge element meets v_j only once the basis has reached that row (a NaN there would not wait: 0 * NaN is NaN):
    b = e_0 on the tridiagonal banded(40) fills one more row of the basis per step, so m_3 = 1e300 enters z at step 4, dot(w, w)
    overflows and h_5 is infinite: three finite columns, then rule S1, and x holds those three columns' update."""
    M = k13.matrix("banded", 40)
    rhs = np.zeros(40)
    rhs[0] = 1.0
    m = np.ones(40)
    m[3] = 1e300
    P = type("P", (), dict(first=None, second=None, m=m, triples=(None, m, None)))
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        want = restated(product, rhs, P, None, 10, 20, 1e-12)
        assert want[:4] == (4, 1, 3, gm.NONFINITE) and np.isfinite(want[6]).all() and np.abs(want[6]).max() > 0
        for every in (1, 3, 1000):
            same(solve(torch, H, 40, rhs, P, None, 10, 20, 1e-12, every), want, "NONFINITE at step 4, %s, check_every %d" % (fmt, every), rhs)
        H.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    L = A.trsv_plan(sm.TRSV_LOWER)
    b = torch.zeros(1, dtype=torch.float64, device="cuda")
    for H in (A, T):
        for first, m in ((None, None), (L, None), (None, b)):
            o, r = sm.gmres_opts(5), sm.GmresResult()
            C.memset(C.byref(r), 0x5a, C.sizeof(r))
            assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, first._t if first else None, sm._dev_ptr(m),
                                               None, C.byref(r), None, None, None) == sm.OK
            assert (r.steps, r.cycles, r.columns, r.reason) == (0, 0, 0, gm.CONVERGED)
            assert_bits([r.rr, r.bb], [0.0, 0.0], "n = 0")
    L.close()
    T.close()
    A.close()


# ==================================================================================================== 8. streams, state, refusals
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_stream_of_the_callers_with_the_operands_still_in_flight(torch, fmt, a, b):
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    P = k18.plans_of(torch, "sgs", Cs)
    rhs, x0 = bi.rhs(M.n), start_vector(M.n)
    side = torch.cuda.Stream()
    H, product = handle(torch, M, fmt, a, b)
    want = restated(product, rhs, P, x0, 6, 100, TOL)
    assert want[3] == gm.CONVERGED
    seen = []
    got = solve(torch, H, M.n, rhs, P, x0, 6, 100, TOL, 3, stream=side, before=so.solver_hook(torch, side, seen))
    assert seen and all(event.query() for event, _ in seen), "the call returned before the work on its stream had finished"
    same(got, want, "gmres with SGS, %s, everything in flight" % fmt, rhs)
    same(solve(torch, H, M.n, rhs, PLAIN, None, 6, 30, 0.0, 4, stream=side), restated(product, rhs, PLAIN, None, 6, 30, 0.0),
         fmt + ", plain, a stream of the caller's", rhs)
    H.close()
    P.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = k13.matrix("nonsym", 63, 20300 + 63)
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, rhs)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o, r, got = sm.gmres_opts(5, 1e-10, 10, 3), sm.GmresResult(), []
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, tr = np.full(6, SENTINEL), np.full(3, SENTINEL)
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)                                     # (keeps the captured graph from being empty)
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), None, None, None, C.byref(r),
                                                   sm._p(rr), sm._p(tr), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (tr == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, PLAIN, None, 3, 5, 1e-10, stream=s), restated(product, rhs, PLAIN, None, 3, 5, 1e-10),
         "outside a capture the same stream is fine", rhs)
    H.close()


def test_the_state_of_the_handle_and_of_the_plans_afterwards(torch):
    M, Cs = pb.case_of("nonsym(1003), coalesced")
    rhs = bi.rhs(M.n)
    x = start_vector(M.n, 4)
    for fmt, a, b in PATHS:
        P = k18.sgs_plans(torch, Cs)
        H, product = handle(torch, M, fmt, a, b)
        name = H.describe()
        dx = dev(torch, x)

        def look():
            out = []
            for _ in range(2):                               # (the tile kernel's sweep direction may alternate: two products)
                buf, dy = guarded_y(torch, M.n)
                if fmt == "tjds":
                    H.set_x(dx)                              # the permuted operand is the last vector's: a fresh set_x, as the header says
                H.spmv(*((dx, dy) if fmt == "csr" else (dy,)))
                torch.cuda.synchronize()
                check_guards(buf, M.n)
                out.append(dy.cpu().numpy())
            for T in (P.first, P.second):
                buf, dy = guarded_y(torch, M.n)
                T.solve(dx, dy)
                torch.cuda.synchronize()
                check_guards(buf, M.n)
                out.append(dy.cpu().numpy())
            return out

        before = look()
        infos = P.first.info(), P.second.info()
        first = solve(torch, H, M.n, rhs, P, None, 3, 7, 0.0, 2)
        assert H.describe() == name
        for got, want in zip(look(), before):
            assert_bits(got, want, "%s %d %d: a product or a solve after the call" % (fmt, a, b))
        for i, j in zip((P.first.info(), P.second.info()), infos):
            assert {k: v for k, v in i.items() if k != "build_ms"} == {k: v for k, v in j.items() if k != "build_ms"}
        same(solve(torch, H, M.n, rhs, P, None, 3, 7, 0.0, 2), first, "%s %d %d: the same call again" % (fmt, a, b), rhs)
        H.close()
        P.close()


def refused(torch, fn, h, n, o, first=None, second=None, result=True, b="own", x0=None, x="own", m=None):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    r = sm.GmresResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, tr = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), first._t if first is not None else None, sm._dev_ptr(m),
                               second._t if second is not None else None, C.byref(r) if result else None, sm._p(rr), sm._p(tr), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (tr == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def bad_opts():
    def o(**kw):
        v = sm.gmres_opts(5)
        for k, x in kw.items():
            setattr(v, k, x)
        return v
    return [None, o(struct_size=20), o(struct_size=0), o(max_steps=0), o(max_steps=-3), o(check_every=0), o(tol=-1e-300),
            o(tol=float("nan")), o(tol=float("inf")), o(restart=0), o(restart=65), o(restart=-1)]


def test_invalid_arguments_plans_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = k13.matrix("nonsym", 63, 20300 + 63)
    P = k18.sgs_plans(torch, trsv.of_matrix("nonsym(63)", M))
    other = k18.sgs_plans(torch, trsv.of_matrix("nonsym(64)", k13.matrix("nonsym", 64, 20300 + 64)))     # plans of another n
    L, U = P.first, P.second
    rhs = bi.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.gmres_opts(5, 1e-10, 10, 3)
    n = M.n
    dm = dev(torch, P.m)
    for fn, H, product, Wide in (("smvp_csr_gmres", A, pa, W), ("smvp_tjds_gmres", T, pt, WT)):
        assert refused(torch, fn, None, n, ok, L, U) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, H._h, n, o) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, n, ok, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=None) == sm.ERR_INVALID             # no d_b
        assert refused(torch, fn, H._h, n, ok, other.first, U) == sm.ERR_INVALID     # a plan of 64 rows
        assert b"first plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, None, other.second, m=dm) == sm.ERR_INVALID
        assert b"second plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, Wide._h, 4, ok) == sm.ERR_INVALID                  # rows != cols
        assert refused(torch, fn, H._h, n, ok, x=None) == sm.ERR_INVALID             # no d_x
        both_ = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")   # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, x0=both_[:n], x=both_[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, x0=both_[1:], x=both_[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, b=both_[:n], x=both_[:n]) == sm.ERR_INVALID      # d_b is d_x
        assert refused(torch, fn, H._h, n, ok, b=both_[1:], x=both_[:n]) == sm.ERR_INVALID
        for first, second in ((L, U), (None, None)):
            assert refused(torch, fn, H._h, n, ok, first, second, m=both_[:n], x=both_[:n]) == sm.ERR_INVALID      # d_m is d_x
            assert refused(torch, fn, H._h, n, ok, first, second, m=both_[1:], x=both_[:n]) == sm.ERR_INVALID
            assert b"d_m and d_x overlap" in sm.lib().smvp_last_error()
        assert (both_.cpu().numpy() == SENTINEL).all()
        for Q in (P, PLAIN):                                                           # all three NULL is accepted here
            same(solve(torch, H, n, rhs, Q, None, 3, 5, 1e-10), restated(product, rhs, Q, None, 3, 5, 1e-10),
                 fn + ": the handle after the refusals", rhs)
    for H in (A, T, W, WT):
        H.close()
    P.close()
    other.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = k13.matrix("nonsym", 1003)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    ok = sm.gmres_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_gmres", inner, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_gmres", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_gmres", T._h, M.n, ok) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, bi.rhs(M.n), PLAIN, None, 30, 2, 1e-10)[:4] == (2, 1, 2, gm.MAX_STEPS)
    T.close()


# ======================================================================================================= 9. through the Python methods
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_whole_use_through_the_python_methods_and_gmres_goes_on_where_bicgstab_breaks_down(torch, fmt, a, b):
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    H, product = handle(torch, M, fmt, a, b)
    A = H if fmt == "csr" else k18.handle_of(Cs)                                      # the plans stand on a CSR handle
    rhs = bi.rhs(M.n)
    db = dev(torch, rhs)
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    f = A.ilu0()
    first, second = f.plans()
    r, rr, tr = H.gmres(db, dx, first, second, restart=10, max_steps=60, tol=TOL, check_every=4)
    want = gm.run_rr(product, rhs, None, *pb.ilu0(Cs), 10, 60, TOL)
    assert (r.steps, r.cycles, r.columns, r.reason) == want[:4] and r.reason == sm.GMRES_CONVERGED and r.cycles > 1
    assert len(rr) == r.steps + 1 and len(tr) == r.cycles
    assert_bits(rr, want[4], "rr_each")
    assert_bits(tr, want[5], "restart_each")
    assert_bits([r.rr, r.bb], [want[7], bi.dot(rhs, rhs)], "the result block")
    assert_bits(dx.cpu().numpy(), want[6], "d_x")
    r, rr, tr = H.gmres(db, dx, max_steps=400, tol=TOL)                               # plain, the defaults: restart 30
    want = gm.run_rr(product, rhs, None, None, None, None, 30, 400, TOL)
    assert (r.steps, r.cycles, r.columns, r.reason) == want[:4] and r.reason == sm.GMRES_CONVERGED
    assert_bits(dx.cpu().numpy(), want[6], "plain: d_x")
    dm = torch.reciprocal(H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda")))
    x0 = dev(torch, start_vector(M.n))
    r, rr, tr = H.gmres(db, x0, m=dm, x0=x0, restart=64, max_steps=300, tol=TOL, check_every=1000, stream=torch.cuda.Stream())
    want = gm.run_rr(product, rhs, start_vector(M.n), None, dm.cpu().numpy(), None, 64, 300, TOL)
    assert (r.steps, r.cycles, r.columns, r.reason) == want[:4] and r.reason == sm.GMRES_CONVERGED
    assert_bits(x0.cpu().numpy(), want[6], "Jacobi: x0 given and aliased")
    # rule S1 at step 1: rr_each has one element, and the method knows
    S = sm.CsrMatrix(3, 3, np.array([0, 1, 1, 1], np.int32), np.zeros(1, np.int32), np.zeros(1))
    d3 = torch.empty(3, dtype=torch.float64, device="cuda")
    r, rr, tr = S.gmres(dev(torch, [1.0, 2.0, 3.0]), d3, restart=5, max_steps=10)
    assert (r.steps, r.cycles, r.columns, r.reason) == (1, 1, 0, sm.GMRES_BREAKDOWN) and len(rr) == 1 and len(tr) == 1
    S.close()
    # where BiCGSTAB breaks down at once (rule A on the swap), GMRES(2) solves
    W = sm.CsrMatrix(2, 2, *bi.swap2().csr)
    two, d2 = dev(torch, [1.0, 0.0]), torch.empty(2, dtype=torch.float64, device="cuda")
    assert W.bicgstab(two, d2)[0].reason == sm.BICGSTAB_BREAKDOWN
    r, rr, tr = W.gmres(two, d2, restart=2)
    assert (r.steps, r.reason) == (2, sm.GMRES_CONVERGED)
    assert_bits(d2.cpu().numpy(), [0.0, 1.0], "the swap solved")
    W.close()
    for bad in (dict(first=A), dict(second=first._t), dict(m=dm.cpu())):
        with pytest.raises(ValueError):
            H.gmres(db, dx, **bad)
    with pytest.raises(sm.SmvpError):
        H.gmres(db, dx, restart=65)
    for X in (first, second, f):
        X.close()
    if A is not H:
        A.close()
    H.close()


# =================================================================================== 10. resources and fresh memory, in a child process
SCRIPT = os.path.join(ROOT, "tests", "gmres_scenarios.py")
_crashed = []


@pytest.mark.parametrize("group", ["resources", "fresh"])
def test_the_call_gives_back_what_it_took_and_reads_no_fresh_memory(group):
    """tests/gmres_scenarios.py against lib/libsmvp_amd_counted.so, one child per group under one time limit, nothing retried: a
    successful call, every refusal and each obtaining call failing in turn leave the counters where they were; the same solves
    under test_gpu_fresh_memory.py's fill patterns give the same bits."""
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
