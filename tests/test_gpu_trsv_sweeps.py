"""GPU: Jacobi-sweep triangular solves as plans (smvp_csr_trsv_create_sweeps, kernel K21) against their restatement
tests/trsv_sweeps_method.py (test_trsv_sweeps_host.py pins that to hand-computed values, to trsv_method.solve and to a derived bound),
against the exact plans of K15 (levels - 1 sweeps are the exact solve, library against library), and inside the solvers of K16,
K18 and K19, which take the plans as they stand.

No tolerance anywhere: every element of every iterate has one right answer.  Comparisons are transposed.assert_bits (a NaN equals a
NaN whatever its sign and payload, an Inf's sign is one of its bits).  Every solve goes through test_gpu_trsv.solve_once(), which
gives d_x a guarded buffer poisoned with NaN, checks the guards and checks that d_b comes back unchanged."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cg_method as cg
import ilu0_method as ilu
import pbicgstab_method as pb
import pcg_method as pcg
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import test_gpu_cg as k12
import test_gpu_gmres as k19
import test_gpu_pbicgstab as k18
import test_gpu_pcg_tri as k16
import trsv_method as tm
import trsv_sweeps_method as ts
from conftest import ROOT
from parity import check_guards, guarded_y
from test_gpu_cg import AUTO, BOTH as BOTH_PATHS, SENTINEL, dev, handle
from test_gpu_resources import COUNTED, LIMIT_S, PKG
from test_gpu_transposed import inner_csr_handle
from test_gpu_trsv import N_CONSTRUCTED, N_EXISTING, chain_width, handle_of, products, solve_once, zero_diagonal
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu

BOTH = [(u, d) for u in (LOWER, UPPER) for d in (STORED, UNIT)]
SWEEPS = (0, 1, 2, 3, 7)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def held_bytes(n):
    """begin and end (ints), two scratch vectors (doubles): no array is shorter than four elements."""
    return max(n, 4) * (2 * 4 + 2 * 8)


def check_info(P, M, uplo, diag, sweeps, what):
    info, f = P.info(), M.facts(uplo, diag)
    for field in ("levels", "max_level_width", "missing_diagonals"):
        assert info[field] == f[field], "%s: %s is %r, the restatement's %r" % (what, field, info[field], f[field])
    assert info["entries"] == ts.entries(M, uplo, diag), what
    assert (info["launches"], info["chains"], info["chain_width"]) == (sweeps + 1 if M.n else 0, 0, 0), what
    assert info["lanes_per_row"] in (2, 4, 8, 16, 32, 64) and info["plan_bytes"] == held_bytes(M.n) and info["build_ms"] >= 0.0
    level_ptr, order = P.schedule()
    assert level_ptr.tolist() == f["level_ptr"].tolist() and order.tolist() == f["order"].tolist(), what
    assert P.sweeps == sweeps
    return info


def check_case(torch, M, sweeps=SWEEPS):
    """Every sweep count on both triangles and both diagonal kinds of M: a first solve, a second with another b on the same plan
    (an iterate left in a scratch vector would show), one on a caller's stream, one with d_x == d_b.  Odd and even counts end on
    either scratch vector."""
    H = handle_of(M)
    b1 = tm.rhs(M.n)
    b2 = tm.rhs(M.n, 2100 + M.n % 89)
    for uplo, diag in BOTH:
        want1, want2 = (ts.iterates(M, uplo, diag, b, max(sweeps)) for b in (b1, b2))
        for s in sweeps:
            what = "%s, uplo %d, diag %d, %d sweeps" % (M.name, uplo, diag, s)
            P = H.trsv_plan(uplo, diag, sweeps=s)
            info = check_info(P, M, uplo, diag, s, what)
            assert_bits(solve_once(torch, P, M.n, b1), want1[s], what)
            assert_bits(solve_once(torch, P, M.n, b2), want2[s], what + ": another b on the same plan")
            assert_bits(solve_once(torch, P, M.n, b1, stream=torch.cuda.Stream()), want1[s], what + ": on a stream of the caller's")
            assert_bits(solve_once(torch, P, M.n, b2, alias=True), want2[s], what + ": d_x is d_b")
            P.close()
        print("%s, uplo %d, diag %d: %d rows, %d entries in the ranges (%d count), %d levels, %d lanes a row"
              % (M.name, uplo, diag, M.n, info["entries"], M.facts(uplo, diag)["entries"], info["levels"], info["lanes_per_row"]))
    H.close()


# ============================================================================================ 1. bits against the restatement
@pytest.mark.parametrize("i", range(N_EXISTING))
def test_every_element_is_the_restatements_on_every_existing_case(torch, i):
    """spd_long and memplus: rows of 700 and 574 entries, further passes, ranges that end inside a lane's chunk; spd_shuffled:
    loose ranges, unsorted columns, repeats; pdp08-pg4: a missing diagonal (NaN and Inf, compared as such)."""
    check_case(torch, tm.existing_cases()[i])


@pytest.mark.parametrize("i", range(N_CONSTRUCTED))
def test_every_element_is_the_restatements_on_every_constructed_case(torch, i):
    """n = 1, 2, w - 1, w, w + 1, 3w + 5: the edges of a group, a wavefront and a workgroup; dense_lower(70), divergent: long rows
    beside short ones; the leveled cases: shuffled rows; every level-0 row under DIAG_UNIT has an empty range and x_i = b_i."""
    check_case(torch, tm.constructed_cases(chain_width())[i])


def test_the_additions_follow_the_stored_order(torch):
    M = tm.order_dependent()
    S = tm.sorted_copy(M)
    a, b = ts.solve(M, LOWER, STORED, M.b, 1), ts.solve(S, LOWER, STORED, S.b, 1)
    assert (a.view(np.int64) != b.view(np.int64)).any(), "the order shows in the restatement"
    for X in (M, S):
        H = handle_of(X)
        for s in (0, 1, 2):
            P = H.trsv_plan(LOWER, STORED, sweeps=s)
            assert_bits(solve_once(torch, P, X.n, X.b), ts.solve(X, LOWER, STORED, X.b, s), "%s, %d sweeps" % (X.name, s))
            P.close()
        H.close()


# ================================================================================================ 2. library against library
def library_cases():
    w = chain_width()
    return (tm.bidiagonal(257), tm.interleaved(2 * w), tm.wide_thin_wide(w), tm.existing_cases()[6], tm.of_matrix("lap2d(32)", tri.lap2d(32)))


@pytest.mark.parametrize("i", range(5))
def test_levels_less_one_sweeps_are_the_exact_plans_bits(torch, i):
    M = library_cases()[i]
    H = handle_of(M)
    for uplo, diag in BOTH:
        E = H.trsv_plan(uplo, diag)
        levels = E.info()["levels"]
        P = H.trsv_plan(uplo, diag, sweeps=levels - 1)
        assert P.info()["levels"] == levels and P.info()["launches"] == levels and E.sweeps is None
        b = tm.rhs(M.n, 22)
        want = solve_once(torch, E, M.n, b)
        assert_bits(solve_once(torch, P, M.n, b), want, "%s, uplo %d, diag %d: %d sweeps against the exact plan" % (M.name, uplo, diag, levels - 1))
        assert_bits(want, tm.solve(M, uplo, diag, b), "the exact plan against its restatement")
        P.close()
        E.close()
    H.close()
    if i == 3:
        assert M.name == "memplus" and M.facts(LOWER, STORED)["levels"] == 174


# ================================================================================================================ 3. non-finite
def test_zero_and_missing_diagonals_give_the_restatements_infinities_and_nans(torch):
    P8 = tm.existing_cases()[-1]
    assert P8.name == "pdp08-pg4" and P8.facts(LOWER, STORED)["missing_diagonals"] == 1
    seen = {"inf": 0, "nan": 0}
    for M in (zero_diagonal(), P8):
        H = handle_of(M)
        b = tm.rhs(M.n)
        for uplo in (LOWER, UPPER):
            exact = max(M.facts(uplo, STORED)["levels"] - 1, 3)                        # (the exact solve's NaNs; an early iterate holds Infs only)
            wants = ts.iterates(M, uplo, STORED, b, exact)
            for s in (0, 1, 3, exact):
                want = wants[s]
                assert not np.isfinite(want).all() and np.isfinite(want).any(), "%s: some of x is finite, some is not" % M.name
                P = H.trsv_plan(uplo, STORED, sweeps=s)
                got = solve_once(torch, P, M.n, b)
                fin = np.isfinite(want)
                assert_bits(got[fin], want[fin], "%s, uplo %d, %d sweeps: where the restatement is finite" % (M.name, uplo, s))
                assert (np.isinf(got) == np.isinf(want)).all() and (got[np.isinf(want)] == want[np.isinf(want)]).all(), "Inf positions and signs"
                assert (np.isnan(got) == np.isnan(want)).all(), "NaN positions"
                seen["inf"] += int(np.isinf(want).sum())
                seen["nan"] += int(np.isnan(want).sum())
                P.close()
        H.close()
    assert seen["inf"] and seen["nan"], seen


# ============================================================================================================ 4. plan behaviour
def test_adopted_values_changed_in_place_are_seen_without_a_new_plan(torch):
    M = tm.existing_cases()[0]
    rp, ci, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in M.csr)
    H = sm.CsrMatrix(M.n, M.n, rp, ci, v)
    plans = {k: H.trsv_plan(*k, sweeps=3) for k in BOTH}
    b = tm.rhs(M.n, 23)
    for k, P in plans.items():
        assert_bits(solve_once(torch, P, M.n, b), ts.solve(M, *k, b, 3), "adopted arrays, uplo %d, diag %d" % k)
    v.mul_(-3.0)
    torch.cuda.synchronize()
    M3 = tm.Case.of_csr("spd(1003) * -3", M.n, M.csr[0], M.csr[1], M.csr[2] * -3.0)
    for k, P in plans.items():
        want = ts.solve(M3, *k, b, 3)
        assert not np.array_equal(want, ts.solve(M, *k, b, 3))
        assert_bits(solve_once(torch, P, M.n, b), want, "values changed in place, uplo %d, diag %d" % k)
        P.close()
    H.close()


def test_the_handles_state_is_left_alone(torch):
    M = tm.existing_cases()[6]                                                        # memplus
    H = handle_of(M)
    name = H.describe()
    dx = dev(torch, tm.rhs(M.n, 17))
    before = products(torch, H, M.n, dx)
    L, U = H.trsv_plan(LOWER, sweeps=2), H.trsv_plan(UPPER, UNIT, sweeps=5)
    for a, b in zip(products(torch, H, M.n, dx), before):
        assert_bits(a, b, "a product after create")
    b = tm.rhs(M.n, 24)
    assert_bits(solve_once(torch, L, M.n, b), ts.solve(M, LOWER, STORED, b, 2), "lower")
    assert_bits(solve_once(torch, U, M.n, b), ts.solve(M, UPPER, UNIT, b, 5), "upper, beside the lower plan")
    for a, b_ in zip(products(torch, H, M.n, dx), before):
        assert_bits(a, b_, "a product after the solves")
    L.close()
    U.close()
    assert H.describe() == name
    for a, b_ in zip(products(torch, H, M.n, dx), before):
        assert_bits(a, b_, "a product after the plans are destroyed")
    H.close()


def test_a_solve_is_captured_as_a_plans_first_call(torch):
    for M, uplo, s in ((tm.wide_thin_wide(chain_width()), LOWER, 3), (tm.existing_cases()[5], UPPER, 4), (tm.existing_cases()[5], LOWER, 0)):
        H = handle_of(M)
        P = H.trsv_plan(uplo, STORED, sweeps=s)                                       # outside the capture: it copies back and allocates
        b = tm.rhs(M.n, 25)
        want = ts.solve(M, uplo, STORED, b, s)
        db = dev(torch, b)
        buf, dx = guarded_y(torch, M.n)
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                rc = sm.lib().smvp_trsv_solve(P._t, sm._dev_ptr(db), sm._dev_ptr(dx), st.cuda_stream)
        assert rc == sm.OK, sm.lib().smvp_last_error().decode()
        for _ in range(2):
            dx.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dx.cpu().numpy(), want, "%s: the replayed capture of %d sweeps" % (M.name, s))
        assert_bits(db.cpu().numpy(), b, "d_b")
        del g
        P.close()
        H.close()


def test_symmetric_gauss_seidel_is_captured_from_two_sweep_plans_of_one_handle(torch):
    """z = U^-1 (d o (L^-1 r)), each solve three sweeps: the lower and the upper plan of one handle back to back, torch.mul between."""
    M = tm.existing_cases()[3]                                                        # tridiagonal(300)
    d = pcg.diagonal_csr(M.n, M.n, *M.csr)
    r = tm.rhs(M.n, 16)
    t1 = ts.solve(M, LOWER, STORED, r, 3)
    want = ts.solve(M, UPPER, STORED, t1 * d, 3)
    H = handle_of(M)
    L, U = H.trsv_plan(LOWER, sweeps=3), H.trsv_plan(UPPER, sweeps=3)
    dd, dr = dev(torch, d), dev(torch, r)
    dt = torch.empty(M.n, dtype=torch.float64, device="cuda")
    buf, dz = guarded_y(torch, M.n)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            L.solve(dr, dt, stream=st)
            torch.mul(dt, dd, out=dt)
            U.solve(dt, dz, stream=st)
    for _ in range(2):
        dz.fill_(float("nan"))
        dt.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        assert_bits(dz.cpu().numpy(), want, "the replayed symmetric Gauss-Seidel application")
    assert_bits(dr.cpu().numpy(), r, "r")
    del g
    L.close()
    U.close()
    H.close()


def test_create_refuses_a_capturing_stream_and_the_capture_stays_valid(torch):
    M = tm.existing_cases()[4]
    H = handle_of(M)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    st = torch.cuda.Stream()
    out, got = C.c_void_p(), []
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            dZ.add_(1.0)
            got.append(sm.lib().smvp_csr_trsv_create_sweeps(C.byref(out), H._h, LOWER, STORED, 3, st.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg and "smvp_csr_trsv_create_sweeps" in msg and out.value is None
    g.replay()
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16
    del g
    H.close()


# ======================================================================================================================= 5. info
def test_info_sweeps_and_a_matrix_without_rows(torch):
    M = tm.existing_cases()[2]                                                        # spd_shuffled: loose ranges
    H = handle_of(M)
    assert ts.entries(M, LOWER, STORED) > M.facts(LOWER, STORED)["entries"]
    for s in (0, 1, 4096):
        P = H.trsv_plan(LOWER, STORED, sweeps=s)
        check_info(P, M, LOWER, STORED, s, "spd_shuffled, %d sweeps" % s)
        P.close()
    E = H.trsv_plan(LOWER)
    n = C.c_int(7)
    assert sm.lib().smvp_trsv_sweeps(E._t, C.byref(n)) == sm.OK and n.value == -1 and E.sweeps is None
    assert sm.lib().smvp_trsv_sweeps(E._t, None) == sm.ERR_INVALID
    E.close()
    for sweeps in (-1, 4097):
        with pytest.raises(sm.SmvpError):
            H.trsv_plan(LOWER, sweeps=sweeps)
    H.close()
    Z = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for uplo, diag in BOTH:
        P = Z.trsv_plan(uplo, diag, sweeps=3)
        info = P.info()
        assert (info["levels"], info["launches"], info["chains"], info["max_level_width"], info["entries"], info["missing_diagonals"]) == (0,) * 6
        assert info["plan_bytes"] == held_bytes(0) and P.sweeps == 3
        level_ptr, order = P.schedule()
        assert level_ptr.tolist() == [0] and order.tolist() == []
        assert sm.lib().smvp_trsv_solve(P._t, None, None, None) == sm.OK
        x = torch.empty(0, dtype=torch.float64, device="cuda")
        assert P.solve(x, x) is x
        P.close()
    Z.close()


# =================================================================================================================== 6. refusals
def test_invalid_arguments_are_refused_and_nothing_is_written(torch):
    L_ = sm.lib()
    M = tm.existing_cases()[4]                                                        # ibm32
    n = M.n
    H = handle_of(M)
    out = C.c_void_p()
    for uplo, diag, sweeps, word in ((2, STORED, 3, "uplo"), (LOWER, 2, 3, "diag"), (LOWER, STORED, -1, "sweeps"), (LOWER, STORED, 4097, "sweeps")):
        assert L_.smvp_csr_trsv_create_sweeps(C.byref(out), H._h, uplo, diag, sweeps, None) == sm.ERR_INVALID
        assert word in L_.smvp_last_error().decode() and out.value is None
    R = sm.CsrMatrix(3, 4, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 3], np.int32), np.ones(3))
    assert L_.smvp_csr_trsv_create_sweeps(C.byref(out), R._h, LOWER, STORED, 3, None) == sm.ERR_INVALID
    assert b"square" in L_.smvp_last_error() and out.value is None
    R.close()
    P = H.trsv_plan(LOWER, sweeps=3)
    buf = torch.full((2 * n + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    assert L_.smvp_trsv_solve(P._t, None, sm._dev_ptr(buf[:n]), None) == sm.ERR_INVALID and b"d_b" in L_.smvp_last_error()
    assert L_.smvp_trsv_solve(P._t, sm._dev_ptr(buf[:n]), None, None) == sm.ERR_INVALID and b"d_x" in L_.smvp_last_error()
    for shift in (1, -1, n - 1):                                                       # d_x one element off d_b, either way; one shared
        b0 = 1 if shift < 0 else 0
        assert L_.smvp_trsv_solve(P._t, sm._dev_ptr(buf[b0:b0 + n]), sm._dev_ptr(buf[b0 + shift:b0 + shift + n]), None) == sm.ERR_INVALID
        assert b"overlap" in L_.smvp_last_error()
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all(), "a refused call wrote something"
    b = tm.rhs(n, 26)
    assert_bits(solve_once(torch, P, n, b), ts.solve(M, LOWER, STORED, b, 3), "after the refusals the plan solves")
    P.close()
    H.close()


def test_unsupported_handles_are_refused(torch):
    L_ = sm.lib()
    A = cg.spd(1003)
    out = C.c_void_p()
    T = sm.TjdsMatrix(sm.tjds_from_coo(A.coo, A.n, A.n))
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_x(dev(torch, np.ones(A.n)))
    T.spmv(torch.empty(A.n, dtype=torch.float64, device="cuda"))                      # (the row-gather plan and its inner handle exist)
    torch.cuda.synchronize()
    inner = inner_csr_handle(T, A.n, A.n, A.nnz)                                      # a CSR handle that is not plain CSR
    assert L_.smvp_csr_trsv_create_sweeps(C.byref(out), inner, LOWER, STORED, 3, None) == sm.ERR_UNSUPPORTED
    assert b"plain CSR" in L_.smvp_last_error() and out.value is None
    T.close()
    row_ptr, col_ind, val = A.csr
    lo, hi = 100, 400
    block = (row_ptr[lo:hi + 1] - row_ptr[lo]).astype(np.int32)
    B = sm.CsrMatrix(hi - lo, A.n, block, col_ind[row_ptr[lo]:row_ptr[hi]], val[row_ptr[lo]:row_ptr[hi]], first_row=lo)
    assert L_.smvp_csr_trsv_create_sweeps(C.byref(out), B._h, LOWER, STORED, 3, None) == sm.ERR_UNSUPPORTED
    assert b"first_row" in L_.smvp_last_error() and out.value is None
    with pytest.raises(sm.SmvpError):
        B.trsv_plan(UPPER, sweeps=2)
    B.close()


# ==================================================================================================================== 7. solvers
class Swept:
    """A preconditioner on the device for the solvers' solve() helpers -- first, second, m -- and the restatement's triples:
    symmetric Gauss-Seidel on the Case's own handle with m = diagonal(), or the library's ILU(0) of it.  sweeps: None (exact plans),
    an int, or "levels": as many as make both plans exact, the larger levels - 1 of the two."""

    def __init__(self, torch, kind, Cs, sweeps):
        self.A = k18.handle_of(Cs)
        self.f = self.A.ilu0() if kind == "ilu0" else None
        self.triples = pb.ilu0(Cs) if kind == "ilu0" else pb.sgs(Cs)
        self.m = None if kind == "ilu0" else self.A.diagonal(torch.empty(Cs.n, dtype=torch.float64, device="cuda")).cpu().numpy()
        if sweeps == "levels":
            exact = self.make(None)
            sweeps = max(T.info()["levels"] for T in exact) - 1
            for T in exact:
                T.close()
        self.sweeps = sweeps
        self.first, self.second = self.make(sweeps)

    def make(self, sweeps):
        if self.f is not None:
            return self.f.plans(sweeps=sweeps)
        return self.A.trsv_plan(LOWER, STORED, sweeps=sweeps), self.A.trsv_plan(UPPER, STORED, sweeps=sweeps)

    def close(self):
        self.first.close()
        self.second.close()
        if self.f is not None:
            self.f.close()
        self.A.close()


def swept_solve(sweeps):
    """pcg_tri_method._solve with trsv_sweeps_method.solve in place of the exact substitution: the one place through which the
    restatements of K16, K18 and K19 apply a plan."""
    seen = {}

    def _solve(plan, b):
        M, uplo, diag = plan
        key = (id(M), uplo, diag, b.tobytes())
        if key not in seen:
            x = ts.solve(M, uplo, diag, b, sweeps)
            x.setflags(write=False)
            seen[key] = (M, x)
        return seen[key][1]

    return _solve


def solver_system(name):
    """(the product's matrix, the Case the plans stand on): coalesced Cases, so that ILU(0) accepts them."""
    if name == "convdiff(32, 0.5)":
        return pb.case_of(name)
    if name == "nonsym(1003)":
        return pb.case_of("nonsym(1003), coalesced")
    Cs = {"spd(1003)": ilu.spd_1003, "lap2d(32)": lambda: ilu.grid(32)}[name]()
    return ilu.as_matrix(Cs), Cs


SOLVERS = [("pcg_tri", name, kind) for name in ("spd(1003)", "lap2d(32)") for kind in ("sgs", "ilu0")]
SOLVERS += [(solver, name, kind) for solver in ("pbicgstab", "gmres 5", "gmres 30") for name in ("convdiff(32, 0.5)", "nonsym(1003)")
            for kind in ("sgs", "ilu0")]
STEPS, TOL = 80, 1e-8


def library_run(torch, solver, H, n, b, P, every=7):
    if solver == "pcg_tri":
        return k16.solve(torch, H, n, b, P, None, STEPS, TOL, every)
    if solver == "pbicgstab":
        return k18.solve(torch, H, n, b, P, None, STEPS, TOL, every)
    return k19.solve(torch, H, n, b, P, None, int(solver.split()[1]), STEPS, TOL, every)


def restated_run(solver, product, b, P):
    if solver == "pcg_tri":
        return tri.run(product, b, None, *P.triples, STEPS, TOL)
    if solver == "pbicgstab":
        return pb.run(product, b, None, *P.triples, STEPS, TOL)
    return k19.restated(product, b, P, None, int(solver.split()[1]), STEPS, TOL)


def same_of(solver):
    return {"pcg_tri": k16.same, "pbicgstab": k18.same}.get(solver, k19.same)


def all_bits(got, want, what):
    """Two runs of the library: every returned number, the result block's doubles included."""
    assert len(got) == len(want)
    for j, (a, b) in enumerate(zip(got, want)):
        if isinstance(a, np.ndarray):
            assert_bits(a, b, "%s: element %d of the result" % (what, j))
        elif isinstance(a, np.floating):
            assert_bits([a], [b], "%s: element %d of the result" % (what, j))
        else:
            assert a == b, "%s: element %d of the result is %r against %r" % (what, j, a, b)


@pytest.mark.parametrize("solver,name,kind", SOLVERS)
def test_solvers_with_levels_less_one_sweeps_return_the_exact_plans_numbers(torch, solver, name, kind):
    """(a) library against library: the counts, the reason, all histories, every bit of x."""
    M, Cs = solver_system(name)
    H, _ = handle(torch, M, "csr", *AUTO)
    b = cg.rhs(M.n)
    E, P = Swept(torch, kind, Cs, None), Swept(torch, kind, Cs, "levels")
    assert P.first.sweeps == P.second.sweeps == P.sweeps >= 1 and E.first.sweeps is None
    want = library_run(torch, solver, H, M.n, b, E)
    all_bits(library_run(torch, solver, H, M.n, b, P), want, "%s on %s with %s, %d sweeps" % (solver, name, kind, P.sweeps))
    print("%s on %s with %s: %d sweeps are exact; %r" % (solver, name, kind, P.sweeps, want[:4]))
    for X in (E, P):
        X.close()
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH_PATHS)
@pytest.mark.parametrize("solver,name,kind", SOLVERS)
def test_solvers_with_three_sweeps_return_the_wrapped_restatements_numbers(torch, monkeypatch, solver, name, kind, fmt, a, b):
    """(b) every number against the restatement of the solver, its plans applied by trsv_sweeps_method.solve."""
    monkeypatch.setattr(tri, "_solve", swept_solve(3))
    M, Cs = solver_system(name)
    H, product = handle(torch, M, fmt, a, b)
    rhs = cg.rhs(M.n)
    P = Swept(torch, kind, Cs, 3)
    want = restated_run(solver, product, rhs, P)
    for every in (1, 10):
        got = library_run(torch, solver, H, M.n, rhs, P, every)
        same_of(solver)(got, want, "%s on %s with %s, three sweeps, %s %d %d, check_every %d" % (solver, name, kind, fmt, a, b, every), rhs)
    print("%s on %s with %s, three sweeps: %r" % (solver, name, kind, tuple(want[:4])))
    P.close()
    H.close()


@pytest.mark.parametrize("fmt,a,b", BOTH_PATHS)
def test_three_sgs_sweeps_take_fewer_steps_than_plain_cg_on_the_grid(torch, monkeypatch, fmt, a, b):
    """(c) lap2d(32) at tol 1e-8: both counts are the restatement's, and the library's are equal to them."""
    monkeypatch.setattr(tri, "_solve", swept_solve(3))
    M, Cs = solver_system("lap2d(32)")
    H, product = handle(torch, M, fmt, a, b)
    rhs = cg.rhs(M.n)
    P = Swept(torch, "sgs", Cs, 3)
    plain, swept = cg.run(product, rhs, None, 300, TOL), tri.run(product, rhs, None, *P.triples, 300, TOL)
    assert plain[2] == cg.CONVERGED and swept[2] == tri.CONVERGED
    got_plain, got_swept = k12.solve(torch, H, M.n, rhs, None, 300, TOL), k16.solve(torch, H, M.n, rhs, P, None, 300, TOL)
    k12.same(got_plain, plain, "plain cg", rhs)
    k16.same(got_swept, swept, "pcg_tri with three SGS sweeps", rhs)
    print("lap2d(32), tol 1e-8: cg %d steps, pcg_tri with three SGS sweeps %d" % (plain[0], swept[0]))
    assert got_swept[0] == swept[0] < plain[0] == got_plain[0]
    P.close()
    H.close()


# ================================================================================================================== 8. resources
SCRIPT = os.path.join(ROOT, "tests", "trsv_sweeps_scenarios.py")


@pytest.mark.parametrize("group", ("balance", "refused", "plan_bytes"))
def test_a_sweeps_plan_gives_back_what_it_took(group):
    """Child processes on the counted build, in the manner of test_gpu_resources.py: create / solve / destroy balance exactly, a
    create whose k-th device allocation is refused returns an error and holds nothing, plan_bytes is what is held."""
    if not os.path.exists(COUNTED):
        subprocess.check_call(["make", "-C", PKG, "lib/libsmvp_amd_counted.so"])
    env = dict(os.environ, SMVP_LIB_PATH=COUNTED)
    p = subprocess.run([sys.executable, SCRIPT, group], env=env, capture_output=True, text=True, timeout=LIMIT_S)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and ("group %s ok" % group) in p.stdout, \
        "group %s: exit status %d\n%s\n%s" % (group, p.returncode, p.stdout[-6000:], p.stderr[-3000:])
