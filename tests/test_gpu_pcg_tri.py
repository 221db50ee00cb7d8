"""GPU: conjugate gradients preconditioned by two triangular solves (smvp_csr_pcg_tri / smvp_tjds_pcg_tri, kernel K16) against their
numpy restatement tests/pcg_tri_method.py (test_pcg_tri_host.py pins that to hand-computed values and known answers).

No tolerance anywhere.  z = M^-1 r is two of K15's solves, each element the serial substitution loop's, and one rounded
multiplication; the header fixes the order of every addition of the dot; everything else is one rounded IEEE operation per element,
and the restatement's product argument is the SAME handle's single product (test_gpu_cg.handle): on every path whose product is the
same from run to run, steps, updates, reason, rr, rz, bb, the three histories and every bit of d_x have one right answer.
Comparisons are transposed.assert_bits on the uint64 views.  Every solver call goes through solve() below, which gives d_x a
guarded buffer, checks the guards, checks that d_b and d_m come back unchanged and that the histories keep a sentinel beyond the
filled elements.  The serial substitution in Python is the reference, so n stays at about 3000 at the most wherever it runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import cg_method as cg
import pcg_method as pcg
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import test_gpu_pcg as k14
import trsv_method as trsv
from parity import check_guards, guarded_y
from test_gpu_cg import AUTO, BOTH, PATHS, SENTINEL, bad_opts, dev, handle, start_vector
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

MAX_STEPS = 60
TOL = 1e-8
same = k14.same


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def fn_of(H):
    return "smvp_%s_pcg_tri" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds")


class Plans:
    """The restatement's (first, m, second) on the device: a CsrMatrix per Case, a TrsvPlan per triple."""

    def __init__(self, first, m, second):
        self.triples, self.m = (first, m, second), m
        self.handles = {}
        for Cs in (first[0], second[0]):
            if id(Cs) not in self.handles:
                self.handles[id(Cs)] = sm.CsrMatrix(Cs.n, Cs.n, *Cs.csr)
        self.first = self.handles[id(first[0])].trsv_plan(first[1], first[2])
        self.second = self.handles[id(second[0])].trsv_plan(second[1], second[2])

    def run(self, product, b, x0, max_steps, tol):
        first, m, second = self.triples
        return tri.run(product, b, x0, first, m, second, max_steps, tol)

    def close(self):
        self.first.close()
        self.second.close()
        for H in self.handles.values():
            H.close()


def solve(torch, H, n, b, P, x0, max_steps, tol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, updates, reason, rr_each, rz_each, sigma_each, x, rr, rz, bb): pcg_tri_method.run's
    tuple, then the result block's three doubles.  P: a Plans, or anything with first, second (TrsvPlans) and m (numpy or None).
    alias: d_x is d_x0.  Nothing is synchronised after the call: it returns when the work is done.
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
    o, r = sm.cg_opts(max_steps, tol, every), sm.PcgResult()
    rr, rz, sigma = np.full(max_steps + 1, SENTINEL), np.full(max_steps + 1, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0, m=dm)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx), P.first._t, sm._dev_ptr(dm),
                                     P.second._t, C.byref(r), sm._p(rr), sm._p(rz), sm._p(sigma), sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    if dm is not None:
        assert_bits(dm.cpu().numpy(), P.m, "d_m after the call")
    assert 0 <= r.updates <= r.steps <= max_steps and r.pad == 0
    for h, filled, name in ((rr, r.updates + 1, "rr_each"), (rz, r.updates + 1, "rz_each"), (sigma, r.steps, "sigma_each")):
        assert (h[filled:] == SENTINEL).all(), name + " was written beyond its filled elements"
        assert not (h[:filled] == SENTINEL).any(), "an element of %s was not filled" % name
    return (r.steps, r.updates, r.reason, rr[:r.updates + 1], rz[:r.updates + 1], sigma[:r.steps], x, np.float64(r.rr), np.float64(r.rz),
            np.float64(r.bb))


# ================================================================================================= 1. bits against run(), every path
@functools.lru_cache(maxsize=None)
def system(name):
    """(the product's matrix, the Case the plans stand on): built once and left unchanged.  The Case holds the matrix's own CSR
    arrays; spd_shuffled's holds the entries AS STORED (unsorted columns, repeats)."""
    M = {"scaled(1003)": lambda: k14.matrix("scaled", 1003), "spd(3001)": lambda: k14.matrix("spd", 3001), "lap2d(32)": lambda: tri.lap2d(32),
         "spd_shuffled": lambda: k14.matrix("spd_shuffled"), "spd_long": lambda: k14.matrix("spd_long")}[name]()
    return M, trsv.of_matrix(name, M, as_stored=name == "spd_shuffled")


SYSTEMS = ("scaled(1003)", "spd(3001)", "lap2d(32)", "spd_shuffled", "spd_long")


def test_the_systems_schedules_are_what_their_choice_rests_on(torch):
    """scaled(1003): thin levels only, each solve one chain; spd(3001): wide launches hand over to a chain inside a step;
    lap2d(32): 63 levels; spd_shuffled: rows whose columns are not ascending; spd_long: rows of 700 entries."""
    info = {}
    for name in SYSTEMS:
        M, Cs = system(name)
        P = Plans(*tri.sgs(Cs))
        info[name] = P.first.info(), P.second.info()
        print(name, info[name][0])
        P.close()
    for i in info["scaled(1003)"]:
        assert i["max_level_width"] <= i["chain_width"] and i["launches"] == i["chains"] == 1
    for i in info["spd(3001)"]:
        assert i["max_level_width"] > i["chain_width"] and i["launches"] > i["chains"] >= 1
    assert info["lap2d(32)"][0]["levels"] == info["lap2d(32)"][1]["levels"] == 63
    row_ptr, col_ind, val = system("spd_shuffled")[1].csr
    assert any((np.diff(col_ind[a:z]) <= 0).any() for a, z in zip(row_ptr[:-1], row_ptr[1:]))
    assert np.diff(system("spd_long")[1].csr[0]).max() >= 700


@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name in SYSTEMS:
        M, Cs = system(name)
        P = Plans(*tri.sgs(Cs))
        H, product = handle(torch, M, fmt, a, b)
        rhs, x0 = cg.rhs(M.n), start_vector(M.n)
        want = {None: P.run(product, rhs, None, MAX_STEPS, TOL), "x0": P.run(product, rhs, x0, MAX_STEPS, TOL)}
        for key, every, alias in ((None, 1, False), (None, 7, False), ("x0", 7, False), ("x0", 1000, True), ("x0", 1, True)):
            what = "%s, %s %d %d, x0 %s%s, check_every %d" % (name, fmt, a, b, key, ", d_x is d_x0" if alias else "", every)
            got = solve(torch, H, M.n, rhs, P, x0 if key else None, MAX_STEPS, TOL, every, alias=alias)
            same(got, want[key], what, rhs)
        w = want[None]
        print("%s, %s %d %d: steps %d, updates %d, reason %d, rr %r, rz %r" % (name, fmt, a, b, w[0], w[1], w[2], float(w[3][-1]), float(w[4][-1])))
        assert w[2] == tri.CONVERGED and w[0] < MAX_STEPS, "%s: the restatement did not converge" % name
        same(solve(torch, H, M.n, rhs, P, None, 6, 0.0, 4), P.run(product, rhs, None, 6, 0.0), name + ", tol 0", rhs)
        H.close()
        P.close()


# ========================================================================== 2. diagonal-only plans are smvp_*_pcg on the GPU, bit for bit
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_diagonal_only_plans_are_the_librarys_jacobi_pcg(torch, fmt, a, b):
    """The last case has an m of ones between the solves -- a multiplication that changes no bit -- at n = 4 * 2048 * 256 + 1, where
    the four-deep bodies of the passes that write, the scaling's among them, run and leave one tail trip."""
    for name, args, steps, tol, ones in (("spd", (1003,), 30, 1e-10, False), ("spd_long", (), 30, 1e-10, False),
                                         ("tridiagonal", (cg.TRIP + 1,), 4, 0.0, False), ("tridiagonal", (4 * cg.TRIP + 1,), 3, 0.0, True)):
        M = k14.matrix(name, *args)
        d = k14.jacobi(name, *args)                                                  # (no serial substitution here: two library calls are compared)
        D = sm.CsrMatrix(M.n, M.n, np.arange(M.n + 1, dtype=np.int32), np.arange(M.n, dtype=np.int32), d)
        P = type("P", (), dict(first=D.trsv_plan(tri.LOWER, tri.STORED), second=D.trsv_plan(tri.UPPER, tri.UNIT),
                               m=np.ones(M.n) if ones else None))
        H, product = handle(torch, M, fmt, a, b)
        rhs = cg.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            jacobi = k14.solve(torch, H, M.n, rhs, d, x0, steps, tol, 3)
            got = solve(torch, H, M.n, rhs, P, x0, steps, tol, 3)
            what = "%s, %s, x0 %s" % (name, fmt, "NULL" if x0 is None else "random")
            assert got[:3] == jacobi[:3], what
            for i, field in ((3, "rr_each"), (4, "rz_each"), (5, "sigma_each"), (6, "d_x")):
                assert_bits(got[i], jacobi[i], "%s: %s" % (what, field))
            assert_bits(list(got[7:]), list(jacobi[7:]), what + ": rr, rz, bb")
        assert got[0] > 1
        H.close()
        P.first.close()
        P.second.close()
        D.close()


# ==================================================================================================================== 3. sizes
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_sizes_around_a_workgroup(torch, n):
    M = k14.matrix("spd", n, 20280 + n)
    P = Plans(*tri.sgs(trsv.of_matrix("spd(%d)" % n, M)))
    rhs = cg.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            same(solve(torch, H, n, rhs, P, x0, 12, 1e-10, 5), P.run(product, rhs, x0, 12, 1e-10), "spd(%d), %s" % (n, fmt), rhs)
        H.close()
    P.close()


# ======================================================================================================= 4. a factor the caller brings
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_an_incomplete_factor_and_its_transposed_handle_without_an_m(torch, fmt, a, b):
    M = tri.lap2d(16)
    F, Ft = tri.ic0(M)
    HF = sm.CsrMatrix(F.n, F.n, *F.csr)
    HFt = HF.transposed()
    P = type("P", (), dict(first=HF.trsv_plan(tri.LOWER), second=HFt.trsv_plan(tri.UPPER), m=None))
    H, product = handle(torch, M, fmt, a, b)
    rhs = cg.rhs(M.n)
    for x0, every in ((None, 10), (start_vector(M.n), 3)):
        want = tri.run(product, rhs, x0, (F, tri.LOWER, tri.STORED), None, (Ft, tri.UPPER, tri.STORED), 100, TOL)
        same(solve(torch, H, M.n, rhs, P, x0, 100, TOL, every), want, "ic0(lap2d(16)), %s" % fmt, rhs)
    want = tri.run(product, rhs, None, (F, tri.LOWER, tri.STORED), None, (Ft, tri.UPPER, tri.STORED), 100, TOL)
    jacobi = k14.solve(torch, H, M.n, rhs, pcg.diagonal(M), None, 100, TOL)
    print("lap2d(16), %s: IC(0) %d steps, Jacobi %d" % (fmt, want[0], jacobi[0]))
    assert want[2] == tri.CONVERGED and jacobi[2] == pcg.CONVERGED and want[0] < jacobi[0]
    H.close()
    P.first.close()
    P.second.close()
    HFt.close()
    HF.close()


# ================================================================================================================ 5. the stop rules
def test_the_stop_rules_on_the_device(torch):
    for name, M, rhs, (first, m, second), tol, expect in tri.stop_cases():
        P = Plans(first, m, second)
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = P.run(product, rhs, None, 10, tol)
            assert want[:3] == expect, "%s: the restatement gives %r" % (name, want[:3])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, P, None, 10, tol, every)             # (solve checks the sentinels beyond the filled elements)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every))
                if expect[1] == 0:
                    assert_bits(got[6], np.zeros(M.n), name + ": d_x holds x_0 = zeros")
            H.close()
        P.close()
    M, x0 = k14.matrix("minus_identity", 2), np.array([0.25, -3.0])                  # rule A leaves the caller's start vector in d_x
    P = Plans(*tri.diagonal_only(np.ones(2)))
    H, product = handle(torch, M, "csr", *AUTO)
    got = solve(torch, H, 2, np.array([1.0, 0.0]) + M.spmv(x0), P, x0, 10, 1e-10, 5)
    assert got[:3] == (1, 0, tri.BREAKDOWN)
    assert_bits(got[6], x0, "x_0 after a breakdown at step 1")
    H.close()
    P.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    L, U = A.trsv_plan(tri.LOWER), A.trsv_plan(tri.UPPER)
    for H in (A, T):
        o, r = sm.cg_opts(5), sm.PcgResult()
        C.memset(C.byref(r), 0x5a, C.sizeof(r))
        b = torch.zeros(1, dtype=torch.float64, device="cuda")
        assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, L._t, None, U._t, C.byref(r), None, None, None,
                                           None) == sm.OK
        assert (r.steps, r.updates, r.reason, r.pad) == (0, 0, tri.CONVERGED, 0)
        assert_bits([r.rr, r.rz, r.bb], [0.0, 0.0, 0.0], "n = 0")
    L.close()
    U.close()
    T.close()
    A.close()


# ====================================================================================================================== 6. refusals
def refused(torch, fn, h, n, o, first, second, result=True, b="own", x0=None, x="own", m=None):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    r = sm.PcgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, rz, sigma = np.full(8, SENTINEL), np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), first._t if first is not None else None, sm._dev_ptr(m),
                               second._t if second is not None else None, C.byref(r) if result else None, sm._p(rr), sm._p(rz),
                               sm._p(sigma), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all(), \
        "%s wrote its outputs although it refused" % fn
    return rc


def test_invalid_arguments_plans_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = k14.matrix("spd", 63, 20280 + 63)
    P = Plans(*tri.sgs(trsv.of_matrix("spd(63)", M)))
    other = Plans(*tri.sgs(trsv.of_matrix("spd(64)", k14.matrix("spd", 64, 20280 + 64))))     # plans of another n
    L, U = P.first, P.second
    rhs = cg.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.cg_opts(5)
    n = M.n
    for fn, H, product, Wide in (("smvp_csr_pcg_tri", A, pa, W), ("smvp_tjds_pcg_tri", T, pt, WT)):
        assert refused(torch, fn, None, n, ok, L, U) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, H._h, n, o, L, U) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, n, ok, L, U, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, b=None) == sm.ERR_INVALID       # no d_b
        assert refused(torch, fn, H._h, n, ok, None, U) == sm.ERR_INVALID            # no first
        assert b"null first plan" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, L, None) == sm.ERR_INVALID            # no second
        assert b"null second plan" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, other.first, U) == sm.ERR_INVALID     # a plan of 64 rows
        assert b"first plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, L, other.second) == sm.ERR_INVALID
        assert b"second plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, Wide._h, 4, ok, L, U) == sm.ERR_INVALID            # rows != cols
        assert refused(torch, fn, H._h, n, ok, L, U, x=None) == sm.ERR_INVALID       # no d_x
        both = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")    # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, L, U, x0=both[:n], x=both[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, x0=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_b is d_x
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_b and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, m=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_m is d_x
        assert refused(torch, fn, H._h, n, ok, L, U, m=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_m and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, L, U, m=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert (both.cpu().numpy() == SENTINEL).all()
        same(solve(torch, H, n, rhs, P, None, 5, 1e-10), P.run(product, rhs, None, 5, 1e-10), fn + ": the handle after the refusals", rhs)
        once = type("P", (), dict(first=L, second=L, m=P.m))                         # first == second is allowed
        want = tri.run(product, rhs, None, P.triples[0], P.m, P.triples[0], 5, 1e-10)
        same(solve(torch, H, n, rhs, once, None, 5, 1e-10), want, fn + ": one plan twice")
    for H in (A, T, W, WT):
        H.close()
    P.close()
    other.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = k14.matrix("spd", 1003)
    P = Plans(*tri.sgs(trsv.of_matrix("spd(1003)", M)))
    t = sm.tjds_from_coo(M.coo, M.n, M.n)
    T = sm.TjdsMatrix(t)
    ok = sm.cg_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_pcg_tri", inner, M.n, ok, P.first, P.second) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_pcg_tri", T._h, M.n, ok, P.first, P.second) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_pcg_tri", T._h, M.n, ok, P.first, P.second) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, cg.rhs(M.n), P, None, 2, 1e-10)[:3] == (2, 2, tri.MAX_STEPS)
    T.close()
    P.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = k14.matrix("spd", 63, 20280 + 63)
    P = Plans(*tri.sgs(trsv.of_matrix("spd(63)", M)))
    rhs = cg.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db, dm = dev(torch, rhs), dev(torch, P.m)
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
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), P.first._t, sm._dev_ptr(dm),
                                                   P.second._t, C.byref(r), sm._p(rr), sm._p(rz), sm._p(sigma), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (rz == SENTINEL).all() and (sigma == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, P, None, 5, 1e-10, stream=s), P.run(product, rhs, None, 5, 1e-10),
         "outside a capture the same stream is fine")
    H.close()
    P.close()


def test_the_python_layer_refuses_what_is_no_open_plan(torch):
    M = k14.matrix("spd", 63, 20280 + 63)
    A = sm.CsrMatrix(M.n, M.n, *M.csr)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    L, U, closed = A.trsv_plan(tri.LOWER), A.trsv_plan(tri.UPPER), A.trsv_plan(tri.UPPER)
    closed.close()
    db = dev(torch, cg.rhs(M.n))
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    dm = A.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda"))
    for H in (A, T):
        for first, second in ((closed, U), (L, closed), (None, U), (L, A), (L._t, U._t)):
            with pytest.raises(ValueError):
                H.pcg_tri(db, dx, first, second, dm)
        with pytest.raises(ValueError):
            H.pcg_tri(db.cpu(), dx, L, U, dm)
        with pytest.raises(ValueError):
            H.pcg_tri(db, dx, L, U, dm.cpu())
        torch.cuda.synchronize()
        assert (dx.cpu().numpy() == SENTINEL).all()
        assert H.pcg_tri(db, torch.empty_like(dx), L, U, dm, max_steps=3, tol=0.0)[0].steps == 3
    for X in (L, U, T, A):
        X.close()


# ========================================================================================================================= 7. state
def test_the_state_of_the_handle_and_of_the_plans_afterwards(torch):
    M, Cs = system("spd_long")
    rhs = cg.rhs(M.n)
    x = start_vector(M.n, 4)
    for fmt, a, b in PATHS:
        P = Plans(*tri.sgs(Cs))
        H, product = handle(torch, M, fmt, a, b)
        name = H.describe()
        dx = dev(torch, x)

        def look():
            out = []
            for _ in range(2):                               # (the tile kernel's sweep direction may alternate: two products)
                buf, dy = guarded_y(torch, M.n)
                if fmt == "tjds":
                    H.set_x(dx)                              # the permuted operand is the last direction's: a fresh set_x, as the header says
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
        first = solve(torch, H, M.n, rhs, P, None, 7, 1e-10, 2)
        assert H.describe() == name
        for got, want in zip(look(), before):
            assert_bits(got, want, "%s %d %d: a product or a solve after the call" % (fmt, a, b))
        for i, j in zip((P.first.info(), P.second.info()), infos):
            assert {k: v for k, v in i.items() if k != "build_ms"} == {k: v for k, v in j.items() if k != "build_ms"}
        same(solve(torch, H, M.n, rhs, P, None, 7, 1e-10, 2), first[:7], "%s %d %d: the same call again" % (fmt, a, b))
        H.close()
        P.close()


def adopted(torch, Cs):
    """(handle, the device tensor of its values): a CsrMatrix over device arrays it adopts in place, on the VECTOR kernel, which
    keeps no second copy of anything."""
    rp, ci, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in Cs.csr)
    H = sm.CsrMatrix(Cs.n, Cs.n, rp, ci, v)
    H.set_kernel(sm.CSR_KERNEL_VECTOR, 0)
    return H, v


def product_of(torch, H, n):
    def product(x):
        buf, dy = guarded_y(torch, n)
        H.spmv(dev(torch, x), dy)
        torch.cuda.synchronize()
        check_guards(buf, n)
        return dy.cpu().numpy()
    return product


def scaled_case(Cs, s):
    r, c, v = Cs.entries()
    return trsv.Case("%s * %g" % (Cs.name, s), Cs.n, r, c, v * s)


def test_adopted_values_of_the_matrix_changed_in_place_are_seen(torch):
    """Symmetric Gauss-Seidel on A itself over adopted arrays: A doubled in place doubles M with it (the diagonal is taken anew,
    as a caller would), so every step's alpha halves and x with it; the plans are the old ones."""
    M = k14.matrix("spd", 1003)
    Cs = trsv.of_matrix("spd(1003)", M)
    H, v = adopted(torch, Cs)
    P = type("P", (), dict(first=H.trsv_plan(tri.LOWER), second=H.trsv_plan(tri.UPPER), m=None))
    rhs = cg.rhs(M.n)
    first, m, second = tri.sgs(Cs)
    P.m = H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert_bits(P.m, m, "the diagonal")
    one = solve(torch, H, M.n, rhs, P, None, 30, TOL)
    same(one, tri.run(product_of(torch, H, M.n), rhs, None, first, m, second, 30, TOL), "adopted arrays", rhs)
    v.mul_(2.0)
    torch.cuda.synchronize()
    first, m, second = tri.sgs(scaled_case(Cs, 2.0))
    P.m = H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda")).cpu().numpy()
    assert_bits(P.m, m, "the diagonal of the doubled matrix")
    two = solve(torch, H, M.n, rhs, P, None, 30, TOL)
    same(two, tri.run(product_of(torch, H, M.n), rhs, None, first, m, second, 30, TOL), "the values doubled in place", rhs)
    assert two[:3] == one[:3] and not np.array_equal(two[6], one[6])
    P.first.close()
    P.second.close()
    H.close()


def test_adopted_values_of_the_factor_changed_in_place_are_seen(torch):
    M = tri.lap2d(16)
    F, Ft = tri.ic0(M)
    HF, vF = adopted(torch, F)
    HFt, vFt = adopted(torch, Ft)
    P = type("P", (), dict(first=HF.trsv_plan(tri.LOWER), second=HFt.trsv_plan(tri.UPPER), m=None))
    H, product = handle(torch, M, "csr", *AUTO)
    rhs = cg.rhs(M.n)
    one = solve(torch, H, M.n, rhs, P, None, 100, TOL)
    same(one, tri.run(product, rhs, None, (F, tri.LOWER, tri.STORED), None, (Ft, tri.UPPER, tri.STORED), 100, TOL), "adopted factors", rhs)
    rng = np.random.default_rng(16)
    s = rng.uniform(0.5, 2.0, F.n)                                                   # F <- S F: M = S F F^T S is still symmetric positive definite
    rF, cF, valF = F.entries()
    rT, cT, valT = Ft.entries()
    F2 = trsv.Case("S F", F.n, rF, cF, valF * s[rF])
    Ft2 = trsv.Case("F^T S", F.n, rT, cT, valT * s[cT])
    vF.copy_(dev(torch, F2.csr[2]))
    vFt.copy_(dev(torch, Ft2.csr[2]))
    torch.cuda.synchronize()
    two = solve(torch, H, M.n, rhs, P, None, 100, TOL)
    want = tri.run(product, rhs, None, (F2, tri.LOWER, tri.STORED), None, (Ft2, tri.UPPER, tri.STORED), 100, TOL)
    same(two, want, "the factors' values changed in place", rhs)
    assert want[2] == tri.CONVERGED and not np.array_equal(two[4], one[4])
    P.first.close()
    P.second.close()
    for X in (H, HFt, HF):
        X.close()


# ======================================================================================================= 8. through the Python methods
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_whole_use_through_the_python_methods(torch, fmt, a, b):
    """diagonal() into a device vector, two trsv_plan()s, pcg_tri() on them: symmetric Gauss-Seidel on lap2d(32), where the
    diagonal is constant and Jacobi is plain CG."""
    M = tri.lap2d(32)
    H, product = handle(torch, M, fmt, a, b)
    A = H if fmt == "csr" else sm.CsrMatrix(M.n, M.n, *M.csr)                         # the plans stand on a CSR handle
    rhs = cg.rhs(M.n)
    dm = H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda"))
    L, U = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    r, rr, rz, sigma = H.pcg_tri(dev(torch, rhs), dx, L, U, m=dm, max_steps=200, tol=TOL)
    first, m, second = tri.sgs(trsv.of_matrix("lap2d(32)", M))
    want = tri.run(product, rhs, None, first, m, second, 200, TOL)
    assert (r.steps, r.updates, r.reason) == want[:3] and r.reason == sm.CG_CONVERGED
    assert len(rr) == len(rz) == r.updates + 1 and len(sigma) == r.steps
    assert_bits(rr, want[3], "rr_each")
    assert_bits(rz, want[4], "rz_each")
    assert_bits(sigma, want[5], "sigma_each")
    assert_bits([r.rr, r.rz, r.bb], [want[3][-1], want[4][-1], cg.dot(rhs, rhs)], "the result block")
    assert_bits(dx.cpu().numpy(), want[6], "d_x")
    jacobi = H.pcg(dev(torch, rhs), torch.empty_like(dx), dm, max_steps=200, tol=TOL)[0]
    print("lap2d(32), %s: SGS %d steps, Jacobi %d" % (fmt, r.steps, jacobi.steps))
    assert jacobi.reason == sm.CG_CONVERGED and 2 * r.steps <= jacobi.steps          # what the triangles are for
    x0 = dev(torch, start_vector(M.n))
    again = H.pcg_tri(dev(torch, rhs), x0, L, U, m=dm, x0=x0, max_steps=200, tol=TOL, check_every=1000, stream=torch.cuda.Stream())
    assert again[0].reason == sm.CG_CONVERGED
    assert_bits(x0.cpu().numpy(), tri.run(product, rhs, start_vector(M.n), first, m, second, 200, TOL)[6], "x0 given and aliased")
    L.close()
    U.close()
    if A is not H:
        A.close()
    H.close()
