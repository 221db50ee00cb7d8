"""GPU: right-preconditioned BiCGSTAB on a handle (smvp_csr_pbicgstab / smvp_tjds_pbicgstab, kernel K18) against its numpy
restatement tests/pbicgstab_method.py (test_pbicgstab_host.py pins that to bicgstab_method.run, to exact cases and to the true
residual), and against the library's own smvp_csr_bicgstab where the definition makes the two the same run.

No tolerance anywhere.  yhat = M^-1 y is up to two of K15's solves, each element the serial substitution loop's, and at most one
rounded multiplication; the header fixes the order of every addition of the dot; everything else is one rounded IEEE operation per
element, and the restatement's product argument is the SAME handle's single product (test_gpu_bicgstab.handle): on every path whose
product is the same from run to run, steps, full, half, reason, rr, bb, both histories and every bit of d_x have one right answer.
Comparisons are transposed.assert_bits on the uint64 views.  Every solver call goes through solve() below, which gives d_x a guarded
buffer, checks the guards, checks that d_b and d_m come back unchanged and that the histories keep a sentinel beyond the filled
elements.  The serial substitution in Python is the reference, so n stays at about 3000 at the most wherever a plan is used."""
import ctypes as C
import functools

import numpy as np
import pytest

import bicgstab_method as bi
import ilu0_method as ilu
import pbicgstab_method as pb
import power_iteration as pi
import smvp_toolkit_amd as sm
import test_gpu_bicgstab as k13
import trsv_method as trsv
from parity import check_guards, guarded_y
from test_gpu_bicgstab import AUTO, BOTH, PATHS, SENTINEL, bad_opts, dev, handle, same, start_vector
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits

pytestmark = pytest.mark.gpu

MAX_STEPS = 80
TOL = 1e-8
banded = functools.lru_cache(maxsize=None)(bi.banded)    # built once and left unchanged
ILU0_STEPS_ON_CONVDIFF = 11                                  # test_pbicgstab_host.py: the restatement's count with the host product


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def fn_of(H):
    return "smvp_%s_pbicgstab" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds")


def handle_of(Cs):
    return sm.CsrMatrix(Cs.n, Cs.n, *Cs.csr)


class Plans:
    """The restatement's (first, m, second), any of them None, on the device: a CsrMatrix per Case, a TrsvPlan per triple."""

    def __init__(self, first, m, second):
        self.triples, self.m = (first, m, second), m
        self.handles, self.keep = {}, []
        for t in (first, second):
            if t is not None and id(t[0]) not in self.handles:
                self.handles[id(t[0])] = handle_of(t[0])
        self.first = self.handles[id(first[0])].trsv_plan(first[1], first[2]) if first is not None else None
        self.second = self.handles[id(second[0])].trsv_plan(second[1], second[2]) if second is not None else None

    def run(self, product, b, x0, max_steps, tol):
        return pb.run(product, b, x0, *self.triples, max_steps, tol)

    def close(self):
        for T in (self.first, self.second):
            if T is not None:
                T.close()
        for X in self.keep + list(self.handles.values()):
            X.close()


def ilu0_plans(Cs):
    """A Plans whose two TrsvPlans are CsrMatrix.ilu0().plans() -- the library's own factor -- and whose restatement is
    ilu0_method's factor of the same Case."""
    P = Plans(None, None, None)
    A = handle_of(Cs)
    f = A.ilu0()
    P.first, P.second = f.plans()
    P.keep = [f, A]
    P.triples = pb.ilu0(Cs)
    return P


def sgs_plans(torch, Cs):
    """Symmetric Gauss-Seidel on the Case's own handle with m = diagonal() (held to the restatement's diagonal here)."""
    first, m, second = pb.sgs(Cs)
    P = Plans((Cs, first[1], first[2]), m, (Cs, second[1], second[2]))
    H = P.handles[id(Cs)]
    assert_bits(H.diagonal(torch.empty(Cs.n, dtype=torch.float64, device="cuda")).cpu().numpy(), m, "diagonal()")
    return P


def plans_of(torch, kind, Cs):
    if kind == "ilu0":
        return ilu0_plans(Cs)
    if kind == "sgs":
        return sgs_plans(torch, Cs)
    if kind == "lower":
        return Plans((Cs, pb.LOWER, pb.STORED), None, None)
    assert kind == "jacobi"
    return Plans(*pb.jacobi(Cs))


def solve(torch, H, n, b, P, x0, max_steps, tol, every=10, stream=None, alias=False, before=None):
    """One call through the C ABI -> (steps, full, half, reason, rr_each, ss_each, x, rr, bb): pbicgstab_method.run's tuple, then the
    result block's two doubles.  P: a Plans, or anything with first, second (TrsvPlans or None) and m (numpy or None).  alias: d_x is
    d_x0.  Nothing is synchronised after the call: it returns when the work is done.  ss_each's count is read off the sentinel as in
    test_gpu_bicgstab.solve, and same() holds it to the restatement's.
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
    o, r = sm.bicgstab_opts(max_steps, tol, every), sm.BicgstabResult()
    rr, ss = np.full(max_steps + 1, SENTINEL), np.full(max_steps, SENTINEL)
    if before is None:
        torch.cuda.synchronize()
    else:
        before(x=dx, b=db, x0=d0, m=dm)
    rc = getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), sm._dev_ptr(d0), sm._dev_ptr(dx),
                                     P.first._t if P.first is not None else None, sm._dev_ptr(dm),
                                     P.second._t if P.second is not None else None, C.byref(r), sm._p(rr), sm._p(ss),
                                     sm._stream_ptr(stream))
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    x = dx.cpu().numpy()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the call")
    if dm is not None:
        assert_bits(dm.cpu().numpy(), P.m, "d_m after the call")
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


# ================================================================================================= 1. bits against run(), every path
SYSTEMS = (("convdiff(32, 0.5)", "ilu0"), ("convdiff(32, 0.5)", "sgs"), ("nonsym(1003), coalesced", "ilu0"),
           ("nonsym(3001), coalesced", "sgs"), ("nonsym_shuffled", "lower"), ("nonsym_long", "jacobi"))


def test_the_systems_schedules_are_what_their_choice_rests_on(torch):
    """convdiff(32, 0.5): 63 levels of at most 32 rows -- thin levels only, each solve one chain; nonsym(1003), coalesced, with
    ILU(0): one wide level (278 and 331 rows: more than the chain width of 256) hands over to one chain; nonsym(3001), coalesced,
    with SGS: several wide launches before the chain inside a step; nonsym_shuffled: rows whose columns are not ascending, one plan
    only; nonsym_long: rows of 700 entries, a diagonal that is not constant, no plan at all."""
    info = {}
    for name, kind in SYSTEMS:
        M, Cs = pb.case_of(name)
        P = plans_of(torch, kind, Cs)
        info[name, kind] = [T.info() for T in (P.first, P.second) if T is not None]
        print(name, kind, info[name, kind][:1])
        P.close()
    for kind in ("ilu0", "sgs"):
        assert [i["levels"] for i in info["convdiff(32, 0.5)", kind]] == [63, 63]
        for i in info["convdiff(32, 0.5)", kind]:
            assert i["max_level_width"] == 32 <= i["chain_width"] and i["launches"] == i["chains"] == 1
    for i in info["nonsym(1003), coalesced", "ilu0"]:
        assert i["max_level_width"] > i["chain_width"] and (i["launches"], i["chains"]) == (2, 1)
    for i in info["nonsym(3001), coalesced", "sgs"]:
        assert i["max_level_width"] > i["chain_width"] and i["launches"] >= 5 and i["chains"] == 1
    assert len(info["nonsym_shuffled", "lower"]) == 1 and info["nonsym_long", "jacobi"] == []
    row_ptr, col_ind, val = pb.case_of("nonsym_shuffled")[1].csr
    assert any((np.diff(col_ind[a:z]) <= 0).any() for a, z in zip(row_ptr[:-1], row_ptr[1:]))
    Cs = pb.case_of("nonsym_long")[1]
    assert np.diff(Cs.csr[0]).max() >= 700 and len(np.unique(pb.jacobi(Cs)[1])) > 600


@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_every_number_is_the_restatements_on_every_reproducible_path(torch, fmt, a, b):
    for name, kind in SYSTEMS:
        M, Cs = pb.case_of(name)
        P = plans_of(torch, kind, Cs)
        H, product = handle(torch, M, fmt, a, b)
        rhs, x0 = bi.rhs(M.n), start_vector(M.n)
        want = {None: P.run(product, rhs, None, MAX_STEPS, TOL), "x0": P.run(product, rhs, x0, MAX_STEPS, TOL)}
        for key, every, alias in ((None, 1, False), (None, 7, False), ("x0", 7, False), ("x0", 1000, True)):
            what = "%s with %s, %s %d %d, x0 %s%s, check_every %d" % (name, kind, fmt, a, b, key, ", d_x is d_x0" if alias else "", every)
            got = solve(torch, H, M.n, rhs, P, x0 if key else None, MAX_STEPS, TOL, every, alias=alias)
            same(got, want[key], what, rhs)
        w = want[None]
        print("%s with %s, %s %d %d: steps %d, full %d, half %d, reason %d" % (name, kind, fmt, a, b, w[0], w[1], w[2], w[3]))
        assert w[3] == pb.CONVERGED and w[0] < MAX_STEPS, "%s with %s: the restatement did not converge" % (name, kind)
        same(solve(torch, H, M.n, rhs, P, None, 4, 0.0, 3), P.run(product, rhs, None, 4, 0.0), "%s with %s, tol 0" % (name, kind), rhs)
        H.close()
        P.close()


# ============================================================================= 2. two library calls against each other on the device
def identity_handle(n):
    return sm.CsrMatrix(n, n, np.arange(n + 1, dtype=np.int32), np.arange(n, dtype=np.int32), np.ones(n))


def bits_of_two_runs(got, want, what):
    assert got[:4] == want[:4], what
    for i, field in ((4, "rr_each"), (5, "ss_each"), (6, "d_x")):
        assert_bits(got[i], want[i], "%s: %s" % (what, field))
    assert_bits(list(got[7:]), list(want[7:]), what + ": rr, bb")


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_identity_plans_and_an_m_of_ones_are_the_librarys_bicgstab(torch, fmt, a, b):
    for name, args, steps, tol in (("nonsym", (1003,), 40, 1e-10), ("nonsym_long", (), 40, 1e-10), ("nonsym_shuffled", (), 6, 0.0),
                                   ("nonsym", (bi.TRIP + 1,), 3, 0.0)):
        M = k13.matrix(name, *args)
        E = identity_handle(M.n)
        ident = type("P", (), dict(first=E.trsv_plan(sm.TRSV_LOWER, sm.TRSV_DIAG_STORED), second=E.trsv_plan(sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT),
                                   m=None))
        ones = type("P", (), dict(first=None, second=None, m=np.ones(M.n)))
        H, product = handle(torch, M, fmt, a, b)
        rhs = bi.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            plain = k13.solve(torch, H, M.n, rhs, x0, steps, tol, 3)
            what = "%s%r, %s, x0 %s" % (name, args, fmt, "NULL" if x0 is None else "random")
            bits_of_two_runs(solve(torch, H, M.n, rhs, ident, x0, steps, tol, 3), plain, what + ", identity plans")
            bits_of_two_runs(solve(torch, H, M.n, rhs, ones, x0, steps, tol, 3), plain, what + ", m of ones")
        assert plain[0] > 2
        H.close()
        ident.first.close()
        ident.second.close()
        E.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_fused_scaling_gives_the_bits_of_the_kernel_of_its_own(torch, fmt, a, b):
    """first = NULL: the kernels that write p and s write m .* p and m .* s beside them.  first = LOWER / DIAG_UNIT on the identity
    handle: w = y - (+0.0), then the scale kernel between the solves.  The same run; on nonsym_long with an UPPER plan behind both,
    too, which then solves in place on the fused result.  banded(4 * TRIP + 1) runs the unrolled bodies of every pass."""
    for name, M, with_upper, steps, tol in (("nonsym_long", k13.matrix("nonsym_long"), True, 6, 0.0),
                                            ("banded", banded(4 * bi.TRIP + 1), False, 3, 0.0)):
        m = 1.0 / pb.pcg.diagonal_csr(M.n, M.n, *M.csr)
        E = identity_handle(M.n)
        A = sm.CsrMatrix(M.n, M.n, *M.csr) if with_upper else None
        copy = E.trsv_plan(sm.TRSV_LOWER, sm.TRSV_DIAG_UNIT)
        U = A.trsv_plan(sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT) if with_upper else None
        H, product = handle(torch, M, fmt, a, b)
        rhs = bi.rhs(M.n)
        for second in (None, U) if with_upper else (None,):
            fused = type("P", (), dict(first=None, second=second, m=m))
            unfused = type("P", (), dict(first=copy, second=second, m=m))
            for x0 in (None, start_vector(M.n)):
                got = solve(torch, H, M.n, rhs, fused, x0, steps, tol, 3)
                bits_of_two_runs(got, solve(torch, H, M.n, rhs, unfused, x0, steps, tol, 3),
                                 "%s, %s, second %s" % (name, fmt, "NULL" if second is None else "UPPER / UNIT"))
                assert got[0] >= 3 and np.isfinite(got[6]).all()
        for X in (copy, U, H, A, E):
            if X is not None:
                X.close()


# ===================================================================================================== 3. check_every changes nothing
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_nothing_depends_on_check_every(torch, fmt, a, b):
    for name, kind in (("convdiff(32, 0.5)", "ilu0"), ("nonsym_long", "jacobi")):
        M, Cs = pb.case_of(name)
        P = plans_of(torch, kind, Cs)
        H, product = handle(torch, M, fmt, a, b)
        rhs = bi.rhs(M.n)
        for x0 in (None, start_vector(M.n)):
            want = P.run(product, rhs, x0, MAX_STEPS, TOL)
            assert want[3] == pb.CONVERGED and 3 < want[0] < MAX_STEPS
            for every in (1, 7, MAX_STEPS):
                same(solve(torch, H, M.n, rhs, P, x0, MAX_STEPS, TOL, every), want,
                     "%s with %s, %s, x0 %s, check_every %d" % (name, kind, fmt, "NULL" if x0 is None else "random", every), rhs)
        H.close()
        P.close()


# ==================================================================================================================== 4. sizes
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1003])
def test_sizes_around_a_wavefront_and_a_workgroup(torch, n):
    M = k13.matrix("nonsym", n, 20300 + n)
    P = Plans(*pb.jacobi(trsv.of_matrix("nonsym(%d)" % n, M)))
    rhs = bi.rhs(n)
    for fmt, a, b in BOTH:
        H, product = handle(torch, M, fmt, a, b)
        for x0 in (None, start_vector(n)):
            same(solve(torch, H, n, rhs, P, x0, 20, 1e-10, 5), P.run(product, rhs, x0, 20, 1e-10), "nonsym(%d), %s" % (n, fmt), rhs)
        H.close()


@pytest.mark.parametrize("n", [bi.TRIP + 1, 4 * bi.TRIP + 1])
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_one_element_past_the_first_grid_trip_and_past_the_unrolled_bodies(torch, n, fmt, a, b):
    """n = 2048 * 256 + 1: the last element is the second trip of lane 0 of workgroup 0 alone.  n = 4 * 2048 * 256 + 1: the smallest
    size at which the four-deep bodies of the passes that write run at all, and one element over.  Jacobi only: the restatement is
    pure numpy."""
    M = banded(n)
    m = 1.0 / (2.0 + (np.arange(n) % 7) / 8.0)
    P = type("P", (), dict(first=None, second=None, m=m))
    rhs = bi.rhs(n)
    H, product = handle(torch, M, fmt, a, b)
    want = pb.run(product, rhs, None, None, m, None, 3, 0.0)
    assert want[:4] == (3, 3, 0, pb.MAX_STEPS)
    same(solve(torch, H, n, rhs, P, None, 3, 0.0, 2), want, "banded(%d), %s" % (n, fmt), rhs)
    H.close()


# ================================================================================================================ 5. the stop rules
def test_the_stop_rules_on_the_device(torch):
    for name, M, rhs, (first, m, second), tol, expect, x in pb.stop_cases():
        P = Plans(first, m, second)
        for fmt, a, b in BOTH:
            H, product = handle(torch, M, fmt, a, b)
            want = P.run(product, rhs, None, 10, tol)
            assert want[:4] == expect, "%s: the restatement gives %r" % (name, want[:4])
            for every in (1, 5):
                got = solve(torch, H, M.n, rhs, P, None, 10, tol, every)             # (solve checks the sentinels beyond the filled elements)
                same(got, want, "%s, %s, check_every %d" % (name, fmt, every))
                if x is not None:
                    assert_bits(got[6], x, name + ": d_x")
            H.close()
        P.close()
    A = k13.matrix("nonsym", 300)                                                     # rule A leaves the caller's start vector in d_x
    Cs = trsv.of_matrix("nonsym(300)", A)
    x0 = start_vector(300)
    for triple in ((None, pb.nan_m(300), None), ((pb.tri.zero_diagonal(A, 17), pb.LOWER, pb.STORED), None, pb.sgs(Cs)[2])):
        P = Plans(*triple)
        for fmt, a, b in BOTH:
            H, product = handle(torch, A, fmt, a, b)
            got = solve(torch, H, 300, bi.rhs(300), P, x0, 10, 1e-10, 5)
            assert got[:4] == (1, 0, 0, pb.NONFINITE) and len(got[5]) == 0
            assert_bits(got[6], x0, "x_0 after NONFINITE by rule A at step 1")
            H.close()
        P.close()


def test_a_matrix_without_rows(torch):
    A = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    T = sm.TjdsMatrix(sm.tjds_from_coo(sm.make_coo([], [], []), 0, 0))
    L, U = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
    b = torch.zeros(1, dtype=torch.float64, device="cuda")
    for H in (A, T):
        for first, m, second in ((L, None, U), (None, b, None), (L, b, None)):
            o, r = sm.bicgstab_opts(5), sm.BicgstabResult()
            C.memset(C.byref(r), 0x5a, C.sizeof(r))
            assert getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(b), None, None, first._t if first else None, sm._dev_ptr(m),
                                               second._t if second else None, C.byref(r), None, None, None) == sm.OK
            assert (r.steps, r.full, r.half, r.reason) == (0, 0, 0, pb.CONVERGED)
            assert_bits([r.rr, r.bb], [0.0, 0.0], "n = 0")
    L.close()
    U.close()
    T.close()
    A.close()


# ==================================================================================================================== 6. operands
def test_operands(torch):
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    rhs, x0 = bi.rhs(M.n), start_vector(M.n)
    side = torch.cuda.Stream()
    for fmt, a, b in BOTH:
        P = sgs_plans(torch, Cs)
        H, product = handle(torch, M, fmt, a, b)
        want = P.run(product, rhs, x0, MAX_STEPS, TOL)
        assert want[3] == pb.CONVERGED
        same(solve(torch, H, M.n, rhs, P, x0, MAX_STEPS, TOL), want, fmt + ", separate vectors", rhs)
        same(solve(torch, H, M.n, rhs, P, x0, MAX_STEPS, TOL, alias=True), want, fmt + ", d_x is d_x0", rhs)
        same(solve(torch, H, M.n, rhs, P, x0, MAX_STEPS, TOL, stream=side), want, fmt + ", a stream of the caller's", rhs)
        once = type("P", (), dict(first=P.first, second=P.first, m=P.m))               # first == second is allowed
        want = pb.run(product, rhs, None, P.triples[0], P.m, P.triples[0], 5, 0.0)
        same(solve(torch, H, M.n, rhs, once, None, 5, 0.0), want, fmt + ": one plan twice")
        H.close()
        P.close()


def test_the_state_of_the_handle_and_of_the_plans_afterwards(torch):
    M, Cs = pb.case_of("nonsym(1003), coalesced")
    rhs = bi.rhs(M.n)
    x = start_vector(M.n, 4)
    for fmt, a, b in PATHS:
        P = sgs_plans(torch, Cs)
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
        first = solve(torch, H, M.n, rhs, P, None, 7, 0.0, 2)
        assert H.describe() == name
        for got, want in zip(look(), before):
            assert_bits(got, want, "%s %d %d: a product or a solve after the call" % (fmt, a, b))
        for i, j in zip((P.first.info(), P.second.info()), infos):
            assert {k: v for k, v in i.items() if k != "build_ms"} == {k: v for k, v in j.items() if k != "build_ms"}
        same(solve(torch, H, M.n, rhs, P, None, 7, 0.0, 2), first[:7], "%s %d %d: the same call again" % (fmt, a, b))
        H.close()
        P.close()


def test_a_factor_computed_anew_in_place_is_seen_by_the_next_call(torch):
    """A's values live in a tensor the handle adopts; Ilu0.factor() after they changed rewrites F's values in place, and the plans
    made before -- which borrow them -- precondition the next call with the new factor."""
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    r, c, v = Cs.entries()
    s = np.random.default_rng(18).uniform(0.5, 2.0, Cs.n)
    Cs2 = trsv.Case("S * convdiff(32, 0.5)", Cs.n, r, c, v * s[r])                    # ILU(0) of S A: M^-1 is about A^-1 S^-1
    assert (Cs2.csr[1] == Cs.csr[1]).all()
    rp, ci, dv = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in Cs.csr)
    A = sm.CsrMatrix(Cs.n, Cs.n, rp, ci, dv)
    f = A.ilu0()
    P = type("P", (), dict(m=None))
    P.first, P.second = f.plans()
    H, product = handle(torch, M, "csr", *AUTO)
    rhs = bi.rhs(M.n)
    one = solve(torch, H, M.n, rhs, P, None, MAX_STEPS, TOL, 1)
    same(one, pb.run(product, rhs, None, *pb.ilu0(Cs), MAX_STEPS, TOL), "the first factor", rhs)
    dv.copy_(dev(torch, Cs2.csr[2]))
    f.factor()
    torch.cuda.synchronize()
    two = solve(torch, H, M.n, rhs, P, None, MAX_STEPS, TOL, 1)
    want = pb.run(product, rhs, None, *pb.ilu0(Cs2), MAX_STEPS, TOL)
    same(two, want, "the factor computed anew in place", rhs)
    assert want[3] == pb.CONVERGED and not np.array_equal(two[4], one[4])
    for X in (P.first, P.second, f, A, H):
        X.close()


# ====================================================================================================================== 7. refusals
def refused(torch, fn, h, n, o, first, second, result=True, b="own", x0=None, x="own", m=None):
    """The status of one call that must be refused: d_x, *result and the histories come back untouched."""
    dx = torch.full((max(n, 1) + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    db = dev(torch, np.ones(max(n, 1))) if isinstance(b, str) else b
    r = sm.BicgstabResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rr, ss = np.full(8, SENTINEL), np.full(8, SENTINEL)
    torch.cuda.synchronize()
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, sm._dev_ptr(db), sm._dev_ptr(x0),
                               sm._dev_ptr(dx if isinstance(x, str) else x), first._t if first is not None else None, sm._dev_ptr(m),
                               second._t if second is not None else None, C.byref(r) if result else None, sm._p(rr), sm._p(ss), None)
    torch.cuda.synchronize()
    assert (dx.cpu().numpy() == SENTINEL).all(), "%s wrote d_x although it refused" % fn
    assert bytes(r) == before and (rr == SENTINEL).all() and (ss == SENTINEL).all(), "%s wrote its outputs although it refused" % fn
    return rc


def test_invalid_arguments_plans_and_overlaps_are_refused_and_nothing_is_written(torch):
    M = k13.matrix("nonsym", 63, 20300 + 63)
    P = sgs_plans(torch, trsv.of_matrix("nonsym(63)", M))
    other = sgs_plans(torch, trsv.of_matrix("nonsym(64)", k13.matrix("nonsym", 64, 20300 + 64)))     # plans of another n
    L, U = P.first, P.second
    rhs = bi.rhs(M.n)
    A, pa = handle(torch, M, "csr", *AUTO)
    T, pt = handle(torch, M, "tjds", sm.TJDS_MODE_ROW_GATHER, 0)
    wide = sm.make_coo([0, 1, 2], [1, 3, 0], [1.5, -2.5, 3.5])                       # 3 x 4
    W = sm.CsrMatrix(3, 4, *sm.csr_from_coo(wide, 3))
    WT = sm.TjdsMatrix(sm.tjds_from_coo(wide, 3, 4))
    ok = sm.bicgstab_opts(5)
    n = M.n
    dm = dev(torch, P.m)
    for fn, H, product, Wide in (("smvp_csr_pbicgstab", A, pa, W), ("smvp_tjds_pbicgstab", T, pt, WT)):
        assert refused(torch, fn, H._h, n, ok, None, None) == sm.ERR_INVALID         # no preconditioner at all
        assert b"all NULL" in sm.lib().smvp_last_error() and b"smvp_csr_bicgstab" in sm.lib().smvp_last_error()
        assert refused(torch, fn, None, n, ok, L, U) == sm.ERR_INVALID
        for o in bad_opts():
            assert refused(torch, fn, H._h, n, o, L, U) == sm.ERR_INVALID, "opts %r" % (o and [getattr(o, f[0]) for f in o._fields_],)
        assert refused(torch, fn, H._h, n, ok, L, U, result=False) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, b=None) == sm.ERR_INVALID       # no d_b
        assert refused(torch, fn, H._h, n, ok, other.first, U) == sm.ERR_INVALID     # a plan of 64 rows
        assert b"first plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, L, other.second) == sm.ERR_INVALID
        assert b"second plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, H._h, n, ok, None, other.second, m=dm) == sm.ERR_INVALID
        assert b"second plan solves 64 rows" in sm.lib().smvp_last_error()
        assert refused(torch, fn, Wide._h, 4, ok, L, U) == sm.ERR_INVALID            # rows != cols
        assert refused(torch, fn, Wide._h, 4, ok, None, None, m=dm) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, x=None) == sm.ERR_INVALID       # no d_x
        both = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")    # d_x0 and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, L, U, x0=both[:n], x=both[1:]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, x0=both[1:], x=both[:n]) == sm.ERR_INVALID
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_b is d_x
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[:n], x=both[1:]) == sm.ERR_INVALID      # d_b and d_x one element apart
        assert refused(torch, fn, H._h, n, ok, L, U, b=both[1:], x=both[:n]) == sm.ERR_INVALID
        for first, second in ((L, U), (None, None)):
            assert refused(torch, fn, H._h, n, ok, first, second, m=both[:n], x=both[:n]) == sm.ERR_INVALID      # d_m is d_x
            assert refused(torch, fn, H._h, n, ok, first, second, m=both[:n], x=both[1:]) == sm.ERR_INVALID      # one element apart
            assert refused(torch, fn, H._h, n, ok, first, second, m=both[1:], x=both[:n]) == sm.ERR_INVALID
            assert b"d_m and d_x overlap" in sm.lib().smvp_last_error()
        assert (both.cpu().numpy() == SENTINEL).all()
        same(solve(torch, H, n, rhs, P, None, 5, 1e-10), P.run(product, rhs, None, 5, 1e-10), fn + ": the handle after the refusals", rhs)
    for H in (A, T, W, WT):
        H.close()
    P.close()
    other.close()


def test_unsupported_handles_are_refused_and_nothing_is_written(torch):
    M = k13.matrix("nonsym", 1003)
    P = Plans(*pb.jacobi(trsv.of_matrix("nonsym(1003)", M)))
    dm = dev(torch, P.m)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    ok = sm.bicgstab_opts(5)
    inner = inner_csr_handle(T, M.n, M.n, M.nnz)                                     # a CSR handle that is not plain CSR
    assert refused(torch, "smvp_csr_pbicgstab", inner, M.n, ok, None, None, m=dm) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    assert refused(torch, "smvp_tjds_pbicgstab", T._h, M.n, ok, None, None, m=dm) == sm.ERR_UNSUPPORTED
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_ref_quirks(True)
    assert refused(torch, "smvp_tjds_pbicgstab", T._h, M.n, ok, None, None, m=dm) == sm.ERR_UNSUPPORTED
    T.set_ref_quirks(False)
    assert solve(torch, T, M.n, bi.rhs(M.n), P, None, 2, 1e-10)[:4] == (2, 2, 0, pb.MAX_STEPS)
    T.close()
    P.close()


@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_a_capturing_stream_is_refused_and_the_capture_stays_valid(torch, fmt, a, b):
    M = k13.matrix("nonsym", 63, 20300 + 63)
    P = sgs_plans(torch, trsv.of_matrix("nonsym(63)", M))
    rhs = bi.rhs(M.n)
    H, product = handle(torch, M, fmt, a, b)
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((M.n,), SENTINEL, dtype=torch.float64, device="cuda")
    db, dm = dev(torch, rhs), dev(torch, P.m)
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
            got.append(getattr(sm.lib(), fn_of(H))(H._h, C.byref(o), sm._dev_ptr(db), None, sm._dev_ptr(dx), P.first._t, sm._dev_ptr(dm),
                                                   P.second._t, C.byref(r), sm._p(rr), sm._p(ss), s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg
    assert bytes(r) == before and (rr == SENTINEL).all() and (ss == SENTINEL).all()
    g.replay()                                               # the capture stayed valid, and holds nothing of the refused call
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == SENTINEL).all()
    del g
    same(solve(torch, H, M.n, rhs, P, None, 5, 1e-10, stream=s), P.run(product, rhs, None, 5, 1e-10),
         "outside a capture the same stream is fine")
    H.close()
    P.close()


# ======================================================================================================= 8. through the Python methods
@pytest.mark.parametrize("fmt,a,b", BOTH)
def test_the_whole_use_through_the_python_methods_and_plain_bicgstab_fails_where_this_converges(torch, fmt, a, b):
    """diagonal() and one torch.reciprocal for Jacobi; ilu0().plans() for ILU(0); trsv_plan()s of the matrix itself and diagonal()
    for symmetric Gauss-Seidel.  Given ILU(0)'s step count on the host plus 2, plain BiCGSTAB ends with MAX_STEPS on
    convdiff(32, 0.5) and the preconditioned run with CONVERGED."""
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    H, product = handle(torch, M, fmt, a, b)
    A = H if fmt == "csr" else handle_of(Cs)                                          # the plans stand on a CSR handle
    rhs = bi.rhs(M.n)
    db = dev(torch, rhs)
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    f = A.ilu0()
    first, second = f.plans()
    steps = ILU0_STEPS_ON_CONVDIFF + 2
    r, rr, ss = H.pbicgstab(db, dx, first, second, max_steps=steps, tol=TOL, check_every=1)
    want = pb.run(product, rhs, None, *pb.ilu0(Cs), steps, TOL)
    assert (r.steps, r.full, r.half, r.reason) == want[:4] and r.reason == sm.BICGSTAB_CONVERGED
    assert len(rr) == r.full + 1 and len(ss) == r.steps
    assert_bits(rr, want[4], "rr_each")
    assert_bits(ss, want[5], "ss_each")
    assert_bits([r.rr, r.bb], [want[5][-1] if r.half else want[4][-1], bi.dot(rhs, rhs)], "the result block")
    assert_bits(dx.cpu().numpy(), want[6], "d_x")
    plain = H.bicgstab(db, torch.empty_like(dx), max_steps=steps, tol=TOL)[0]
    print("convdiff(32, 0.5), %s: ILU(0) %d steps; plain BiCGSTAB after %d: reason %d, rr %r" % (fmt, r.steps, steps, plain.reason, plain.rr))
    assert plain.reason == sm.BICGSTAB_MAX_STEPS and plain.rr > (np.float64(TOL) * np.float64(TOL)) * r.bb

    dd = H.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda"))            # a TJDS handle has a diagonal too
    dm = torch.reciprocal(dd)
    jac = H.pbicgstab(db, torch.empty_like(dx), m=dm, max_steps=200, tol=TOL)
    want = pb.run(product, rhs, None, None, dm.cpu().numpy(), None, 200, TOL)
    assert (jac[0].steps, jac[0].reason) == (want[0], sm.BICGSTAB_CONVERGED)
    assert_bits(jac[1], want[4], "Jacobi: rr_each")
    L, U = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
    x0 = dev(torch, start_vector(M.n))
    sgs = H.pbicgstab(db, x0, L, U, m=dd, x0=x0, max_steps=200, tol=TOL, check_every=1000, stream=torch.cuda.Stream())
    want = pb.run(product, rhs, start_vector(M.n), *pb.sgs(Cs), 200, TOL)
    assert sgs[0].reason == sm.BICGSTAB_CONVERGED and 2 * sgs[0].steps <= jac[0].steps
    assert_bits(x0.cpu().numpy(), want[6], "SGS: x0 given and aliased")
    with pytest.raises(sm.SmvpError):
        H.pbicgstab(db, dx)                                                           # no preconditioner: the library's refusal
    for bad in (dict(first=A), dict(second=L._t), dict(m=dm.cpu())):
        with pytest.raises(ValueError):
            H.pbicgstab(db, dx, **bad)
    for X in (L, U, first, second, f):
        X.close()
    if A is not H:
        A.close()
    H.close()
