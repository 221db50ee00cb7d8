"""GPU: sparse triangular solves on a CSR handle (smvp_csr_trsv_create / smvp_trsv_solve, kernel K15) against their restatement
tests/trsv_method.py (test_trsv_host.py pins that to hand-computed values and to a derived bound).

No tolerance anywhere: every x_i is the serial substitution loop's.  Comparisons are transposed.assert_bits on every element of
d_x (a NaN equals a NaN whatever its sign and payload -- x86 and the GPU differ there -- while an Inf's sign is one of its bits).
Every solve goes through solve_once(), which gives d_x a guarded buffer poisoned with NaN, checks the guards and checks that d_b
comes back unchanged.  The constructed schedules are built from the chain width smvp_trsv_info reports, not from a mirror of it."""
import ctypes as C
import functools

import numpy as np
import pytest

import cg_method as cg
import pcg_method as pcg
import smvp_toolkit_amd as sm
import trsv_method as tm
from parity import U as ROUNDOFF, check_guards, guarded_y
from test_gpu_cg import AUTO, SENTINEL, dev, handle
from test_gpu_transposed import inner_csr_handle
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu

BOTH = [(u, d) for u in (LOWER, UPPER) for d in (STORED, UNIT)]
N_EXISTING = len(tm.existing_cases())
N_CONSTRUCTED = len(tm.constructed_cases(8))         # (how many there are does not depend on the width)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def chain_width():
    """The library's constant, as smvp_trsv_info reports it."""
    H = sm.CsrMatrix(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1))
    P = H.trsv_plan(LOWER)
    w = P.info()["chain_width"]
    P.close()
    H.close()
    assert w >= 64
    return w


def handle_of(M):
    return sm.CsrMatrix(M.n, M.n, *M.csr)


def solve_once(torch, P, n, b, stream=None, alias=False):
    """One solve into a guarded buffer poisoned with NaN: every element is written, nothing beside them, d_b is left as it was.
    alias: d_x is d_b."""
    db = dev(torch, b)
    buf, dx = guarded_y(torch, n)
    if alias:
        dx.copy_(db)
    torch.cuda.synchronize()
    assert P.solve(dx if alias else db, dx, stream=stream) is dx
    torch.cuda.synchronize()
    check_guards(buf, n)
    assert_bits(db.cpu().numpy(), b, "d_b after the solve")
    return dx.cpu().numpy()


def check_plan(torch, H, M, uplo, diag, calls=("again", "stream", "alias")):
    """A plan's info and schedule against the restatement's, and its solves against the restatement's bits.  Returns the info."""
    what = "%s, uplo %d, diag %d" % (M.name, uplo, diag)
    P = H.trsv_plan(uplo, diag)
    info, f = P.info(), M.facts(uplo, diag)
    for field in ("levels", "max_level_width", "missing_diagonals", "entries"):
        assert info[field] == f[field], "%s: %s is %r, the restatement's %r" % (what, field, info[field], f[field])
    assert info["launches"] == tm.launches(f["widths"], info["chain_width"]), what
    assert info["chains"] == tm.chains(f["widths"], info["chain_width"]), what
    assert info["plan_bytes"] >= 4 * (M.n + f["levels"] + 1) and info["build_ms"] >= 0.0
    level_ptr, order = P.schedule()
    assert level_ptr.tolist() == f["level_ptr"].tolist() and order.tolist() == f["order"].tolist(), what
    b, want = M.reference(uplo, diag)
    assert_bits(solve_once(torch, P, M.n, b), want, what)
    if "again" in calls:
        assert_bits(solve_once(torch, P, M.n, b), want, what + ": the same call again")
    if "stream" in calls:
        assert_bits(solve_once(torch, P, M.n, b, stream=torch.cuda.Stream()), want, what + ": on a stream of the caller's")
    if "alias" in calls:
        assert_bits(solve_once(torch, P, M.n, b, alias=True), want, what + ": d_x is d_b")
    P.close()
    return info


# ========================================================================================================= 1. bits on every case
@pytest.mark.parametrize("i", range(N_EXISTING))
def test_every_element_is_the_restatements_on_every_case(torch, i):
    M = tm.existing_cases()[i]
    H = handle_of(M)
    for uplo, diag in BOTH:
        info = check_plan(torch, H, M, uplo, diag)
        print("%s, uplo %d, diag %d: %d rows, %d entries read, %d levels (widest %d), %d launches of which %d chains, %d lanes a row"
              % (M.name, uplo, diag, M.n, info["entries"], info["levels"], info["max_level_width"], info["launches"], info["chains"],
                 info["lanes_per_row"]))
    H.close()


# ===================================================================================================== 2. constructed schedules
@pytest.mark.parametrize("i", range(N_CONSTRUCTED))
def test_constructed_schedules(torch, i):
    w = chain_width()
    M = tm.constructed_cases(w)[i]
    flipped = M.name.endswith("flipped")
    base, shaped = M.name.split("(")[0], UPPER if flipped else LOWER     # the triangle that holds the constructed schedule
    H = handle_of(M)
    for uplo, diag in BOTH:
        info = check_plan(torch, H, M, uplo, diag)
        if uplo != shaped and base != "identity":
            assert info["levels"] == 1, "the other triangle of a constructed case holds the diagonal only"
            continue
        if base == "identity":
            assert (info["levels"], info["launches"], info["chains"]) == (1, 1, 1 if M.n <= w else 0)
        elif base == "bidiagonal":
            assert (info["levels"], info["max_level_width"], info["launches"], info["chains"]) == (M.n, 1, 1, 1)
        elif base == "dense_lower":
            assert (info["levels"], info["launches"]) == (70, 1)
        elif base == "wide_thin_wide":
            assert (info["levels"], info["launches"], info["chains"]) == (9, 4, 2)
        elif base == "adjacent":
            assert (info["levels"], info["launches"], info["chains"]) == (5, 5, 3)
        elif base == "divergent":
            assert (info["levels"], info["launches"], info["chains"]) == (6, 1, 1)
        elif base == "interleaved":
            assert (info["levels"], info["launches"]) == (4, 1 if M.n <= 4 * w else 4)
        else:
            raise AssertionError(M.name)
    H.close()


def test_the_chain_width_option_changes_the_schedule_and_no_bit(torch):
    """Plan option trsv_chain_width (256 by default, 512 or 1024: a lane of a chain's workgroup takes two or four rows of a level),
    read when a plan is made: the launches follow the width the plan reports, the bits do not change."""
    w = chain_width()
    for M in (tm.existing_cases()[7], tm.wide_thin_wide(w), tm.adjacent(w)):          # pwt: levels of up to 534 rows
        H = handle_of(M)
        seen = set()
        for width in (2 * w, 4 * w):
            with sm.option("trsv_chain_width", width):
                info = check_plan(torch, H, M, LOWER, STORED, calls=("alias",))
            assert info["chain_width"] == width
            seen.add(info["launches"])
        info = check_plan(torch, H, M, LOWER, STORED, calls=())                       # outside the context: the default again
        assert info["chain_width"] == w and info["launches"] > max(seen)
        H.close()


# ============================================================================================================ 3. storage order
def test_the_additions_follow_the_stored_order(torch):
    for M in (tm.order_dependent(), tm.existing_cases()[2]):
        S = tm.sorted_copy(M)
        H, HS = handle_of(M), handle_of(S)
        for uplo, diag in ((LOWER, STORED), (LOWER, UNIT)):
            a, b = M.reference(uplo, diag)[1], S.reference(uplo, diag)[1]
            assert (a.view(np.int64) != b.view(np.int64)).any(), "%s: the order shows in the restatement" % M.name
            check_plan(torch, H, M, uplo, diag, calls=())
            check_plan(torch, HS, S, uplo, diag, calls=())
        H.close()
        HS.close()


# ================================================================================================= 4. the other triangle ignored
def test_the_other_triangle_is_skipped_and_stored_zeros_only_add_levels(torch):
    M = tm.existing_cases()[0]
    for uplo, diag in BOTH:
        want = M.reference(uplo, diag)[1]
        T, Z = tm.triangle_of(M, uplo), tm.triangle_of(M, uplo, zeros=True)
        for X in (T, Z):
            assert_bits(X.reference(uplo, diag)[1], want, "the restatement: %s" % X.name)
            H = handle_of(X)
            check_plan(torch, H, X, uplo, diag, calls=())
            H.close()
        H = handle_of(T)
        assert check_plan(torch, H, T, 1 - uplo, UNIT, calls=())["levels"] == 1
        H.close()
        H = handle_of(Z)                                                              # stored zeros are structure: levels, x = b
        assert check_plan(torch, H, Z, 1 - uplo, UNIT, calls=())["levels"] == M.facts(1 - uplo, UNIT)["levels"] > 1
        assert_bits(Z.reference(1 - uplo, UNIT)[1], Z.reference(1 - uplo, UNIT)[0], "zeros change no finite number")
        H.close()


# ============================================================================================================ 5. values in place
def test_adopted_values_changed_in_place_are_seen_without_a_new_plan(torch):
    M = tm.existing_cases()[0]
    rp, ci, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in M.csr)
    H = sm.CsrMatrix(M.n, M.n, rp, ci, v)
    plans = {k: H.trsv_plan(*k) for k in BOTH}
    for k, P in plans.items():
        assert_bits(solve_once(torch, P, M.n, M.reference(*k)[0]), M.reference(*k)[1], "adopted arrays, uplo %d, diag %d" % k)
    v.mul_(-3.0)
    torch.cuda.synchronize()
    M3 = tm.Case.of_csr("spd(1003) * -3", M.n, M.csr[0], M.csr[1], M.csr[2] * -3.0)
    for k, P in plans.items():
        b, want = M3.reference(*k)
        assert not np.array_equal(want, M.reference(*k)[1])
        assert_bits(solve_once(torch, P, M.n, b), want, "values changed in place, uplo %d, diag %d" % k)
        P.close()
    H.close()


# ================================================================================================================ 6. non-finite
def zero_diagonal():
    """spd(300)'s structure with dominant values, the diagonal of row 40 stored as 0.0 and that of row 200 as a pair that cancels."""
    S = cg.spd(300)
    r, c, v = tm.dominant("zero_diagonal", 300, S.coo["row"], S.coo["col"], 20320).entries()
    v = v.copy()
    v[(r == 40) & (c == 40)] = 0.0
    r, c, v = np.concatenate([r, [200]]), np.concatenate([c, [200]]), np.concatenate([v, -v[(r == 200) & (c == 200)]])
    return tm.Case("zero_diagonal", 300, r, c, v, finite_stored=False)


def test_zero_and_missing_diagonals_give_the_restatements_infinities_and_nans(torch):
    P8 = tm.existing_cases()[-1]
    assert P8.name == "pdp08-pg4" and P8.facts(LOWER, STORED)["missing_diagonals"] == 1
    seen = {"inf": 0, "nan": 0}
    for M in (zero_diagonal(), P8):
        H = handle_of(M)
        for uplo in (LOWER, UPPER):
            b, want = M.reference(uplo, STORED)
            assert not np.isfinite(want).all() and np.isfinite(want).any(), "%s: some of x is finite, some is not" % M.name
            P = H.trsv_plan(uplo, STORED)
            got = solve_once(torch, P, M.n, b)
            fin = np.isfinite(want)
            assert_bits(got[fin], want[fin], "%s, uplo %d: where the restatement is finite" % (M.name, uplo))
            assert (np.isinf(got) == np.isinf(want)).all() and (got[np.isinf(want)] == want[np.isinf(want)]).all(), "Inf positions and signs"
            assert (np.isnan(got) == np.isnan(want)).all(), "NaN positions"
            seen["inf"] += int(np.isinf(want).sum())
            seen["nan"] += int(np.isnan(want).sum())
            P.close()
            check_plan(torch, H, M, uplo, UNIT, calls=())                             # the unit diagonal never looks at them
        H.close()
    assert seen["inf"] and seen["nan"], seen


# =================================================================================================================== 7. capture
def test_a_solve_is_captured_as_a_plans_first_call(torch):
    w = chain_width()
    for M, uplo in ((tm.wide_thin_wide(w), LOWER), (tm.existing_cases()[5], UPPER)):  # wide launches and chains; curtis54
        H = handle_of(M)
        P = H.trsv_plan(uplo, STORED)                                                 # outside the capture: it copies back and allocates
        b, want = M.reference(uplo, STORED)
        db = dev(torch, b)
        buf, dx = guarded_y(torch, M.n)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                rc = sm.lib().smvp_trsv_solve(P._t, sm._dev_ptr(db), sm._dev_ptr(dx), s.cuda_stream)
        assert rc == sm.OK, sm.lib().smvp_last_error().decode()
        for _ in range(2):
            dx.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            check_guards(buf, M.n)
            assert_bits(dx.cpu().numpy(), want, "%s: the replayed capture" % M.name)
        assert_bits(db.cpu().numpy(), b, "d_b")
        del g
        P.close()
        H.close()


def test_symmetric_gauss_seidel_is_captured_from_two_plans_of_one_handle(torch):
    """z = U^-1 (d o (L^-1 r)): the lower and the upper plan of one handle back to back, torch.mul in between."""
    M = tm.existing_cases()[3]                                                        # tridiagonal(300): two chains of 300 levels
    d = pcg.diagonal_csr(M.n, M.n, *M.csr)
    r = tm.rhs(M.n, 16)
    t1 = tm.solve(M, LOWER, STORED, r)
    want = tm.solve(M, UPPER, STORED, t1 * d)
    H = handle_of(M)
    L, U = H.trsv_plan(LOWER), H.trsv_plan(UPPER)
    dd, dr = dev(torch, d), dev(torch, r)
    dt = torch.empty(M.n, dtype=torch.float64, device="cuda")
    buf, dz = guarded_y(torch, M.n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            L.solve(dr, dt, stream=s)
            torch.mul(dt, dd, out=dt)
            U.solve(dt, dz, stream=s)
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
    s = torch.cuda.Stream()
    out, got = C.c_void_p(), []
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)
            got.append(sm.lib().smvp_csr_trsv_create(C.byref(out), H._h, LOWER, STORED, s.cuda_stream))
            msg = sm.lib().smvp_last_error().decode()
            dZ.add_(1.0)
    assert got == [sm.ERR_INVALID] and "captur" in msg and out.value is None
    g.replay()
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16
    del g
    H.close()


# ================================================================================================================ 8. the whole use
def test_gauss_seidel_composed_from_the_public_calls(torch):
    """x += L^-1 (b - A x), twenty sweeps on spd(1003): the handle's spmv, torch.sub, the lower plan's solve, torch.add; against the
    same composition of the restatement around the SAME handle's product.  The residual's 1-norm falls with every sweep: r' = -U
    L^-1 r with U the strict upper triangle, and ||U L^-1||_1 = ||L^-T U^T||_inf < 1 for a matrix that is strictly dominant by
    columns (Gauss-Seidel's classical bound, applied to the transpose) -- spd is symmetric and strictly dominant by rows.  That is a
    property of the construction in exact arithmetic, so it is asserted on the restatement only, and for every sweep whose residual
    is more than rounding error: the computed b - fl(A x) differs from b - A x by at most (k_i + 2) u (|A| |x| + |b|)_i in row i
    (k_i entries: the product's bound and one subtraction), and a residual whose 1-norm is under the sum of that says nothing about
    the true one.  On this matrix the norm falls about twentyfold a sweep and reaches that floor (8.8e-13) at sweep 12 (measured
    on the CPU: 3.1e-12 at sweep 11, 1.9e-13 at 12, then 1.5e-14 to the end); every sweep before is held to the strict fall, and the
    run must get under the floor and stay there."""
    A = cg.spd(1003)
    M = tm.of_matrix("spd(1003)", A)
    H, product = handle(torch, A, "csr", *AUTO)
    P = H.trsv_plan(LOWER)
    b = cg.rhs(A.n)
    db, dx = dev(torch, b), torch.zeros(A.n, dtype=torch.float64, device="cuda")
    dy, dr, dz = (torch.empty(A.n, dtype=torch.float64, device="cuda") for _ in range(3))
    x, norms, floors = np.zeros(A.n), [], []
    for sweep in range(20):
        r = b - product(x)
        norms.append(np.abs(r).sum())
        floors.append(((A.terms + 2) * ROUNDOFF * (A.scale(x) + np.abs(b))).sum())
        x = x + tm.solve(M, LOWER, STORED, r)
        H.spmv(dx, dy)
        torch.sub(db, dy, out=dr)
        P.solve(dr, dz)
        dx.add_(dz)
        torch.cuda.synchronize()
        assert_bits(dr.cpu().numpy(), r, "the residual before sweep %d" % sweep)
        assert_bits(dx.cpu().numpy(), x, "x after sweep %d" % sweep)
    print("1-norm of the residual before every sweep:", " ".join("%.3g" % v for v in norms), "| floor %.3g" % floors[-1])
    above = [k for k in range(20) if norms[k] > floors[k]]
    assert above == list(range(len(above))) and len(above) >= 10, "the residual gets under the floor once, after ten sweeps or more"
    assert all(norms[k + 1] < norms[k] for k in above), norms
    assert all(norms[k] <= floors[k] for k in range(len(above), 20)), norms
    P.close()
    H.close()


# ========================================================================================================================= 9. state
def products(torch, H, n, dx):
    """Two products of the handle (the tile kernel's sweep direction may alternate)."""
    out = []
    for _ in range(2):
        buf, dy = guarded_y(torch, n)
        H.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, n)
        out.append(dy.cpu().numpy())
    return out


def test_the_handles_state_is_left_alone(torch):
    M = tm.existing_cases()[6]                                                        # memplus: wide launches and chains
    H = handle_of(M)
    name = H.describe()
    dx = dev(torch, tm.rhs(M.n, 17))
    before = products(torch, H, M.n, dx)
    L, U = H.trsv_plan(LOWER), H.trsv_plan(UPPER, UNIT)
    for now in (products(torch, H, M.n, dx),):
        for a, b in zip(now, before):
            assert_bits(a, b, "a product after create")
    assert_bits(solve_once(torch, L, M.n, M.reference(LOWER, STORED)[0]), M.reference(LOWER, STORED)[1], "lower")
    assert_bits(solve_once(torch, U, M.n, M.reference(UPPER, UNIT)[0]), M.reference(UPPER, UNIT)[1], "upper, beside the lower plan")
    for a, b in zip(products(torch, H, M.n, dx), before):
        assert_bits(a, b, "a product after the solves")
    L.close()
    U.close()
    assert H.describe() == name
    for a, b in zip(products(torch, H, M.n, dx), before):
        assert_bits(a, b, "a product after the plans are destroyed")
    L = H.trsv_plan(LOWER)                                                            # and the handle still plans and solves
    assert_bits(solve_once(torch, L, M.n, M.reference(LOWER, STORED)[0]), M.reference(LOWER, STORED)[1], "a new plan")
    L.close()
    H.close()


# ===================================================================================================================== 10. refusals
def test_invalid_arguments_are_refused_and_nothing_is_written(torch):
    L_ = sm.lib()
    M = tm.existing_cases()[4]                                                        # ibm32
    n = M.n
    H = handle_of(M)
    out = C.c_void_p()
    for uplo, diag, word in ((-1, STORED, "uplo"), (2, STORED, "uplo"), (LOWER, -1, "diag"), (LOWER, 2, "diag")):
        assert L_.smvp_csr_trsv_create(C.byref(out), H._h, uplo, diag, None) == sm.ERR_INVALID
        assert word in L_.smvp_last_error().decode() and out.value is None
    assert L_.smvp_csr_trsv_create(None, H._h, LOWER, STORED, None) == sm.ERR_INVALID and b"out" in L_.smvp_last_error()
    assert L_.smvp_csr_trsv_create(C.byref(out), None, LOWER, STORED, None) == sm.ERR_INVALID and out.value is None
    R = sm.CsrMatrix(3, 4, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 3], np.int32), np.ones(3))
    assert L_.smvp_csr_trsv_create(C.byref(out), R._h, LOWER, STORED, None) == sm.ERR_INVALID
    assert b"square" in L_.smvp_last_error() and out.value is None
    R.close()

    P = H.trsv_plan(LOWER)
    buf = torch.full((2 * n + 1,), SENTINEL, dtype=torch.float64, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        assert (buf.cpu().numpy() == SENTINEL).all(), "a refused call wrote something"

    assert L_.smvp_trsv_solve(None, sm._dev_ptr(buf[:n]), sm._dev_ptr(buf[n:2 * n]), None) == sm.ERR_INVALID
    assert b"plan" in L_.smvp_last_error()
    assert L_.smvp_trsv_solve(P._t, None, sm._dev_ptr(buf[:n]), None) == sm.ERR_INVALID and b"d_b" in L_.smvp_last_error()
    assert L_.smvp_trsv_solve(P._t, sm._dev_ptr(buf[:n]), None, None) == sm.ERR_INVALID and b"d_x" in L_.smvp_last_error()
    for shift in (1, -1, n - 1):                                                       # d_x one element off d_b, either way; one shared
        b0 = 1 if shift < 0 else 0
        assert L_.smvp_trsv_solve(P._t, sm._dev_ptr(buf[b0:b0 + n]), sm._dev_ptr(buf[b0 + shift:b0 + shift + n]), None) == sm.ERR_INVALID
        assert b"overlap" in L_.smvp_last_error()
    untouched()
    i = sm.TrsvInfo()
    i.struct_size = C.sizeof(sm.TrsvInfo) - 8
    i.levels = -7
    assert L_.smvp_trsv_info(P._t, C.byref(i)) == sm.ERR_INVALID and i.levels == -7 and b"struct_size" in L_.smvp_last_error()
    assert L_.smvp_trsv_info(P._t, None) == sm.ERR_INVALID
    with pytest.raises(ValueError):
        P.solve(torch.zeros(n + 1, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        P.solve(torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        P.solve(torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        P.solve(torch.zeros(2 * n, dtype=torch.float64, device="cuda")[::2], torch.zeros(n, dtype=torch.float64, device="cuda"))
    assert P.matrix is H, "the plan keeps its matrix alive"
    b, want = M.reference(LOWER, STORED)
    assert_bits(solve_once(torch, P, n, b), want, "after the refusals the plan solves")
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
    assert L_.smvp_csr_trsv_create(C.byref(out), inner, LOWER, STORED, None) == sm.ERR_UNSUPPORTED
    assert b"plain CSR" in L_.smvp_last_error() and out.value is None
    T.close()
    row_ptr, col_ind, val = A.csr
    lo, hi = 100, 400
    block = (row_ptr[lo:hi + 1] - row_ptr[lo]).astype(np.int32)
    B = sm.CsrMatrix(hi - lo, A.n, block, col_ind[row_ptr[lo]:row_ptr[hi]], val[row_ptr[lo]:row_ptr[hi]], first_row=lo)
    assert L_.smvp_csr_trsv_create(C.byref(out), B._h, LOWER, STORED, None) == sm.ERR_UNSUPPORTED
    assert b"first_row" in L_.smvp_last_error() and out.value is None
    with pytest.raises(sm.SmvpError):
        B.trsv_plan(UPPER)
    B.close()


def test_a_matrix_without_rows(torch):
    E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    for uplo, diag in BOTH:
        P = E.trsv_plan(uplo, diag)
        info = P.info()
        assert (info["levels"], info["launches"], info["chains"], info["max_level_width"], info["entries"], info["missing_diagonals"]) == (0,) * 6
        level_ptr, order = P.schedule()
        assert level_ptr.tolist() == [0] and order.tolist() == []
        assert sm.lib().smvp_trsv_solve(P._t, None, None, None) == sm.OK
        x = torch.empty(0, dtype=torch.float64, device="cuda")
        assert P.solve(x, x) is x
        P.close()
    E.close()
