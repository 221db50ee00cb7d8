"""GPU: ILU(0) on a CSR handle (smvp_csr_ilu0_create / smvp_ilu0_factor, kernel K17) against its restatement tests/ilu0_method.py
(test_ilu0_host.py pins that to hand-computed values, to the library's host loop and to a derived bound).

No tolerance anywhere: every element of F is the serial loop's.  Comparisons are transposed.assert_bits on every value read back
from the addresses Ilu0.matrix.device_arrays() reports (a NaN equals a NaN whatever its sign and payload, an Inf's sign is one of
its bits).  The constructed schedules are built from the chain width smvp_ilu0_info reports, not from a mirror of it."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

import cg_method as cg
import ilu0_method as im
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import test_gpu_pcg_tri as k16
import trsv_method as trsv
from parity import check_guards, guarded_y
from test_gpu_cg import PATHS, dev, handle
from test_gpu_transposed import _Raw, arrays_of, inner_csr_handle
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu

ALL = list(range(im.N_CONSTRUCTED + im.N_MORE))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def chain_width():
    """The library's constant, as smvp_ilu0_info reports it."""
    H = sm.CsrMatrix(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.ones(1))
    f = H.ilu0()
    w = f.info()["chain_width"]
    f.close()
    H.close()
    assert w >= 64
    return w


def handle_of(M):
    return sm.CsrMatrix(M.n, M.n, *M.csr)


def values_of(torch, f):
    """F's values, copied back after everything enqueued has finished."""
    torch.cuda.synchronize()
    return arrays_of(torch, f.matrix)[2]


def values_tensor(torch, f):
    """F's values as a tensor over the library's own memory: to poison them in front of a factorisation."""
    return torch.as_tensor(_Raw(f.matrix.device_arrays()[2], max(f.matrix.nnz, 1), "<f8"), device="cuda")


def products(torch, H, n, dx):
    out = []
    for _ in range(2):                                       # (the tile kernel's sweep direction may alternate: two products)
        buf, dy = guarded_y(torch, n)
        H.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, n)
        out.append(dy.cpu().numpy())
    return out


def solve_once(torch, P, n, b):
    buf, dx = guarded_y(torch, n)
    P.solve(dev(torch, b), dx)
    torch.cuda.synchronize()
    check_guards(buf, n)
    return dx.cpu().numpy()


# ========================================================================================================= 1. bits on every case
@pytest.mark.parametrize("i", ALL)
def test_every_element_of_the_factor_is_the_restatements(torch, i):
    M = im.case(chain_width(), i)
    want = im.factor(M).csr[2]
    H = handle_of(M)
    dx = dev(torch, trsv.rhs(M.n, 17))
    before = products(torch, H, M.n, dx), arrays_of(torch, H)
    f = H.ilu0()
    assert_bits(values_of(torch, f), want, M.name + ": after create")
    rp, ci, v = f.matrix.device_arrays()
    assert (rp, ci) == H.device_arrays()[:2] and v != H.device_arrays()[2] and v % 16 == 0, "F adopts A's pattern and has values of its own"
    assert (f.matrix.rows, f.matrix.cols, f.matrix.nnz) == (M.n, M.n, M.nnz)
    info, facts = f.info(), M.facts(LOWER, UNIT)
    for field in ("levels", "max_level_width"):
        assert info[field] == facts[field], "%s: %s is %r, the restatement's %r" % (M.name, field, info[field], facts[field])
    assert info["launches"] == trsv.launches(facts["widths"], info["chain_width"]), M.name
    assert info["chains"] == trsv.chains(facts["widths"], info["chain_width"]), M.name
    assert (info["entries"], info["pivots"]) == (M.nnz, facts["off"]), M.name
    assert info["plan_bytes"] >= 8 * M.nnz + 4 * (2 * M.n + facts["levels"] + 1) and info["build_ms"] >= 0.0
    assert info["lanes_per_row"] in (2, 4, 8, 16, 32, 64)
    poison = values_tensor(torch, f)
    poison.fill_(float("nan"))
    assert f.factor() is f
    assert_bits(values_of(torch, f), want, M.name + ": factor() again, over NaNs")
    poison.fill_(float("nan"))
    torch.cuda.synchronize()
    f.factor(stream=torch.cuda.Stream())
    assert_bits(values_of(torch, f), want, M.name + ": factor() on a stream of the caller's")
    for got, was in zip(arrays_of(torch, H), before[1]):
        assert got.tobytes() == was.tobytes(), M.name + ": A's arrays changed"
    for got, was in zip(products(torch, H, M.n, dx), before[0]):
        assert_bits(got, was, M.name + ": a product on A afterwards")
    print("%s: %d rows, %d entries, %d pivots, %d levels (widest %d), %d launches of which %d chains, %d lanes a row, build %.2f ms"
          % (M.name, M.n, M.nnz, info["pivots"], info["levels"], info["max_level_width"], info["launches"], info["chains"],
             info["lanes_per_row"], info["build_ms"]))
    f.close()
    H.close()


def test_the_chain_width_option_changes_the_launches_and_no_bit(torch):
    w = chain_width()
    M = im.case(w, 9)                                        # wide_thin_wide: 4 launches by default
    assert M.name.startswith("wide_thin_wide")
    H = handle_of(M)
    seen = []
    for width in (w, 2 * w, 4 * w):
        with sm.option("trsv_chain_width", width):
            f = H.ilu0()
        info = f.info()
        assert info["chain_width"] == width and info["launches"] == trsv.launches(M.facts(LOWER, UNIT)["widths"], width)
        assert_bits(values_of(torch, f), im.factor(M).csr[2], "%s at a chain width of %d" % (M.name, width))
        seen.append(info["launches"])
        f.close()
    assert seen[0] == 4 and seen[0] > seen[1] > seen[2] == 1
    H.close()


# ============================================================================================================ 2. re-factorisation
def test_new_values_on_the_old_pattern_are_factorised_and_old_plans_see_them(torch):
    M = im.case(chain_width(), 9)
    r, c, _ = M.entries()
    M2 = trsv.dominant(M.name + ", second values", M.n, r, c, 20450)
    assert (M2.csr[1] == M.csr[1]).all()
    rp, ci, v = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in M.csr)
    H = sm.CsrMatrix(M.n, M.n, rp, ci, v)
    f = H.ilu0()
    L, U = f.plans()
    assert (L.uplo, L.diag, U.uplo, U.diag) == (LOWER, UNIT, UPPER, STORED) and L.matrix is f.matrix
    b = trsv.rhs(M.n)
    F1 = im.factor(M)
    assert_bits(solve_once(torch, L, M.n, b), trsv.solve(F1, LOWER, UNIT, b), "L of the first factor")
    v.copy_(dev(torch, M2.csr[2]))
    f.factor()
    F2 = im.factor(M2)
    assert not np.array_equal(F2.csr[2], F1.csr[2])
    assert_bits(values_of(torch, f), F2.csr[2], "the second values' factor")
    assert_bits(v.cpu().numpy(), M2.csr[2], "A's values are only read")
    w = trsv.solve(F2, LOWER, UNIT, b)
    assert_bits(solve_once(torch, L, M.n, b), w, "the old LOWER / UNIT plan on the new factor")
    assert_bits(solve_once(torch, U, M.n, w), trsv.solve(F2, UPPER, STORED, w), "the old UPPER / STORED plan on the new factor")
    for X in (L, U, f, H):
        X.close()


# =================================================================================================================== 3. capture
def test_factor_and_both_solves_are_captured_as_the_objects_first_calls(torch):
    M = im.case(chain_width(), 9)                            # wide launches and chains
    F = im.factor(M)
    b = trsv.rhs(M.n, 18)
    w = trsv.solve(F, LOWER, UNIT, b)
    want = trsv.solve(F, UPPER, STORED, w)
    H = handle_of(M)
    f = H.ilu0()
    L, U = f.plans()
    db = dev(torch, b)
    buf, dz = guarded_y(torch, M.n)
    fv = values_tensor(torch, f)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            rc = sm.lib().smvp_ilu0_factor(f._f, s.cuda_stream)
            L.solve(db, dz, stream=s)
            U.solve(dz, dz, stream=s)
    assert rc == sm.OK, sm.lib().smvp_last_error().decode()
    for _ in range(2):
        dz.fill_(float("nan"))
        fv.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        check_guards(buf, M.n)
        assert_bits(fv.cpu().numpy(), F.csr[2], "F after the replayed capture")
        assert_bits(dz.cpu().numpy(), want, "z = U^-1 L^-1 b after the replayed capture")
    del g
    for X in (L, U, f, H):
        X.close()


# ==================================================================================================================== 4. the solver
@functools.lru_cache(maxsize=None)
def system(name):
    Cs = {"lap2d(16)": lambda: im.grid(16), "lap2d(32)": lambda: im.grid(32), "spd(1003)": im.spd_1003}[name]()
    return im.as_matrix(Cs), Cs


@pytest.mark.parametrize("fmt,a,b", PATHS)
def test_pcg_tri_with_the_factors_plans_is_the_restatements_run(torch, fmt, a, b):
    for name in ("lap2d(16)", "lap2d(32)", "spd(1003)"):
        M, Cs = system(name)
        A = handle_of(Cs)
        f = A.ilu0()
        first, second = f.plans()
        P = type("P", (), dict(first=first, second=second, m=None))
        H, product = handle(torch, M, fmt, a, b)
        rhs = cg.rhs(M.n)
        want = tri.run(product, rhs, None, *im.plans(im.factor(Cs)), k16.MAX_STEPS, k16.TOL)
        assert want[2] == tri.CONVERGED and want[0] < k16.MAX_STEPS, "%s: the restatement did not converge" % name
        for every in (1, 10):
            got = k16.solve(torch, H, M.n, rhs, P, None, k16.MAX_STEPS, k16.TOL, every)
            k16.same(got, want, "%s, %s %d %d, check_every %d" % (name, fmt, a, b, every), rhs)
        print("%s, %s %d %d: %d steps with ILU(0)" % (name, fmt, a, b, want[0]))
        for X in (first, second, f, A, H):
            X.close()


def test_the_whole_use_through_the_python_methods(torch):
    M, Cs = system("lap2d(32)")
    A = handle_of(Cs)
    f = A.ilu0()
    first, second = f.plans()
    rhs = cg.rhs(M.n)
    dx = torch.empty(M.n, dtype=torch.float64, device="cuda")
    r, rr, rz, sigma = A.pcg_tri(dev(torch, rhs), dx, first, second, max_steps=200, tol=k16.TOL, check_every=1)
    L, U = A.trsv_plan(LOWER), A.trsv_plan(UPPER)
    dm = A.diagonal(torch.empty(M.n, dtype=torch.float64, device="cuda"))
    sgs = A.pcg_tri(dev(torch, rhs), torch.empty_like(dx), L, U, m=dm, max_steps=200, tol=k16.TOL)[0]
    print("lap2d(32): ILU(0) %d steps, SGS %d" % (r.steps, sgs.steps))
    assert r.reason == sgs.reason == sm.CG_CONVERGED and r.steps < sgs.steps
    for X in (first, second, L, U, f, A):
        X.close()


# ====================================================================================================================== 5. refusals
def refused(h, stream=None):
    out = C.c_void_p()
    rc = sm.lib().smvp_csr_ilu0_create(C.byref(out), h, stream)
    return rc, out.value, sm.lib().smvp_last_error().decode()


def test_what_does_not_qualify_is_refused_and_out_is_untouched(torch):
    L_ = sm.lib()
    A = cg.spd(1003)
    for M, word in ((trsv.of_matrix("spd(1003)", A), "repeated"),
                    (trsv.of_matrix("spd_shuffled", cg.spd_shuffled(), as_stored=True), "column"),
                    (trsv.sample("pdp08-pg4"), "no diagonal")):
        H = handle_of(M)
        rc, out, msg = refused(H._h)
        assert (rc, out) == (sm.ERR_UNSUPPORTED, None) and word in msg and "row " in msg, msg
        with pytest.raises(sm.SmvpError):
            H.ilu0()
        H.close()
    row_ptr, col_ind, val = im.spd_1003().csr
    lo, hi = 100, 400
    block = (row_ptr[lo:hi + 1] - row_ptr[lo]).astype(np.int32)
    B = sm.CsrMatrix(hi - lo, 1003, block, col_ind[row_ptr[lo]:row_ptr[hi]], val[row_ptr[lo]:row_ptr[hi]], first_row=lo)
    rc, out, msg = refused(B._h)
    assert (rc, out) == (sm.ERR_UNSUPPORTED, None) and "first_row" in msg
    B.close()
    T = sm.TjdsMatrix(sm.tjds_from_coo(A.coo, A.n, A.n))
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    T.set_x(dev(torch, np.ones(A.n)))
    T.spmv(torch.empty(A.n, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    rc, out, msg = refused(inner_csr_handle(T, A.n, A.n, A.nnz))
    assert (rc, out) == (sm.ERR_UNSUPPORTED, None) and "plain CSR" in msg
    T.close()
    R = sm.CsrMatrix(3, 4, np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 2], np.int32), np.ones(3))
    rc, out, msg = refused(R._h)
    assert (rc, out) == (sm.ERR_INVALID, None) and "square" in msg
    R.close()
    assert refused(None)[:2] == (sm.ERR_INVALID, None)
    H = handle_of(im.case(chain_width(), 17))
    assert L_.smvp_csr_ilu0_create(None, H._h, None) == sm.ERR_INVALID
    f = H.ilu0()
    i = sm.Ilu0Info()
    i.struct_size = C.sizeof(sm.Ilu0Info) - 8
    i.levels = -7
    assert L_.smvp_ilu0_info(f._f, C.byref(i)) == sm.ERR_INVALID and i.levels == -7 and b"struct_size" in L_.smvp_last_error()
    assert L_.smvp_ilu0_info(f._f, None) == sm.ERR_INVALID and L_.smvp_ilu0_info(None, C.byref(i)) == sm.ERR_INVALID
    assert L_.smvp_ilu0_factor(None, None) == sm.ERR_INVALID
    out = C.c_void_p(7)
    assert L_.smvp_ilu0_matrix(None, C.byref(out)) == sm.ERR_INVALID and out.value == 7
    assert L_.smvp_ilu0_matrix(f._f, None) == sm.ERR_INVALID
    assert_bits(values_of(torch, f), im.factor(im.case(chain_width(), 17)).csr[2], "after the refusals")
    f.close()
    H.close()


def test_create_refuses_a_capturing_stream_and_the_capture_stays_valid(torch):
    H = handle_of(im.case(chain_width(), 17))
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    got = []
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dZ.add_(1.0)
            got.append(refused(H._h, s.cuda_stream))
            dZ.add_(1.0)
    assert got[0][:2] == (sm.ERR_INVALID, None) and "captur" in got[0][2]
    g.replay()
    torch.cuda.synchronize()
    assert dZ.cpu().numpy().tolist() == [2.0] * 16
    del g
    H.close()


def test_no_rows_and_one_row(torch):
    E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
    f = E.ilu0()
    info = f.info()
    assert (info["levels"], info["launches"], info["chains"], info["max_level_width"], info["entries"], info["pivots"]) == (0,) * 6
    assert f.factor() is f
    L, U = f.plans()
    x = torch.empty(0, dtype=torch.float64, device="cuda")
    assert L.solve(x, x) is x and U.solve(x, x) is x
    for X in (L, U, f, E):
        X.close()
    one = sm.CsrMatrix(1, 1, np.array([0, 1], np.int32), np.zeros(1, np.int32), np.array([-2.5]))
    f = one.ilu0()
    info = f.info()
    assert (info["levels"], info["launches"], info["chains"], info["entries"], info["pivots"]) == (1, 1, 1, 1, 0)
    assert_bits(values_of(torch, f), [-2.5], "n = 1")
    f.close()
    one.close()


# ================================================================================================================ 6. non-finite
def test_a_zero_pivot_gives_the_restatements_infinities_and_nans(torch):
    Cs = im.case(chain_width(), 8)                           # dense_lower(70), symmetrised: every row divides by u_00
    Z = tri.zero_diagonal(im.as_matrix(Cs), 0)               # row 0 has no pivot: u_00 is the stored zero
    assert (Z.csr[1] == Cs.csr[1]).all()
    want = im.ilu0(Z, finite=False).csr[2]
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    H = handle_of(Z)
    out = C.c_void_p()
    assert sm.lib().smvp_csr_ilu0_create(C.byref(out), H._h, None) == sm.OK
    sm.lib().smvp_ilu0_destroy(out)
    f = H.ilu0()
    got = values_of(torch, f)
    assert_bits(got, want, "a zero stored at (0, 0)")      # (a NaN equals a NaN; an Inf's sign is one of its bits)
    assert (np.isnan(got) == np.isnan(want)).all() and (np.isinf(got) == np.isinf(want)).all()
    assert sm.lib().smvp_ilu0_factor(f._f, None) == sm.OK
    assert_bits(values_of(torch, f), want, "factor() again")
    f.close()
    H.close()


# ======================================================================================================================= 7. lifetime
def test_the_borrowed_matrix_and_objects_side_by_side(torch):
    M = im.case(chain_width(), 20)                           # pwt
    assert M.name == "pwt"
    want = im.factor(M).csr[2]
    H = handle_of(M)
    name = H.describe()
    f1, f2 = H.ilu0(), H.ilu0()
    T = H.trsv_plan(LOWER)
    b, x = M.reference(LOWER, STORED)
    h = f1.matrix._h.value
    f1.matrix.close()                                        # destroys nothing: the handle is f1's
    assert f1.matrix._h.value == h
    assert_bits(values_of(torch, f1), want, "the first factorisation after matrix.close()")
    assert f1.matrix.device_arrays()[2] != f2.matrix.device_arrays()[2]
    assert_bits(values_of(torch, f2), want, "the second, beside it")
    assert_bits(solve_once(torch, T, M.n, b), x, "a plan on A beside them")
    L1, U1 = f1.plans()
    f2.factor()
    w = trsv.solve(im.factor(M), LOWER, UNIT, b)
    assert_bits(solve_once(torch, L1, M.n, b), w, "f1's plan while f2 factorises again")
    dx = dev(torch, trsv.rhs(M.n, 17))
    G = handle_of(im.factor(M))                              # F is an ordinary handle: its product is that of the same arrays uploaded
    for got, ref in zip(products(torch, f1.matrix, M.n, dx), products(torch, G, M.n, dx)):
        assert_bits(got, ref, "the product of F's handle")
    G.close()
    assert H.describe() == name
    f2.close()
    assert_bits(values_of(torch, f1), want, "the first after the second is destroyed")
    for X in (L1, U1, T, f1):
        X.close()
    assert not f1.matrix._h
    T = H.trsv_plan(LOWER)
    assert_bits(solve_once(torch, T, M.n, b), x, "A after everything on it is closed")
    T.close()
    H.close()


def test_plans_and_the_borrowed_matrix_keep_the_factorisation_alive(torch):
    """`L, U = A.ilu0().plans()` drops the caller's only reference to the Ilu0 at once: the plans keep `matrix`, and `matrix` keeps
    the Ilu0 that owns its handle and its values, so nothing is freed under them."""
    M = im.case(chain_width(), 9)
    F = im.factor(M)
    H = handle_of(M)
    L, U = H.ilu0().plans()
    Fm = H.ilu0().matrix                                     # a second factorisation of which only the matrix is kept
    gc.collect()
    spare = [torch.full((M.nnz,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4)]   # (would reuse freed blocks)
    torch.cuda.synchronize()
    owner = L.matrix._keep
    assert isinstance(owner, sm.Ilu0) and owner._f and U.matrix is L.matrix and isinstance(Fm._keep, sm.Ilu0) and Fm._keep._f
    b = trsv.rhs(M.n, 19)
    w = trsv.solve(F, LOWER, UNIT, b)
    assert_bits(solve_once(torch, L, M.n, b), w, "the LOWER plan of a factorisation nobody else holds")
    assert_bits(solve_once(torch, U, M.n, w), trsv.solve(F, UPPER, STORED, w), "the UPPER plan likewise")
    assert_bits(arrays_of(torch, Fm)[2], F.csr[2], "the values behind a matrix whose Ilu0 nobody else holds")
    del spare
    other = Fm._keep
    for X in (L, U, owner, other):
        X.close()
    assert not Fm._h and Fm._keep is None and owner.matrix._keep is None
    H.close()
