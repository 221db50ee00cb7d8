"""Host checks of tests/pcg_tri_method.py, the numpy restatement of conjugate gradients preconditioned by two triangular solves
(include/smvp_amd.h, K16): hand-computed runs, the restatements of K14 and K12 it must fall back to bit for bit, the true residual
of what it calls converged, what symmetric Gauss-Seidel buys where Jacobi cannot, every stop rule -- so that test_gpu_pcg_tri.py
compares the library with a reference that is what it claims.  And what of the C ABI needs no device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import cg_method as cg
import pcg_method as pcg
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import trsv_method as trsv
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_pcg_tri", "smvp_tjds_pcg_tri")
TOL = 1e-8


@functools.lru_cache(maxsize=None)
def system(name):
    """(matrix, b, (first, m, second)): the systems of this file with symmetric Gauss-Seidel on the matrix itself; "ic0" is
    lap2d(16) with its incomplete Cholesky factor and no m."""
    M = {"lap2d(32)": lambda: tri.lap2d(32), "scaled(1003)": lambda: pcg.scaled(cg.spd(1003), 2), "spd(3001)": lambda: cg.spd(3001),
         "ic0": lambda: tri.lap2d(16)}[name]()
    if name == "ic0":
        F, Ft = tri.ic0(M)
        plans = (F, tri.LOWER, tri.STORED), None, (Ft, tri.UPPER, tri.STORED)
    else:
        plans = tri.sgs(trsv.of_matrix(name, M))
    return M, cg.rhs(M.n), plans


@functools.lru_cache(maxsize=None)
def solved(name):
    M, b, (first, m, second) = system(name)
    return tri.run(M.spmv, b, None, first, m, second, 200, TOL)


# ------------------------------------------------------------------------------------------------------------ computed by hand
def test_a_hand_computed_two_by_two_case():
    """A = [[2, 1], [1, 2]], symmetric Gauss-Seidel on it (m = (2, 2)), b = (4, 4).  r_0 = (4, 4); w = ((4)/2, (4 - 2)/2) = (2, 1);
    v = (4, 2); z_1 = 2/2 = 1, z_0 = (4 - 1)/2 = 3/2.  rr_0 = 32, rho_0 = 6 + 4 = 10, q_1 = A z_0 = (4, 7/2), sigma_1 = 6 + 7/2 = 19/2."""
    M = pcg.pi.Matrix(2, [0, 0, 1, 1], [0, 1, 0, 1], [2.0, 1.0, 1.0, 2.0])
    first, m, second = tri.sgs(trsv.of_matrix("2 x 2", M))
    assert_bits(m, [2.0, 2.0], "the diagonal")
    b = np.array([4.0, 4.0])
    assert_bits(tri.apply(first, m, second, b), [1.5, 1.0], "z_0")
    steps, updates, reason, rr, rz, sigma, x = tri.run(M.spmv, b, None, first, m, second, 1, 0.0)
    assert (steps, updates, reason) == (1, 1, tri.MAX_STEPS)
    assert rr[0] == 32.0 and rz[0] == 10.0 and sigma[0] == 9.5
    alpha = np.float64(10.0) / np.float64(9.5)
    assert_bits(x, [alpha * 1.5, alpha * 1.0], "x_1 = alpha_1 z_0")
    r1 = np.array([4.0 - alpha * 4.0, 4.0 - alpha * 3.5])
    w0 = r1[0] / 2.0
    w1 = (r1[1] - 1.0 * w0) / 2.0
    z1 = (2.0 * w1) / 2.0
    z0 = (2.0 * w0 - 1.0 * z1) / 2.0
    assert_bits([rr[1]], [r1[0] * r1[0] + r1[1] * r1[1]], "rr_1")
    assert_bits([rz[1]], [r1[0] * z0 + r1[1] * z1], "rho_1 = r_1 . z_1")
    full = tri.run(M.spmv, b, None, first, m, second, 10, 1e-12)                     # two steps solve a 2 x 2 system
    assert full[2] == tri.CONVERGED and full[0] == 2
    assert np.allclose(full[6], np.linalg.solve(cg.dense(M), b), rtol=1e-14, atol=0.0)


def test_a_hand_computed_three_by_three_case_with_an_exact_factor():
    """F = [[2, 0, 0], [1, 2, 0], [0, 1, 2]], A = F F^T = [[4, 2, 0], [2, 5, 2], [0, 2, 5]], no m, b = (8, 0, 0): w = (4, -2, 1),
    z_2 = 1/2, z_1 = (-2 - 1/2)/2 = -5/4, z_0 = (4 + 5/4)/2 = 21/8.  M is A itself, so q_1 = A z_0 = b, rho_0 = sigma_1 = 21, alpha_1 =
    1, x_1 = z_0 and r_1 = 0: converged in one step, every number dyadic."""
    A = pcg.pi.Matrix(3, [0, 0, 1, 1, 1, 2, 2], [0, 1, 0, 1, 2, 1, 2], [4.0, 2.0, 2.0, 5.0, 2.0, 2.0, 5.0])
    F = trsv.Case("F", 3, [0, 1, 1, 2, 2], [0, 0, 1, 1, 2], [2.0, 1.0, 2.0, 1.0, 2.0])
    Ft = trsv.Case("F^T", 3, [0, 0, 1, 1, 2], [0, 1, 1, 2, 2], [2.0, 1.0, 2.0, 1.0, 2.0])
    b = np.array([8.0, 0.0, 0.0])
    first, second = (F, tri.LOWER, tri.STORED), (Ft, tri.UPPER, tri.STORED)
    assert_bits(tri.apply(first, None, second, b), [2.625, -1.25, 0.5], "z_0")
    steps, updates, reason, rr, rz, sigma, x = tri.run(A.spmv, b, None, first, None, second, 10, 0.0)
    assert (steps, updates, reason) == (1, 1, tri.CONVERGED)
    assert_bits(rr, [64.0, 0.0], "rr_each")
    assert_bits(rz, [21.0, 0.0], "rz_each")
    assert_bits(sigma, [21.0], "sigma_each")
    assert_bits(x, [2.625, -1.25, 0.5], "x_1")
    ones = np.ones(3)                                                                # an m of ones changes no bit
    assert_bits(tri.run(A.spmv, b, None, first, ones, second, 10, 0.0)[6], x, "m = ones")
    # the other triangle is skipped, not refused: the same plans on A's full storage with F's values in place
    both = trsv.Case("F and F^T in one matrix", 3, [0, 0, 1, 1, 1, 2, 2], [0, 1, 0, 1, 2, 1, 2], [2.0, 1.0, 1.0, 2.0, 1.0, 1.0, 2.0])
    assert_bits(tri.apply((both, tri.LOWER, tri.STORED), None, (both, tri.UPPER, tri.STORED), b), [2.625, -1.25, 0.5], "one handle")


# ------------------------------------------------------------------------------------- what it must fall back to, bit for bit
@pytest.mark.parametrize("name", ["scaled", "spd_shuffled"])
def test_diagonal_only_plans_are_jacobi_pcg_bit_for_bit(name):
    M = pcg.scaled(cg.spd(1003), 2) if name == "scaled" else cg.spd_shuffled()
    d = pcg.diagonal(M)
    first, m, second = tri.diagonal_only(d)
    assert m is None
    b = cg.rhs(M.n)
    for x0 in (None, np.random.default_rng(9).uniform(-2.0, 2.0, M.n)):
        for tol, steps in ((1e-8, 40), (0.0, 6)):
            want = pcg.run(M.spmv, b, x0, d, steps, tol)
            got = tri.run(M.spmv, b, x0, first, m, second, steps, tol)
            assert got[:3] == want[:3]
            for i, what in ((3, "rr_each"), (4, "rz_each"), (5, "sigma_each"), (6, "x")):
                assert_bits(got[i], want[i], "%s: %s" % (name, what))


def test_signed_zeros_pass_the_diagonal_only_plans():
    first, m, second = tri.diagonal_only(np.array([2.0, 4.0, 8.0]))
    r = np.array([-0.0, 0.0, -3.0])
    assert_bits(tri.apply(first, m, second, r), r / np.array([2.0, 4.0, 8.0]), "r_i - (+0.0) is r_i")


@pytest.mark.parametrize("name", ["spd", "spd_long"])
def test_identity_plans_and_an_m_of_ones_are_plain_cg_bit_for_bit(name):
    M = cg.spd(300) if name == "spd" else cg.spd_long()
    I = trsv.Case("identity", M.n, np.arange(M.n), np.arange(M.n), np.ones(M.n))
    b = cg.rhs(M.n)
    for first, second in (((I, tri.LOWER, tri.STORED), (I, tri.UPPER, tri.STORED)), ((I, tri.LOWER, tri.UNIT), (I, tri.LOWER, tri.UNIT))):
        for x0 in (None, np.random.default_rng(9).uniform(-2.0, 2.0, M.n)):
            for tol, steps in ((1e-10, 40), (0.0, 12)):
                want = cg.run(M.spmv, b, x0, steps, tol)
                got = tri.run(M.spmv, b, x0, first, np.ones(M.n), second, steps, tol)
                assert got[:3] == want[:3]
                assert_bits(got[3], want[3], "rr_each")
                assert_bits(got[4], want[3], "rz_each is rr_each: z is r")
                assert_bits(got[5], want[4], "sigma_each")
                assert_bits(got[6], want[5], "x")


# ------------------------------------------------------------------------------------------------ what it calls converged
@pytest.mark.parametrize("name", ["lap2d(32)", "scaled(1003)", "spd(3001)", "ic0"])
def test_the_true_residual_of_a_converged_run(name):
    """|b - A x| <= 2 tol |b|: the rule stops on the recurrence's r, not on the true residual, hence the factor 2."""
    M, b, plans = system(name)
    steps, updates, reason, rr, rz, sigma, x = solved(name)
    true = np.linalg.norm(b - cg.dense(M) @ x) / np.linalg.norm(b)
    print("%s: %d steps, reason %d, |b - A x| / |b| = %.3g = %.2f tol" % (name, steps, reason, true, true / TOL))
    assert reason == tri.CONVERGED and steps == updates < 200
    assert true <= 2.0 * TOL


# ---------------------------------------------------------------------------------------------- what the triangles buy
def test_sgs_halves_the_steps_where_the_diagonal_is_constant():
    M, b, plans = system("lap2d(32)")
    d = pcg.diagonal(M)
    assert (d == 4.0).all()
    jacobi = pcg.run(M.spmv, b, None, d, 200, TOL)
    plain = cg.run(M.spmv, b, None, 200, TOL)
    got = solved("lap2d(32)")
    print("lap2d(32): cg %d, Jacobi %d, SGS %d steps" % (plain[0], jacobi[0], got[0]))
    assert jacobi[2] == pcg.CONVERGED and got[2] == tri.CONVERGED and jacobi[0] < 200
    assert jacobi[0] == plain[0]                                                     # a constant diagonal: Jacobi is plain CG's steps
    assert 2 * got[0] <= jacobi[0]


def test_sgs_needs_no_more_steps_than_jacobi_on_a_badly_scaled_system():
    M, b, plans = system("scaled(1003)")
    jacobi = pcg.run(M.spmv, b, None, pcg.diagonal(M), 60, TOL)
    got = solved("scaled(1003)")
    print("scaled(1003): Jacobi %d, SGS %d steps" % (jacobi[0], got[0]))
    assert jacobi[2] == pcg.CONVERGED and got[2] == tri.CONVERGED and got[0] <= jacobi[0]


def test_an_incomplete_factor_beats_jacobi():
    M, b, (first, m, second) = system("ic0")
    F, Ft = first[0], second[0]
    r, c, v = F.entries()
    assert (c <= r).all() and (Ft.entries()[1] >= Ft.entries()[0]).all()
    dense_f = np.zeros((M.n, M.n))
    dense_f[r, c] = v
    rt, ct, vt = Ft.entries()
    dense_ft = np.zeros((M.n, M.n))
    dense_ft[rt, ct] = vt
    assert (dense_ft == dense_f.T).all()
    A = cg.dense(M)
    assert np.allclose((dense_f @ dense_f.T)[A != 0.0], A[A != 0.0], rtol=1e-13, atol=0.0)   # IC(0): exact on A's pattern
    jacobi = pcg.run(M.spmv, b, None, pcg.diagonal(M), 200, TOL)
    got = solved("ic0")
    print("lap2d(16): Jacobi %d, IC(0) %d steps" % (jacobi[0], got[0]))
    assert got[2] == tri.CONVERGED and jacobi[2] == pcg.CONVERGED and got[0] < jacobi[0]


# ------------------------------------------------------------------------------------------------------------- the stop rules
def test_every_stop_rule():
    for name, M, b, (first, m, second), tol, expect in tri.stop_cases():
        steps, updates, reason, rr, rz, sigma, x = tri.run(M.spmv, b, None, first, m, second, 10, tol)
        assert (steps, updates, reason) == expect, "%s: %r" % (name, (steps, updates, reason))
        assert len(rr) == len(rz) == updates + 1 and len(sigma) == steps, name
        if updates == 0:
            assert_bits(x, np.zeros(M.n), name + ": x is unchanged")
    cases = {c[0]: c for c in tri.stop_cases()}
    name, M, b, (first, m, second), tol, expect = cases["a zero stored diagonal in first's triangle"]
    got = tri.run(M.spmv, b, None, first, m, second, 10, tol)
    assert np.isfinite(got[3][0]) and not np.isfinite(got[4][0])                     # rr_0 is fine, rho_0 is not
    name, M, b, (first, m, second), tol, expect = cases["m = -diag"]
    got = tri.run(M.spmv, b, None, first, m, second, 10, tol)
    assert got[4][0] < 0.0
    name, M, b, (first, m, second), tol, expect = cases["max_steps"]
    longer = tri.run(M.spmv, b, None, first, m, second, 12, tol)
    assert_bits(tri.run(M.spmv, b, None, first, m, second, 10, tol)[3], longer[3][:11], "the first steps of a longer run")


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_pcg_tri_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert len(getattr(sm.lib(), name).argtypes) == 13, name


def call(fn, h, o, b, first, second, result):
    r = sm.PcgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, first, None, second,
                               C.byref(r) if result else None, None, None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """K14's checks in K14's order (a NULL d_m is no error here), then the plans: they come before the handle is looked at and
    before any HIP call, so blocks of zeros stand in for a handle and for the plans."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    t = C.cast(C.create_string_buffer(4096), C.c_void_p)
    ok = sm.cg_opts(5)
    assert call(fn, None, ok, b, t, t, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, t, t, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, t, t, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, t, t, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    assert call(fn, h, ok, b, None, t, True) == (sm.ERR_INVALID, b"%s: null first plan" % fn.encode())
    assert call(fn, h, ok, b, t, None, True) == (sm.ERR_INVALID, b"%s: null second plan" % fn.encode())
    assert call(fn, h, ok, b, None, None, True) == (sm.ERR_INVALID, b"%s: null first plan" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.cg_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, t, t, True)
        assert rc == sm.ERR_INVALID and (b"smvp_cg_opts_t" in msg if field == "struct_size" else b"tol" in msg), (field, value, msg)


def test_the_python_calls_refuse_what_is_no_open_plan_before_the_library_is_called():
    import torch
    v = torch.ones(4, dtype=torch.float64)

    class Closed(sm.TrsvPlan):
        def __init__(self):
            self._t = C.c_void_p()

    for first, second in ((None, Closed()), (Closed(), Closed()), (object(), object()), (3, 4)):
        with pytest.raises(ValueError):
            sm._pcg_tri("smvp_no_such_function", None, v, v, first, second, None, None, 5, 1e-10, 1, None)
