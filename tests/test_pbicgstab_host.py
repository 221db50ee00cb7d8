"""Host checks of tests/pbicgstab_method.py, the numpy restatement of right-preconditioned BiCGSTAB as include/smvp_amd.h defines it
(K18): the two identities with bicgstab_method.run bit for bit, an exact case, K13's rule cases under identity plans, the
non-finite preconditioners, the true residual under every preconditioner and what the preconditioners are for -- so that
test_gpu_pbicgstab.py compares the library with a reference that is what it claims.  And what of the C ABI needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_method as bi
import pbicgstab_method as pb
import smvp_toolkit_amd as sm
import trsv_method as trsv
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_pbicgstab", "smvp_tjds_pbicgstab")
TOL = 1e-8
SYSTEMS = ("convdiff(32, 0.5)", "nonsym(1003), coalesced")
KINDS = ("plain", "jacobi", "sgs", "ilu0")


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, n)


def preconditioner(kind, Cs):
    return pb.plain() if kind == "plain" else getattr(pb, kind)(Cs)


@pytest.fixture(scope="module")
def solved():
    """{(system, kind): (run's tuple, the true relative residual)} at tol = 1e-8 with the library's host product: computed once."""
    out = {}
    for name in SYSTEMS:
        M, Cs = pb.case_of(name)
        A, b = bi.dense(M), bi.rhs(M.n)
        for kind in KINDS:
            got = pb.run(M.spmv, b, None, *preconditioner(kind, Cs), 200, TOL)
            out[name, kind] = got, np.linalg.norm(b - A @ got[6]) / np.linalg.norm(b)
    return out


# ------------------------------------------------------------------------------------------------------------ the identities
@pytest.mark.parametrize("name", ["nonsym(300)", "nonsym_shuffled"])
def test_identity_plans_and_an_m_of_ones_are_plain_bicgstab_bit_for_bit(name):
    M = bi.nonsym(300) if name == "nonsym(300)" else bi.nonsym_shuffled()
    b = bi.rhs(M.n)
    for x0 in (None, start_vector(M.n)):
        for tol in (0.0, 1e-10):
            want = bi.run(M.spmv, b, x0, 40, tol)
            for what, (first, m, second) in (("identity plans", pb.identity_plans(M.n)), ("m of ones", (None, np.ones(M.n), None)),
                                             ("identity plans around an m of ones", pb.identity_plans(M.n)[:1] + (np.ones(M.n),) +
                                              pb.identity_plans(M.n)[2:])):
                got = pb.run(M.spmv, b, x0, first, m, second, 40, tol)
                assert got[:4] == want[:4], what
                for i, field in ((4, "rr_each"), (5, "ss_each"), (6, "x")):
                    assert_bits(got[i], want[i], "%s, %s: %s" % (name, what, field))
            assert want[0] > 2


def test_apply_takes_every_part_on_its_own():
    Cs = trsv.of_matrix("nonsym(300)", bi.nonsym(300))
    y = bi.rhs(300, 3)
    first, m, second = pb.sgs(Cs)
    w = trsv.solve(Cs, pb.LOWER, pb.STORED, y)
    assert_bits(pb.apply(first, None, None, y), w, "first alone")
    assert_bits(pb.apply(None, m, None, y), m * y, "m alone")
    assert_bits(pb.apply(None, None, second, y), trsv.solve(Cs, pb.UPPER, pb.STORED, y), "second alone")
    assert_bits(pb.apply(first, m, None, y), m * w, "first and m")
    assert_bits(pb.apply(first, m, second, y), trsv.solve(Cs, pb.UPPER, pb.STORED, m * w), "all three")
    assert_bits(pb.apply(None, None, None, y), y, "none")
    out = pb.apply(None, None, None, y)
    out[0] = 7.0                                                                     # an array of its own
    assert y[0] != 7.0


# ------------------------------------------------------------------------------------------------------------ the exact cases
def test_the_matrix_itself_as_the_preconditioner_stops_in_the_first_half_step_with_the_exact_x():
    """A lower triangular with integer entries, first = LOWER / STORED on A: M = A, phat = A^-1 b exactly, v = r_0, sigma = rho_0,
    alpha = 1, s = 0: rule H at step 1 with half = 1."""
    A, b, x_want = pb.lower_integer()
    plan = (trsv.of_matrix("lower_integer", A), pb.LOWER, pb.STORED)
    steps, full, half, reason, rr, ss, x = pb.run(A.spmv, b, None, plan, None, None, 10, 1e-10)
    assert (steps, full, half, reason) == (1, 0, 1, pb.CONVERGED)
    assert_bits(rr, [bi.dot(b, b)], "rr_each")
    assert_bits(ss, [0.0], "ss_each")
    assert_bits(x, x_want, "x = A^-1 b exactly")
    assert bi.run(A.spmv, b, None, 10, 1e-10)[0] > 1                                  # (plain BiCGSTAB needs more than that)


def test_the_stop_cases_give_their_tuples():
    """K13's rule_t() and rule_b() under identity plans and an m of ones; a zero stored diagonal in either triangle and a NaN in m end
    the run with NONFINITE by rule A at step 1 and x stays x_0."""
    for name, M, b, (first, m, second), tol, expect, x_want in pb.stop_cases():
        got = pb.run(M.spmv, b, None, first, m, second, 10, tol)
        assert got[:4] == expect, "%s: %r" % (name, got[:4])
        if x_want is not None:
            assert_bits(got[6], x_want, name + ": x")
        if expect[1] == 0 and expect[2] == 0:
            assert len(got[4]) == 1
        if expect == (1, 0, 0, pb.NONFINITE) or expect == (1, 0, 0, pb.BREAKDOWN):
            assert len(got[5]) == 0, name + ": rule A leaves no ss"
    assert_bits(pb.run(bi.rule_t()[0].spmv, bi.rule_t()[1], None, *pb.identity_plans(3), 10, 1e-10)[5], [2.0], "rule T: ss_each")
    assert_bits(pb.run(bi.rule_b()[0].spmv, bi.rule_b()[1], None, *pb.identity_plans(3), 10, 1e-10)[4], [2.0, 1.0], "rule B: rr_each")


def test_rule_a_leaves_the_callers_start_vector():
    A = bi.nonsym(300)
    Cs = trsv.of_matrix("nonsym(300)", A)
    x0 = start_vector(300)
    for first, m, second in ((None, pb.nan_m(300), None), ((pb.tri.zero_diagonal(A, 17), pb.LOWER, pb.STORED), None, pb.sgs(Cs)[2])):
        got = pb.run(A.spmv, bi.rhs(300), x0, first, m, second, 10, 1e-10)
        assert got[:4] == (1, 0, 0, pb.NONFINITE)
        assert_bits(got[6], x0, "x stays x_0")


# --------------------------------------------------------------------------------------------------- the run on general matrices
def test_convdiff_is_what_its_docstring_says():
    M = pb.convdiff(32, 0.5)
    A = bi.dense(M)
    assert M.n == 1024 and M.nnz == 5 * 1024 - 4 * 32 and not np.array_equal(A, A.T)
    assert (np.diag(A) == 4.0).all() and A[33, 32] == -1.5 == A[33, 1] and A[33, 34] == -0.5 == A[33, 65]
    row_ptr, col_ind, _ = M.csr
    assert all((np.diff(col_ind[a:z]) > 0).all() for a, z in zip(row_ptr[:-1], row_ptr[1:]))
    pb.ilu.diag_positions(pb.case_of("convdiff(32, 0.5)")[1])                        # sorted rows, a diagonal each: asserted inside


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_preconditioner_converges_and_the_true_residual_is_within_ten_tol(solved, name, kind):
    """With right preconditioning r is the residual of the original system, so the stop rule is plain BiCGSTAB's; the recurrence's
    residual and the true one differ by rounding (measured here: between 3.1e-12 and 8.2e-9 relative at tol = 1e-8), hence the 10."""
    (steps, full, half, reason, rr, ss, x), ratio = solved[name, kind]
    print("%s, %s: steps %d, full %d, half %d, |b - A x| / |b| = %.3g" % (name, kind, steps, full, half, ratio))
    assert reason == pb.CONVERGED and steps < 200
    assert len(rr) == full + 1 and len(ss) == steps and full == steps - half
    b = bi.rhs(len(x))
    thr = (np.float64(TOL) * np.float64(TOL)) * bi.dot(b, b)
    assert (ss[-1] if half else rr[-1]) <= thr and (rr[:-1] > thr).all() and (ss[:-1] > thr).all()
    assert ratio <= 10 * TOL


def test_ilu0_and_sgs_take_at_most_half_of_plain_bicgstabs_steps_on_convdiff(solved):
    """What the triangles are for, as a condition.  With the library's host product (the oracle's CSR loop) the restatement takes, on
    convdiff(32, 0.5) at tol = 1e-8 and bicgstab_method.rhs: plain 60 steps, Jacobi 60 (the diagonal is constant: m scales p and s
    by a power of two), SGS 15, ILU(0) 11.  On nonsym(1003), coalesced: plain 11, Jacobi 5, SGS 2, ILU(0) 2."""
    steps = {kind: solved["convdiff(32, 0.5)", kind][0][0] for kind in KINDS}
    print("convdiff(32, 0.5):", steps, " nonsym(1003), coalesced:", {kind: solved["nonsym(1003), coalesced", kind][0][0] for kind in KINDS})
    assert 2 * steps["ilu0"] <= steps["plain"] and 2 * steps["sgs"] <= steps["plain"]
    assert steps["jacobi"] == steps["plain"]                                         # m = 1/4 everywhere: exact scalings, the same run
    other = {kind: solved["nonsym(1003), coalesced", kind][0][0] for kind in KINDS}
    assert other["ilu0"] <= other["sgs"] <= other["jacobi"] < other["plain"]


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_pbicgstab_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert len(getattr(sm.lib(), name).argtypes) == 12, name
    assert callable(sm.CsrMatrix.pbicgstab) and callable(sm.TjdsMatrix.pbicgstab)


def call(fn, h, o, b, result, first=None, m=None, second=None):
    r = sm.BicgstabResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, first, m, second, C.byref(r) if result else None,
                               None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """K13's argument checks and "no preconditioner at all" come before the handle is looked at and before any HIP call: a block of
    zeros stands in for a handle, another for d_m."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    m = C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.bicgstab_opts(5)
    assert call(fn, None, ok, b, True, m=m) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, True, m=m) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, False, m=m) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, True, m=m) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.bicgstab_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, True, m=m)
        assert rc == sm.ERR_INVALID and (b"smvp_bicgstab_opts_t" in msg if field == "struct_size" else b"tol" in msg), (field, value, msg)
    rc, msg = call(fn, h, ok, b, True)                                               # first, d_m and second all NULL
    assert rc == sm.ERR_INVALID and b"all NULL" in msg and b"smvp_csr_bicgstab" in msg


def test_the_python_call_refuses_cpu_tensors_and_what_is_no_plan():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm._pbicgstab("smvp_csr_pbicgstab", None, v, v, None, None, v, None, 5, 1e-10, 1, None)
    with pytest.raises(ValueError):
        sm._pbicgstab("smvp_csr_pbicgstab", None, v, v, "a plan", None, None, None, 5, 1e-10, 1, None)
