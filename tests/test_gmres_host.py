"""Host checks of tests/gmres_method.py, the numpy restatement of right-preconditioned restarted GMRES as include/smvp_amd.h defines
it (K19): hand-computed runs, the estimate against the true residual, the estimate's monotonic fall inside a cycle, the basis'
orthogonality, the preconditioner identities bit for bit and the step counts test_gpu_gmres.py compares with -- so that the GPU
test compares the library with a reference that is what it claims.  And what of the C ABI needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_method as bi
import gmres_method as gm
import pbicgstab_method as pb
import power_iteration as pi
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_gmres", "smvp_tjds_gmres")
TOL = 1e-8
U = 2.0 ** -53                                               # the unit roundoff of a double
RESTARTS = (1, 2, 5, 30)
# the restatement's step counts on convdiff(32, 0.5) with the host product, restart 30, tol 1e-8, bicgstab_method.rhs
STEPS_ON_CONVDIFF = {"plain": 170, "jacobi": 170, "sgs": 22, "ilu0": 18}
PLAIN = (None, None, None)


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, n)


def system(name):
    if name == "convdiff(32, 0.5)":
        return pb.case_of(name)[0]
    return bi.nonsym(1003) if name == "nonsym(1003)" else bi.banded(3000)


SYSTEMS = ("nonsym(1003)", "banded(3000)", "convdiff(32, 0.5)")


@pytest.fixture(scope="module")
def solved():
    """{(system, restart): (run_rr's tuple, the bases of its cycles)} at tol = 1e-8 with the host product: computed once."""
    out = {}
    for name in SYSTEMS:
        M = system(name)
        for restart in RESTARTS:
            trace = []
            out[name, restart] = gm.run_rr(M.spmv, bi.rhs(M.n), None, *PLAIN, restart, 400, TOL, trace), trace
    return out


# ------------------------------------------------------------------------------------------------------- the hand-computed runs
def test_the_identity_takes_one_step_and_gives_b_exactly():
    """b = (2, -2, 2, 2): tr = 16, beta = 4, v_1 = b / 4, h_1 = 1, w = 0 after the first pass, h_2 = 0: d = 1, c = 1, s = 0,
    rr_1 = +0.0 (a happy breakdown: CONVERGED even at tol = 0), y_1 = 4, x = 4 v_1 = b."""
    b = np.array([2.0, -2.0, 2.0, 2.0])
    for tol in (0.0, 1e-10):
        steps, cycles, columns, reason, rr, tr, x = gm.run(bi.identity(4).spmv, b, None, *PLAIN, 30, 10, tol)
        assert (steps, cycles, columns, reason) == (1, 1, 1, gm.CONVERGED)
        assert_bits(rr, [16.0, 0.0], "rr_each")
        assert_bits(tr, [16.0], "restart_each")
        assert_bits(x, b, "x = b exactly")


def test_the_zero_matrix_breaks_down_at_step_one_and_leaves_x():
    Z = pi.Matrix(3, [0], [0], [0.0])
    b, x0 = np.array([1.0, 2.0, 3.0]), np.array([0.5, -0.25, 4.0])
    for start in (None, x0):
        steps, cycles, columns, reason, rr, tr, x = gm.run(Z.spmv, b, start, *PLAIN, 5, 10, 1e-10)
        assert (steps, cycles, columns, reason) == (1, 1, 0, gm.BREAKDOWN)
        assert_bits(rr, [14.0], "rr_each: rule S1 leaves no rr_1")
        assert_bits(x, np.zeros(3) if start is None else x0, "x untouched")


def test_a_two_by_two_case_by_hand():
    """A = [[0, -1], [1, 0]], b = (1, 0).  Step 1: v_1 = (1, 0), w = (0, 1), h_1 = 0, h_2 = 1, d = 1, c_1 = 0, s_1 = 1, g_2 = -1,
    rr_1 = 1, g_1 = 0: stopped there by max_steps = 1, y_1 = 0 and x = 0.  Step 2: v_2 = (0, 1), w = (-1, 0), h = (-1, 0), h_3 = 0;
    the rotation gives h_1 = 0, h_2 = 1; d = 1, c_2 = 1, s_2 = 0, g_3 = +0.0, rr_2 = +0.0; y_2 = -1, y_1 = 0, x = (0, -1)."""
    A, b = bi.dense3([[0, -1], [1, 0]]), np.array([1.0, 0.0])
    steps, cycles, columns, reason, rr, tr, x = gm.run(A.spmv, b, None, *PLAIN, 2, 1, 1e-10)
    assert (steps, cycles, columns, reason) == (1, 1, 1, gm.MAX_STEPS)
    assert_bits(rr, [1.0, 1.0], "rr_each after one step")
    assert_bits(x, [0.0, 0.0], "x after one step")
    steps, cycles, columns, reason, rr, tr, x = gm.run(A.spmv, b, None, *PLAIN, 2, 10, 1e-10)
    assert (steps, cycles, columns, reason) == (2, 1, 2, gm.CONVERGED)
    assert_bits(rr, [1.0, 1.0, 0.0], "rr_each")
    assert_bits(tr, [1.0], "restart_each")
    assert_bits(x, [0.0, -1.0], "x")
    # restart 1 never gets anywhere on a rotation: every cycle's one column has h_1 = 0
    steps, cycles, columns, reason, rr, tr, x = gm.run(A.spmv, b, None, *PLAIN, 1, 3, 1e-10)
    assert (steps, cycles, columns, reason) == (3, 3, 1, gm.MAX_STEPS)
    assert_bits(rr, [1.0] * 4, "rr_each with restart 1")
    assert_bits(tr, [1.0] * 3, "restart_each with restart 1")


def test_max_steps_in_mid_cycle_and_the_start_rules():
    M = bi.nonsym(300)
    b = bi.rhs(300)
    steps, cycles, columns, reason, rr, tr, x = gm.run(M.spmv, b, None, *PLAIN, 5, 7, 1e-300)
    assert (steps, cycles, columns, reason) == (7, 2, 2, gm.MAX_STEPS) and len(rr) == 8 and len(tr) == 2
    steps, cycles, columns, reason, rr, tr, x = gm.run(M.spmv, b, None, *PLAIN, 5, 10, 1e-300)   # at a cycle's end: no third cycle
    assert (steps, cycles, columns, reason) == (10, 2, 5, gm.MAX_STEPS) and len(tr) == 2
    assert gm.run(M.spmv, np.zeros(300), None, *PLAIN, 5, 7, 0.0)[:4] == (0, 1, 0, gm.CONVERGED)
    inf = b.copy()
    inf[17] = np.inf
    assert gm.run(M.spmv, inf, None, *PLAIN, 5, 7, 1e-10)[:4] == (0, 1, 0, gm.NONFINITE)
    assert gm.run(M.spmv, np.full(300, 1e200), None, *PLAIN, 5, 7, 1e-10)[:4] == (0, 1, 0, gm.NONFINITE)


def test_a_nan_value_ends_the_run_with_nonfinite():
    b = bi.rhs(300)
    steps, cycles, columns, reason, rr, tr, x = gm.run(bi.nan_value().spmv, b, None, *PLAIN, 5, 7, 1e-10)
    assert (steps, cycles, columns, reason) == (1, 1, 0, gm.NONFINITE) and len(rr) == 1
    assert_bits(x, np.zeros(300), "x stays")


# ----------------------------------------------------------------------------------------------------------------- the numerics
@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("restart", RESTARTS)
def test_the_run_converges_and_the_estimate_is_the_true_residual_within_its_rounding_bound(solved, name, restart):
    """|sqrt(rr) - |b - A x|| against a first-order bound.  The estimate is anchored at the true residual tr_c of the last cycle's
    start, so only that cycle's `columns` steps count.  A step's product errs by at most p u |A| |z| (p: the longest row), its two
    Gram-Schmidt updates by 2 columns u per element, the scaling by u: (p + 2 columns + 3) u per step and one step more for b - A x
    itself, on vectors no longer than |b| + |A|_F |x|.  The estimate also takes the basis for orthonormal; its Gram matrix is off
    by at most n u per entry (the dot's worst case), which moves |V g| by (columns + 1) n u |g|."""
    (steps, cycles, columns, reason, rr, tr, x, last), _ = solved[name, restart]
    M = system(name)
    A, b = bi.dense(M), bi.rhs(M.n)
    assert reason == gm.CONVERGED and steps < 400
    assert len(rr) == steps + 1 and len(tr) == cycles == -(-steps // restart) and columns == steps - (cycles - 1) * restart
    thr = (np.float64(TOL) * np.float64(TOL)) * bi.dot(b, b)
    assert last == rr[-1] <= thr and (rr[:-1] > thr).all() and (tr > thr).all()
    true, est = np.linalg.norm(b - A @ x), np.sqrt(last)
    p = int(np.diff(M.csr[0]).max())
    bound = (columns + 1) * (p + 2 * columns + 3) * U * (np.linalg.norm(b) + np.linalg.norm(A) * np.linalg.norm(x)) \
        + (columns + 1) * M.n * U * est
    print("%s, restart %d: steps %d, cycles %d, |b - A x| = %.17g, sqrt(rr) = %.17g, apart %.3g, bound %.3g" % (
        name, restart, steps, cycles, true, est, abs(true - est), bound))
    assert abs(true - est) <= bound
    # every restart's true residual against the estimate the cycle before ended with, by the same bound for `restart` columns
    for c in range(1, cycles):
        full = (restart + 1) * (p + 2 * restart + 3) * U * (np.linalg.norm(b) + np.linalg.norm(A) * np.linalg.norm(x)) \
            + (restart + 1) * M.n * U * np.sqrt(tr[c])
        assert abs(np.sqrt(tr[c]) - np.sqrt(rr[c * restart])) <= full


@pytest.mark.parametrize("name", SYSTEMS)
@pytest.mark.parametrize("restart", RESTARTS)
def test_the_estimate_never_rises_inside_a_cycle_and_the_basis_stays_orthonormal(solved, name, restart):
    """s_j = h_{j+1} / sqrt(h_j^2 + h_{j+1}^2) is at most 1 in rounded arithmetic too (the root of a rounded square is the number
    itself), so |g_{j+1}| <= |g_j|; a cycle's first estimate is held against beta * beta, which may be an ulp above tr_c."""
    (steps, cycles, columns, reason, rr, tr, x, last), trace = solved[name, restart]
    for k in range(1, steps + 1):
        c, j = divmod(k - 1, restart)
        before = np.sqrt(tr[c]) * np.sqrt(tr[c]) if j == 0 else rr[k - 1]
        assert rr[k] <= before, "step %d" % k
    assert len(trace) == cycles
    worst = max(np.abs(V @ V.T - np.eye(len(V))).max() for V in trace)
    print("%s, restart %d: max |V^T V - I| = %.1f ulp" % (name, restart, worst / 2.0 ** -52))
    assert worst <= 300 * 2.0 ** -52


def test_a_restart_of_at_least_n_converges_in_at_most_n_steps():
    rng = np.random.default_rng(19)
    for n in (1, 2, 6, 11):
        a = rng.uniform(-1.0, 1.0, (n, n)) + 3.0 * np.eye(n)
        A, b = bi.dense3(a), bi.rhs(n, 3)
        assert abs(np.linalg.det(a)) > 1e-3
        for restart in (n, n + 3, 64):
            steps, cycles, columns, reason, rr, tr, x = gm.run(A.spmv, b, None, *PLAIN, restart, 100, 1e-10)
            assert reason == gm.CONVERGED and steps <= n and cycles == 1 and columns == steps, (n, restart, steps)
            assert np.linalg.norm(b - a @ x) <= 1e-9 * np.linalg.norm(b)


def test_x0_is_where_the_run_starts():
    M = bi.nonsym(300)
    b, x0 = bi.rhs(300), start_vector(300)
    steps, cycles, columns, reason, rr, tr, x = gm.run(M.spmv, b, x0, *PLAIN, 5, 60, 1e-10)
    assert reason == gm.CONVERGED
    r0 = b - M.spmv(x0)
    assert_bits(tr[:1], [bi.dot(r0, r0)], "tr_0 = dot(b - A x_0)")
    assert np.linalg.norm(b - bi.dense(M) @ x) <= 1e-9 * np.linalg.norm(b)
    exact = np.linalg.solve(bi.dense(M), b)                                           # started at the solution: the start rule
    assert gm.run(M.spmv, b, exact, *PLAIN, 5, 60, 1e-10)[:4] == (0, 1, 0, gm.CONVERGED)


# -------------------------------------------------------------------------------------------------- the preconditioner identities
@pytest.mark.parametrize("name", ["nonsym(300)", "nonsym_shuffled"])
def test_identity_plans_and_an_m_of_ones_are_the_plain_run_bit_for_bit(name):
    M = bi.nonsym(300) if name == "nonsym(300)" else bi.nonsym_shuffled()
    b = bi.rhs(M.n)
    for x0 in (None, start_vector(M.n)):
        for restart, tol in ((4, 0.0), (30, 1e-10)):
            want = gm.run(M.spmv, b, x0, *PLAIN, restart, 25, tol)
            for what, (first, m, second) in (("identity plans", pb.identity_plans(M.n)), ("m of ones", (None, np.ones(M.n), None))):
                got = gm.run(M.spmv, b, x0, first, m, second, restart, 25, tol)
                assert got[:4] == want[:4], what
                for i, field in ((4, "rr_each"), (5, "restart_each"), (6, "x")):
                    assert_bits(got[i], want[i], "%s, %s: %s" % (name, what, field))
            assert want[0] > 2


def test_the_step_counts_on_convdiff_are_the_pinned_ones():
    """What the preconditioners are for, and what test_gpu_gmres.py holds the device to where the product's bits are the host
    loop's.  Jacobi changes nothing here: the diagonal is 4 everywhere, so m scales by a power of two."""
    M, Cs = pb.case_of("convdiff(32, 0.5)")
    b = bi.rhs(M.n)
    A = bi.dense(M)
    got = {}
    for kind in STEPS_ON_CONVDIFF:
        P = PLAIN if kind == "plain" else getattr(pb, kind)(Cs)
        steps, cycles, columns, reason, rr, tr, x = gm.run(M.spmv, b, None, *P, 30, 400, TOL)
        assert reason == gm.CONVERGED and np.linalg.norm(b - A @ x) <= 10 * TOL * np.linalg.norm(b), kind
        got[kind] = steps
    print("convdiff(32, 0.5), restart 30:", got)
    assert got == STEPS_ON_CONVDIFF
    assert 4 * got["ilu0"] <= got["plain"] and 4 * got["sgs"] <= got["plain"]


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_gmres_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS + ("smvp_gmres_opts_default",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    for name in FUNCTIONS:
        assert len(getattr(sm.lib(), name).argtypes) == 12, name
    assert callable(sm.CsrMatrix.gmres) and callable(sm.TjdsMatrix.gmres)
    o = sm.gmres_opts()
    assert (o.struct_size, o.max_steps, o.check_every, o.restart, o.tol) == (C.sizeof(sm.GmresOpts), 100, 10, 30, 1e-10)
    assert (sm.GMRES_CONVERGED, sm.GMRES_MAX_STEPS, sm.GMRES_BREAKDOWN, sm.GMRES_NONFINITE) == (
        gm.CONVERGED, gm.MAX_STEPS, gm.BREAKDOWN, gm.NONFINITE)
    counted = os.path.join(os.path.dirname(sm.LIB_PATH), "libsmvp_amd_counted.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", counted], text=True)
    for name in FUNCTIONS:
        assert re.search(r" T %s$" % name, out, flags=re.M), "%s in the counted build" % name


def call(fn, h, o, b, result):
    r = sm.GmresResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, None, None, None,
                               C.byref(r) if result else None, None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """The argument checks come before the handle is looked at and before any HIP call: a block of zeros stands in for a handle."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.gmres_opts(5)
    assert call(fn, None, ok, b, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf")), ("restart", 0), ("restart", 65), ("restart", -1)):
        o = sm.gmres_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, True)
        want = b"smvp_gmres_opts_t" if field == "struct_size" else b"restart" if field == "restart" else b"tol"
        assert rc == sm.ERR_INVALID and want in msg, (field, value, msg)


def test_the_python_call_refuses_cpu_tensors_and_what_is_no_plan():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm._gmres("smvp_csr_gmres", None, v, v, None, None, None, None, 30, 5, 1e-10, 1, None)
    with pytest.raises(ValueError):
        sm._gmres("smvp_csr_gmres", None, v, v, "a plan", None, None, None, 30, 5, 1e-10, 1, None)
