"""Host checks of tests/bicgstab_method.py, the numpy restatement of BiCGSTAB as include/smvp_amd.h defines it: the exact small
cases give their tuples and their x bit for bit, the run solves three general matrices to the true residual, and the history is the
residual's -- so that test_gpu_bicgstab.py compares the library with a reference that is what it claims.  And what of the C ABI needs
no device: the symbols, the defaults, the arguments refused before any HIP call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bicgstab_method as bi
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_bicgstab_opts_default", "smvp_csr_bicgstab", "smvp_tjds_bicgstab")
TYPES = ("smvp_bicgstab_opts_t", "smvp_bicgstab_result_t")
MAX_STEPS = 40
TOL = 1e-10
# |b - A x| <= C_RESIDUAL * tol * |b| with the dense matrix: a check against a gross error of the method, not a tolerance on bits
# (the recurrence's residual, which the stop rule sees, and the true one differ by rounding).  The next power of ten above the worst
# ratio |b - A x| / (tol |b|) measured on the three matrices below, x0 None / random:
#   nonsym(257) 0.466 / 0.432    nonsym_long() 0.402 / 0.342    nonsym_shuffled() 0.989 / 0.585
C_RESIDUAL = 1.0


def start_vector(n, seed=9):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, n)


# ------------------------------------------------------------------------------------------------------- the exact small cases
def test_identity_and_minus_identity_stop_in_the_half_step_with_x_equal_to_plus_or_minus_b():
    b = bi.rhs(300, 5)
    for M, x_want in ((bi.identity(300), b), (bi.minus_identity(300), -b)):
        for tol in (0.0, 1e-10):
            steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, None, 10, tol)
            assert (steps, full, half, reason) == (1, 0, 1, bi.CONVERGED)
            assert_bits(rr, [bi.dot(b, b)], "rr_each")
            assert_bits(ss, [0.0], "ss_each")
            assert_bits(x, x_want, "x")


def test_swap2_breaks_down_by_rule_a():
    """v = A p = (0, 1), sigma = rhat . v = 0."""
    x0 = np.array([0.25, -3.0])
    M = bi.swap2()
    for start in (None, x0):
        b = np.array([1.0, 0.0]) if start is None else np.array([1.0, 0.0]) + M.spmv(x0)    # r_0 = (1, 0) either way
        steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, start, 10, 1e-10)
        assert (steps, full, half, reason) == (1, 0, 0, bi.BREAKDOWN)
        assert_bits(rr, [1.0], "rr_each")
        assert len(ss) == 0
        assert_bits(x, np.zeros(2) if start is None else x0, "x is unchanged")


def test_rule_t_breaks_down_with_the_half_update():
    """sigma = -1, alpha = -1, s = (0, -1, 1), t = A s = 0, tt = 0: x = alpha p = (-1, 0, 0), every step exact."""
    M, b = bi.rule_t()
    assert np.array_equal(bi.dense(M), [[-1, -1, -1], [-1, -1, -1], [1, -1, -1]])
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, None, 10, 1e-10)
    assert (steps, full, half, reason) == (1, 0, 1, bi.BREAKDOWN)
    assert_bits(rr, [1.0], "rr_each")
    assert_bits(ss, [2.0], "ss_each")
    assert_bits(x, [-1.0, 0.0, 0.0], "x")


def test_rule_b_breaks_down_after_a_full_update():
    """sigma = -4, alpha = -1/2, s = (0, 0, -1), t = (1, 1, 0), ts = 0, tt = 2, omega = 0: x_1 = (-1/2, -1/2, 0), r_1 = s, rr_1 = 1,
    rho_1 = rhat . r_1 = 0; rr_1 is above thr and 1 is not max_steps, so omega == 0 is the first of rule B that holds."""
    M, b = bi.rule_b()
    assert np.array_equal(bi.dense(M), [[-1, -1, -1], [-1, -1, -1], [-1, -1, 0]])
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, None, 10, 1e-10)
    assert (steps, full, half, reason) == (1, 1, 0, bi.BREAKDOWN)
    assert_bits(rr, [2.0, 1.0], "rr_each")
    assert_bits(ss, [1.0], "ss_each")
    assert_bits(x, [-0.5, -0.5, 0.0], "x")
    assert bi.run(M.spmv, b, None, 1, 1e-10)[:4] == (1, 1, 0, bi.MAX_STEPS)              # max_steps comes before the breakdown


def test_a_nan_matrix_value_stops_by_rule_a_at_step_one():
    M = bi.nan_value()
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, bi.rhs(M.n), None, 10, 1e-10)
    assert (steps, full, half, reason) == (1, 0, 0, bi.NONFINITE) and len(rr) == 1 and len(ss) == 0
    assert_bits(x, np.zeros(M.n), "x is unchanged")


def test_nonfinite_right_hand_sides_stop_at_step_zero():
    M = bi.nonsym(300)
    b = bi.rhs(300)
    b[17] = np.inf
    assert bi.run(M.spmv, b, None, 10, 1e-10)[:4] == (0, 0, 0, bi.NONFINITE)
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, np.full(300, 1e200), None, 10, 1e-10)
    assert (steps, full, half, reason) == (0, 0, 0, bi.NONFINITE) and np.isinf(rr[0]) and len(ss) == 0    # bb overflows


def test_a_zero_right_hand_side_converges_at_step_zero():
    for tol in (1e-10, 0.0):
        steps, full, half, reason, rr, ss, x = bi.run(bi.nonsym(300).spmv, np.zeros(300), None, 10, tol)
        assert (steps, full, half, reason) == (0, 0, 0, bi.CONVERGED) and len(rr) == 1 and len(ss) == 0
        assert_bits(x, np.zeros(300), "x stays zero")


def test_max_steps():
    M, b = bi.nonsym(300), bi.rhs(300)
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, None, 10, 1e-300)              # tol * tol underflows: thr = 0
    assert (steps, full, half, reason) == (10, 10, 0, bi.MAX_STEPS) and len(rr) == 11 and len(ss) == 10
    longer = bi.run(M.spmv, b, None, MAX_STEPS, 1e-300)
    assert_bits(rr, longer[4][:11], "the first steps of a longer run")


# ------------------------------------------------------------------------------------------------- the run on general matrices
LARGE = [("nonsym", (257,)), ("nonsym_long", ()), ("nonsym_shuffled", ())]


@pytest.fixture(scope="module", params=LARGE, ids=[name for name, _ in LARGE])
def general(request):
    name, args = request.param
    M = getattr(bi, name)(*args)
    return name, M, bi.dense(M), bi.rhs(M.n)


def test_the_matrices_are_not_symmetric_and_strictly_row_dominant(general):
    name, M, A, b = general
    assert not np.array_equal(A, A.T)
    d = np.abs(np.diag(A))
    assert (d > np.abs(A).sum(axis=1) - d).all()
    assert {"nonsym": 257, "nonsym_long": 700, "nonsym_shuffled": 1003}[name] == M.n
    if name == "nonsym_long":
        assert (np.count_nonzero(A[[5, 350, 699]], axis=1) == 700).all()
    if name == "nonsym_shuffled":
        rows, cols = np.array(M.coo["row"]), np.array(M.coo["col"])
        assert len(rows) - len(set(zip(rows.tolist(), cols.tolist()))) >= 25 and (np.diff(rows) < 0).any()


@pytest.mark.parametrize("start", ["NULL", "random"])
def test_run_converges_and_the_true_residual_is_within_c_tol(general, start):
    name, M, A, b = general
    x0 = None if start == "NULL" else start_vector(M.n)
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, x0, MAX_STEPS, TOL)
    ratio = np.linalg.norm(b - A @ x) / (TOL * np.linalg.norm(b))
    print("%s, x0 %s: steps %d, full %d, half %d, |b - A x| / (tol |b|) = %.3f" % (name, start, steps, full, half, ratio))
    assert reason == bi.CONVERGED and steps < MAX_STEPS
    assert len(rr) == full + 1 and len(ss) == steps and full == steps - half
    thr = (np.float64(TOL) * np.float64(TOL)) * bi.dot(b, b)
    assert (ss[-1] if half else rr[-1]) <= thr and (rr[:-1] > thr).all() and (ss[:-1] > thr).all()
    assert ratio <= C_RESIDUAL
    want = np.linalg.solve(A, b)
    assert np.linalg.norm(x - want) <= 1e-8 * np.linalg.norm(want)


@pytest.mark.parametrize("start", ["NULL", "random"])
def test_the_history_is_the_residuals(general, start):
    """rr_each[k] is dot(r_k, r_k) of the run's own r_k, and r_0 is b - A x_0 (b itself, bit for bit, without an x_0)."""
    name, M, A, b = general
    x0 = None if start == "NULL" else start_vector(M.n)
    trace = []
    steps, full, half, reason, rr, ss, x = bi.run(M.spmv, b, x0, MAX_STEPS, TOL, trace=trace)
    assert len(trace) == full + 1 == len(rr)
    assert_bits(rr, [bi.dot(r, r) for r in trace], "rr_each")
    assert_bits(trace[0], b if x0 is None else b - M.spmv(x0), "r_0")
    for k in (1, full):                                          # the recurrence's residual is the true one up to rounding
        assert np.linalg.norm(trace[k]) < np.linalg.norm(trace[0])


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_bicgstab_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    for name in TYPES:
        assert re.search(r"\}\s*%s\s*;" % name, header), name
    assert (sm.BICGSTAB_CONVERGED, sm.BICGSTAB_MAX_STEPS, sm.BICGSTAB_BREAKDOWN, sm.BICGSTAB_NONFINITE) == (
        bi.CONVERGED, bi.MAX_STEPS, bi.BREAKDOWN, bi.NONFINITE)
    for i, name in enumerate(("CONVERGED", "MAX_STEPS", "BREAKDOWN", "NONFINITE")):
        assert re.search(r"\bSMVP_BICGSTAB_%s\s*=\s*%d\b" % (name, i), header), name


def test_bicgstab_opts_default():
    o = sm.BicgstabOpts()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    sm.lib().smvp_bicgstab_opts_default(C.byref(o))
    assert o.struct_size == C.sizeof(sm.BicgstabOpts) == 24
    assert (o.max_steps, o.check_every, o.tol) == (100, 10, 1e-10)
    assert C.sizeof(sm.BicgstabResult) == 32
    sm.lib().smvp_bicgstab_opts_default(None)
    o = sm.bicgstab_opts(7, tol=1e-3, check_every=2)
    assert (o.struct_size, o.max_steps, o.check_every, o.tol) == (24, 7, 2, 1e-3)


def call(fn, h, o, b, result):
    r = sm.BicgstabResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, C.byref(r) if result else None, None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", ["smvp_csr_bicgstab", "smvp_tjds_bicgstab"])
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """The argument checks come before the handle is looked at and before any HIP call: a block of zeros stands in for a handle."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.bicgstab_opts(5)
    assert call(fn, None, ok, b, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.bicgstab_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, True)
        assert rc == sm.ERR_INVALID and (b"smvp_bicgstab_opts_t" in msg if field == "struct_size" else b"tol" in msg), (field, value, msg)


def test_the_python_call_refuses_cpu_tensors():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm._bicgstab("smvp_csr_bicgstab", None, v, v, None, 5, 1e-10, 1, None)
