"""Host checks of tests/cg_method.py, the numpy restatement of the order-defined dot product and of conjugate gradients
(include/smvp_amd.h): the dot gives hand-computed values where its order shows, the run solves a symmetric positive definite system
and gives the known answers of every stop rule -- so that test_gpu_cg.py compares the library with a reference that is what it
claims.  And what of the C ABI needs no device: the symbols, the defaults, the arguments refused before any HIP call."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cg_method as cg
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_vector_dot", "smvp_cg_opts_default", "smvp_csr_cg", "smvp_tjds_cg")
TYPES = ("smvp_cg_opts_t", "smvp_cg_result_t")
U = 2.0 ** -53                                                  # half an ulp of 1.0: 1.0 + U rounds back to 1.0 (ties to even)


# ------------------------------------------------------------------------------------------------------------------- the dot
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1003])
def test_dot_of_ones_is_n(n):
    got = cg.dot(np.ones(n), np.ones(n))
    assert got == float(n) and not np.signbit(got)


def test_dot_of_negative_zero_terms_is_positive_zero():
    assert_bits([cg.dot(np.full(300, -0.0), np.ones(300))], [0.0], "an accumulator starts at +0.0 and never becomes -0.0")
    assert_bits([cg.dot([], [])], [0.0], "n = 0")


def test_the_order_shows_inside_a_workgroup():
    """n = 256: one 1.0 in lane 0 and 255 halves of an ulp.  A serial sum loses every one of them (1.0 + U = 1.0).  The defined
    order: in wavefront 0 the butterfly adds c_32 = U to 1.0 (lost), then the sums 2U, 4U, 8U, 16U, 32U of the other lanes, which
    are exact: w0 = 1 + 62 U.  Wavefronts 1 to 3 hold 64 U each, exactly.  ((w0 + w1) + w2) + w3 = 1 + 254 U, every step exact."""
    a = np.full(256, U)
    a[0] = 1.0
    serial = 0.0
    for v in a:
        serial += v
    assert serial == 1.0
    assert cg.dot(a, np.ones(256)) == 1.0 + 254 * U
    assert math.fsum(a) == 1.0 + 255 * U and 1.0 + 255 * U == 1.0 + 256 * U    # the exact sum rounds up to even: a third value


def test_the_order_shows_across_trips_and_partials():
    """n = one grid trip + 1: slot 0 holds 1.0 and, one trip later, U -- the same lane adds it to 1.0 and loses it -- and slot 1
    holds U, which the butterfly's last step adds to lane 0's 1.0 and loses too.  Any order that met the two U first keeps them."""
    a = np.zeros(cg.TRIP + 1)
    a[0], a[1], a[cg.TRIP] = 1.0, U, U
    assert cg.dot(a, np.ones(len(a))) == 1.0
    assert math.fsum(a) == 1.0 + 2 * U
    b = np.zeros(257)                                           # two workgroups: the partials 1.0 and U meet in the second level's
    b[0], b[256] = 1.0, 3 * U                                   # lanes 0 and 1 and are added by the butterfly's last step
    assert cg.dot(b, np.ones(257)) == 1.0 + 4 * U               # 1 + 3U lies between 1 + 2U and 1 + 4U: ties to even
    c = np.zeros(65537)                                         # 257 partials: partial 256 is the second trip of lane 0 of the
    c[0], c[65536] = 1.0, U                                     # second level
    assert cg.dot(c, np.ones(65537)) == 1.0


@pytest.mark.parametrize("n", [1, 64, 255, 257, 1003, 65537, cg.TRIP + 1])
def test_dot_is_within_the_bound_of_any_order_of_fsum(n):
    """Any order of n additions of rounded terms is within n * 2^-53 * sum |a_i b_i| of the exact sum (to first order; the terms'
    own rounding is inside it for n >= 2, and for n = 1 the dot is the rounded product itself)."""
    rng = np.random.default_rng(20272 + n)
    a = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
    b = rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.integers(-3, 4, n)
    exact = math.fsum(a * b)
    assert abs(cg.dot(a, b) - exact) <= n * U * math.fsum(np.abs(a * b))


def test_fold256_is_vectorised_over_workgroups():
    c = np.random.default_rng(3).standard_normal((5, 256))
    rows = cg.fold256(c)
    for g in range(5):
        w = []
        for v in c[g].reshape(4, 64):
            v = v.copy()
            for h in (32, 16, 8, 4, 2, 1):
                for j in range(h):
                    v[j] = v[j] + v[j + h]
            w.append(v[0])
        assert rows[g] == ((w[0] + w[1]) + w[2]) + w[3]


# --------------------------------------------------------------------------------------- the run on a positive definite matrix
@pytest.fixture(scope="module")
def spd1003():
    M = cg.spd(1003)
    return M, cg.dense(M), cg.rhs(1003)


def test_spd_is_symmetric_positive_definite(spd1003):
    M, A, b = spd1003
    assert np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    assert 0.5 < w[0] and w[-1] < 2.1
    for f in (cg.spd_long, cg.spd_shuffled):
        L = cg.dense(f())
        assert np.array_equal(L, L.T) and np.linalg.eigvalsh(L)[0] > 0.5, f.__name__


@pytest.mark.parametrize("tol", [1e-6, 1e-10])
def test_run_converges_and_the_true_residual_is_within_twice_tol(spd1003, tol):
    M, A, b = spd1003
    steps, updates, reason, rr, sigma, x = cg.run(M.spmv, b, None, 40, tol)
    assert reason == cg.CONVERGED and steps == updates < 40
    assert len(rr) == updates + 1 and len(sigma) == steps and (sigma > 0).all()
    assert rr[-1] <= (tol * tol) * cg.dot(b, b) < rr[-2]
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) <= 2 * tol
    if tol == 1e-10:
        want = np.linalg.solve(A, b)
        assert np.linalg.norm(x - want) <= 1e-8 * np.linalg.norm(want)


def test_a_start_vector_is_used(spd1003):
    M, A, b = spd1003
    x0 = np.linalg.solve(A, b) + 1e-3
    steps, updates, reason, rr, sigma, x = cg.run(M.spmv, b, x0, 40, 1e-10)
    assert reason == cg.CONVERGED and rr[0] < 1e-2 * cg.dot(b, b)
    assert np.linalg.norm(b - A @ x) / np.linalg.norm(b) <= 2e-10


# ------------------------------------------------------------------------------------------------------------- known answers
def test_identity_converges_at_step_one_with_x_equal_to_b():
    b = cg.rhs(300, 5)
    steps, updates, reason, rr, sigma, x = cg.run(cg.identity(300).spmv, b, None, 10, 0.0)
    assert (steps, updates, reason) == (1, 1, cg.CONVERGED) and rr[1] == 0.0
    assert_bits(x, b, "identity: x is b")


def test_a_zero_right_hand_side_converges_at_step_zero():
    steps, updates, reason, rr, sigma, x = cg.run(cg.spd(300).spmv, np.zeros(300), None, 10, 1e-10)
    assert (steps, updates, reason) == (0, 0, cg.CONVERGED) and len(rr) == 1 and len(sigma) == 0
    assert_bits(x, np.zeros(300), "x stays zero")


@pytest.mark.parametrize("name", ["minus_identity", "swap2"])
def test_a_matrix_that_is_not_positive_definite_breaks_down(name):
    M = cg.minus_identity(2) if name == "minus_identity" else cg.swap2()
    x0 = np.array([0.25, -3.0])
    for start in (None, x0):
        b = np.array([1.0, 0.0]) if start is None else np.array([1.0, 0.0]) + M.spmv(x0)    # r_0 = (1, 0) either way
        steps, updates, reason, rr, sigma, x = cg.run(M.spmv, b, start, 10, 1e-10)
        assert (steps, updates, reason) == (1, 0, cg.BREAKDOWN)
        assert len(rr) == 1 and sigma[0] == (-1.0 if name == "minus_identity" else 0.0)
        assert_bits(x, np.zeros(2) if start is None else x0, "x is unchanged")


def test_nonfinite_right_hand_sides_stop_at_step_zero():
    M = cg.spd(300)
    b = cg.rhs(300)
    b[17] = np.inf
    assert cg.run(M.spmv, b, None, 10, 1e-10)[:3] == (0, 0, cg.NONFINITE)
    steps, updates, reason, rr, sigma, x = cg.run(M.spmv, np.full(300, 1e200), None, 10, 1e-10)
    assert (steps, updates, reason) == (0, 0, cg.NONFINITE) and np.isinf(rr[0])                # bb overflows


def test_a_nan_matrix_value_stops_at_step_one_without_an_update():
    M = cg.nan_value()
    steps, updates, reason, rr, sigma, x = cg.run(M.spmv, cg.rhs(M.n), None, 10, 1e-10)
    assert (steps, updates, reason) == (1, 0, cg.NONFINITE) and np.isnan(sigma[0]) and len(rr) == 1
    assert_bits(x, np.zeros(M.n), "x is unchanged")


def test_max_steps(spd1003):
    M, A, b = spd1003
    steps, updates, reason, rr, sigma, x = cg.run(M.spmv, b, None, 5, 1e-10)
    assert (steps, updates, reason) == (5, 5, cg.MAX_STEPS) and len(rr) == 6 and len(sigma) == 5
    full = cg.run(M.spmv, b, None, 40, 1e-10)
    assert_bits(rr, full[3][:6], "the first steps of a longer run")


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_cg_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    for name in TYPES:
        assert re.search(r"\}\s*%s\s*;" % name, header), name
    assert (sm.CG_CONVERGED, sm.CG_MAX_STEPS, sm.CG_BREAKDOWN, sm.CG_NONFINITE) == (cg.CONVERGED, cg.MAX_STEPS, cg.BREAKDOWN, cg.NONFINITE)
    for i, name in enumerate(("CONVERGED", "MAX_STEPS", "BREAKDOWN", "NONFINITE")):
        assert re.search(r"\bSMVP_CG_%s\s*=\s*%d\b" % (name, i), header), name


def test_cg_opts_default():
    o = sm.CgOpts()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    sm.lib().smvp_cg_opts_default(C.byref(o))
    assert o.struct_size == C.sizeof(sm.CgOpts) == 24
    assert (o.max_steps, o.check_every, o.tol) == (100, 10, 1e-10)
    assert C.sizeof(sm.CgResult) == 32
    sm.lib().smvp_cg_opts_default(None)
    o = sm.cg_opts(7, tol=1e-3, check_every=2)
    assert (o.struct_size, o.max_steps, o.check_every, o.tol) == (24, 7, 2, 1e-3)


def call(fn, h, o, b, result):
    r = sm.CgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, C.byref(r) if result else None, None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", ["smvp_csr_cg", "smvp_tjds_cg"])
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """The argument checks come before the handle is looked at and before any HIP call: a block of zeros stands in for a handle."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.cg_opts(5)
    assert call(fn, None, ok, b, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.cg_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, True)
        assert rc == sm.ERR_INVALID and (b"smvp_cg_opts_t" in msg if field == "struct_size" else b"tol" in msg), (field, value, msg)


def test_vector_dot_refuses_bad_arguments_without_a_device():
    out = C.c_double(-7.0)
    b = C.cast(C.create_string_buffer(64), C.c_void_p)
    L = sm.lib()
    assert L.smvp_vector_dot(0, -1, b, b, C.byref(out), None) == sm.ERR_INVALID
    assert L.smvp_vector_dot(0, 4, None, b, C.byref(out), None) == sm.ERR_INVALID
    assert L.smvp_vector_dot(0, 4, b, None, C.byref(out), None) == sm.ERR_INVALID
    assert L.smvp_vector_dot(0, 4, b, b, None, None) == sm.ERR_INVALID
    assert out.value == -7.0
    assert L.smvp_vector_dot(0, 0, None, None, C.byref(out), None) == sm.OK                    # n = 0: +0.0, no device needed
    assert_bits([out.value], [0.0], "n = 0")


def test_the_python_calls_refuse_cpu_tensors():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm.vector_dot(v, v)
    with pytest.raises(ValueError):
        sm._cg("smvp_csr_cg", None, v, v, None, 5, 1e-10, 1, None)
