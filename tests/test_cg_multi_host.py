"""Host checks of tests/cg_multi_method.py, the restatement of conjugate gradients for k right-hand sides as include/smvp_amd.h
defines them (K20): the block that ends in every stop reason at once, the layout of the two-dimensional histories, the column-wise
definition itself -- so that test_gpu_cg_multi.py compares the library with a reference that is what it claims.  And what of the
C ABI and of the binding needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cg_method as cg
import cg_multi_method as cm
import pcg_method as pcg
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_cg_multi", "smvp_tjds_cg_multi")
SENTINEL = -12345.678


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_the_mixed_block_ends_in_every_reason(fmt):
    M, B = cm.signed_diagonal(), cm.mixed_block()
    product = cm.product_of(M, fmt)
    plain = cm.run(product, B, None, None, cm.MIXED_STEPS, cm.MIXED_TOL)
    assert cm.outcomes(plain) == cm.MIXED_PLAIN
    assert {r[2] for r in plain} == {cm.CONVERGED, cm.MAX_STEPS, cm.BREAKDOWN, cm.NONFINITE}
    m = np.abs(cm.signed_diagonal_values())
    jacobi = cm.run(product, B, None, m, cm.MIXED_STEPS, cm.MIXED_TOL)
    assert cm.outcomes(jacobi) == cm.MIXED_JACOBI
    # the eigenvector column is solved exactly by one step, either way
    for runs in (plain, jacobi):
        x = cm.solution(runs)[:, 1]
        want = np.zeros(M.n)
        want[3] = 1.5 / cm.signed_diagonal_values()[3]
        assert_bits(x, want, "1.5 e_3 / d_3")
    # a column that breaks down at step 1, and the columns stopped at step 0, keep x_0 = zeros; rule A at step 2 keeps x_1
    X = cm.solution(plain)
    assert not X[:, 2].any() and not X[:, 3].any() and not X[:, 5].any() and X[:, 4].any()


def test_a_column_is_the_one_vector_run_whatever_stands_beside_it():
    M = cg.spd(300)
    product = cm.csr_product(M)
    b, x0 = cg.rhs(300), cg.rhs(300, 9)
    m = pcg.diagonal(M)
    bad = np.full(300, np.nan)
    B, X0 = np.stack([bad, b, np.zeros(300)], axis=1), np.stack([x0, x0, bad], axis=1)
    runs = cm.run(product, B, X0, None, 30, 1e-10)
    alone = cg.run(product, b, x0, 30, 1e-10)
    assert runs[1][:3] == alone[:3] and alone[2] == cg.CONVERGED
    for got, want, what in ((runs[1][3], alone[3], "rr_each"), (runs[1][4], alone[3], "rz_each is rr_each without an m"),
                            (runs[1][5], alone[4], "sigma_each"), (runs[1][6], alone[5], "x")):
        assert_bits(got, want, what)
    assert cm.outcomes(runs)[0] == (0, 0, cm.NONFINITE) and cm.outcomes(runs)[2][2] == cm.NONFINITE
    with_m = cm.run(product, B, X0, m, 30, 1e-10)
    want = pcg.run(product, b, x0, m, 30, 1e-10)
    assert with_m[1][:3] == want[:3]
    for i in (3, 4, 5, 6):
        assert_bits(with_m[1][i], want[i], "pcg_method.run's element %d" % i)
    ones = cm.run(product, B, X0, np.ones(300), 30, 1e-10)                     # m all ones: every number is the plain run's
    for i in (3, 4, 5, 6):
        assert_bits(ones[1][i], runs[1][i], "m = ones, element %d" % i)


def test_the_layout_of_the_histories():
    """Column v's rr and rz at [v * (max_steps + 1) + j], j = 0 .. updates_v; its sigma at [v * max_steps + j], j = 0 .. steps_v - 1;
    the fill everywhere else.  Hand-made runs, so that every element says where it belongs."""
    max_steps = 4

    def made(v, steps, updates):
        return (steps, updates, cm.CONVERGED, 100.0 * v + np.arange(updates + 1), 100.0 * v + 50 + np.arange(updates + 1),
                100.0 * v + 80 + np.arange(steps), None)
    runs = [made(0, 4, 4), made(1, 0, 0), made(2, 3, 2)]
    rr, rz, sigma = cm.flat_histories(runs, max_steps, SENTINEL)
    S = SENTINEL
    assert rr.tolist() == [0, 1, 2, 3, 4, 100, S, S, S, S, 200, 201, 202, S, S]
    assert rz.tolist() == [50, 51, 52, 53, 54, 150, S, S, S, S, 250, 251, 252, S, S]
    assert sigma.tolist() == [80, 81, 82, 83, S, S, S, S, 280, 281, 282, S]
    assert rr.reshape(3, max_steps + 1)[2, 1] == 201 and sigma.reshape(3, max_steps)[2, 2] == 282     # the (k, .) view of the binding
    # and on real runs: the mixed block's
    M, B = cm.signed_diagonal(), cm.mixed_block()
    runs = cm.run(cm.csr_product(M), B, None, None, cm.MIXED_STEPS, cm.MIXED_TOL)
    rr, rz, sigma = cm.flat_histories(runs, cm.MIXED_STEPS, S)
    filled_rr = [u + 1 for _, u, _ in cm.MIXED_PLAIN]
    filled_sigma = [s for s, _, _ in cm.MIXED_PLAIN]
    assert [(row != S).sum() for row in rr.reshape(6, cm.MIXED_STEPS + 1)][:5] == filled_rr[:5]       # (column 5's rr_0 is NaN)
    assert [(row != S).sum() for row in sigma.reshape(6, cm.MIXED_STEPS)] == filled_sigma
    assert_bits(rr[4 * (cm.MIXED_STEPS + 1):4 * (cm.MIXED_STEPS + 1) + 2], runs[4][3], "column 4's two values of rr")


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_cg_multi_symbols_are_declared_bound_and_exported():
    """The test that fails without the feature on a machine with no GPU."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert len(getattr(sm.lib(), name).argtypes) == 15, name
    assert callable(sm.CsrMatrix.cg_multi) and callable(sm.TjdsMatrix.cg_multi)
    counted = os.path.join(os.path.dirname(sm.LIB_PATH), "libsmvp_amd_counted.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", counted], text=True)
    for name in FUNCTIONS:
        assert re.search(r" T %s$" % name, out, flags=re.M), "%s in the counted build" % name


def call(fn, h, o, B, results=True, k=2):
    r = (sm.PcgResult * 2)()
    C.memset(r, 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, k, B, 2, None, 0, None, 2, None, r if results else None, None,
                               None, None, None)
    assert bytes(r) == before, "results were written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """The argument checks come before the handle is looked at and before any HIP call: a block of zeros stands in for a handle."""
    fake = C.create_string_buffer(4096)
    h, B = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.cg_opts(5)
    assert call(fn, None, ok, B) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, B) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, B, results=False) == (sm.ERR_INVALID, b"%s: null results" % fn.encode())
    assert call(fn, h, ok, None) == (sm.ERR_INVALID, b"%s: null d_B" % fn.encode())
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.cg_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, B)
        assert rc == sm.ERR_INVALID and (b"smvp_cg_opts_t" if field == "struct_size" else b"tol") in msg, (field, value, msg)


def test_the_binding_takes_the_leading_dimensions_from_the_strides():
    import torch
    wide = torch.zeros(7, 9, dtype=torch.float64)
    B, X, X0 = wide[:, 1:4], torch.zeros(7, 3, dtype=torch.float64), torch.zeros(7, 5, dtype=torch.float64)[:, 2:]
    m = torch.ones(7, dtype=torch.float64)
    assert sm.cg_multi_operands(B, X, X0, m, 7) == (3, 9, 3, 5)
    assert sm.cg_multi_operands(B, X, None, None, 7) == (3, 9, 3, 0)
    for bad in ((B, X[:, :2], None, None), (B.t(), X.t(), None, None), (B, X, X0[:6], None), (B, X, None, m[:6]), (B, X.float(), None, None),
                (B[:, 0], X[:, 0], None, None), (B, X, None, torch.ones(14, dtype=torch.float64)[::2])):
        with pytest.raises(ValueError):
            sm.cg_multi_operands(*bad, 7)
    with pytest.raises(ValueError):                                              # CPU tensors: their addresses mean nothing on the device
        sm._cg_multi("smvp_csr_cg_multi", None, 7, B, X, None, None, 5, 1e-10, 1, None)
