"""Host checks of tests/pcg_method.py, the numpy restatement of the diagonal of a handle and of conjugate gradients with a diagonal
preconditioner (include/smvp_amd.h, K14): with m = ones the run is cg_method.run bit for bit, a hand-computed case, what Jacobi buys
on badly scaled systems, every stop rule -- so that test_gpu_pcg.py compares the library with a reference that is what it claims.
And what of the C ABI needs no device: the symbols, the result block, the arguments refused before any HIP call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cg_method as cg
import pcg_method as pcg
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_diagonal", "smvp_tjds_diagonal", "smvp_csr_pcg", "smvp_tjds_pcg")


# --------------------------------------------------------------------------------------------------------------- the diagonal
def test_the_diagonal_of_every_case_is_the_dense_diagonal_where_nothing_repeats():
    for M in pcg.diag_cases():
        d = pcg.diagonal(M)                                                          # (asserts that the CSR and the TJDS walk agree)
        assert d.shape == (M.rows,) and not np.signbit(d[d == 0.0]).any(), M.name
        r, c, v = (np.array(M.coo[f]) for f in ("row", "col", "val"))
        on = r == c
        counts = np.bincount(r[on], minlength=M.rows)
        once = np.zeros(M.rows)
        once[r[on]] = v[on]
        single = counts == 1
        assert_bits(d[single] + 0.0, once[single] + 0.0, M.name + ": rows that store their diagonal once")     # (+ 0.0: -0.0 reads +0.0)
        assert_bits(d[counts == 0], np.zeros((counts == 0).sum()), M.name + ": rows without a diagonal")


def test_the_cases_are_what_their_names_say():
    by_name = {M.name.split(",")[0].split(":")[0]: M for M in pcg.diag_cases()}
    Z = by_name["signed zeros on the diagonal"]
    assert_bits(pcg.diagonal(Z)[[3, 7, 11, 15]], [0.0, 0.0, 0.0, 2.5], "stored zeros of either sign")
    R = by_name["three repeats of mixed sign"]
    d = pcg.diagonal(R)
    assert_bits(d[[5, 64, 199]], [0.0, 0.0, 0.0], "(1e16 + 1.0) - 1e16 in storage order")
    assert (1e16 - 1e16) + 1.0 == 1.0                                                # what another order gives
    N = by_name["NaN and Inf on and off the diagonal"]
    d = pcg.diagonal(N)
    assert np.isnan(d[2]) and d[9] == np.inf and d[30] == -np.inf and np.isnan(d[41])
    assert_bits(d[[4, 17, 33, 50]], [1.5, -2.5, 3.5, 0.0], "the off-diagonal NaN and Inf do not leak")
    assert np.isfinite(np.delete(d, [2, 9, 30, 41])).all()
    for M in pcg.diag_cases():
        if not M.name.startswith("the diagonal first"):
            continue
        row_ptr, col_ind, val = M.csr
        seen = set()
        for a, L in enumerate(pcg.LENGTHS):
            for b, at in enumerate((0, L // 2, L - 1)):
                i = 3 + 9 * a + 3 * b
                assert row_ptr[i + 1] - row_ptr[i] == L and col_ind[row_ptr[i] + at] == i, (M.name, L, at)
                assert (col_ind[row_ptr[i]:row_ptr[i + 1]] == i).sum() == 1
                seen.add(i)
        d = pcg.diagonal(M)
        assert (d[sorted(seen)] != 0.0).all() and (np.delete(d, sorted(seen)) == 0.0).all()
    wide, tall = by_name["200 x 300"], by_name["300 x 200"]
    assert pcg.diagonal(wide).shape == (200,) and pcg.diagonal(tall).shape == (300,)
    assert_bits(pcg.diagonal(tall)[200:], np.zeros(100), "rows beyond the last column")
    assert (pcg.diagonal(tall)[:200] != 0.0).any()


def test_a_row_blocks_diagonal_lies_at_first_row_plus_r():
    M = cg.spd(1003)
    row_ptr, col_ind, val = M.csr
    lo, hi = 100, 400
    block = row_ptr[lo:hi + 1] - row_ptr[lo]
    d = pcg.diagonal_csr(hi - lo, M.n, block, col_ind[row_ptr[lo]:row_ptr[hi]], val[row_ptr[lo]:row_ptr[hi]], first_row=lo)
    assert_bits(d, pcg.diagonal(M)[lo:hi], "rows 100 .. 399 of spd(1003)")
    assert (d > 0.5).all()


# ------------------------------------------------------------------------------------- m = ones is conjugate gradients, bit for bit
@pytest.mark.parametrize("name", ["spd", "spd_long", "spd_shuffled"])
def test_an_all_ones_preconditioner_is_plain_cg_bit_for_bit(name):
    M = cg.spd(300) if name == "spd" else getattr(cg, name)()
    b = cg.rhs(M.n)
    for x0 in (None, np.random.default_rng(9).uniform(-2.0, 2.0, M.n)):
        for tol, steps in ((1e-10, 40), (0.0, 12)):
            want = cg.run(M.spmv, b, x0, steps, tol)
            got = pcg.run(M.spmv, b, x0, np.ones(M.n), steps, tol)
            assert got[:3] == want[:3]
            assert_bits(got[3], want[3], "rr_each")
            assert_bits(got[4], want[3], "rz_each is rr_each: z is r")
            assert_bits(got[5], want[4], "sigma_each")
            assert_bits(got[6], want[5], "x")


def test_a_hand_computed_two_by_two_case():
    """A = [[4, 1], [1, 3]], m = (4, 2), b = (1, 2), every number a small dyadic rational until alpha_1: r_0 = (1, 2), z_0 = (1/4, 1),
    rr_0 = 5, rho_0 = 9/4, q_1 = A z_0 = (2, 13/4), sigma_1 = 1/2 + 13/4 = 15/4, alpha_1 = (9/4) / (15/4) = fl(0.6)."""
    M = pcg.pi.Matrix(2, [0, 0, 1, 1], [0, 1, 0, 1], [4.0, 1.0, 1.0, 3.0])
    b, m = np.array([1.0, 2.0]), np.array([4.0, 2.0])
    steps, updates, reason, rr, rz, sigma, x = pcg.run(M.spmv, b, None, m, 1, 0.0)
    assert (steps, updates, reason) == (1, 1, pcg.MAX_STEPS)
    assert rr[0] == 5.0 and rz[0] == 2.25 and sigma[0] == 3.75
    alpha = np.float64(2.25) / np.float64(3.75)
    assert_bits(x, [alpha * 0.25, alpha * 1.0], "x_1 = alpha_1 z_0")
    r1 = np.array([1.0 - alpha * 2.0, 2.0 - alpha * 3.25])
    assert_bits([rr[1]], [r1[0] * r1[0] + r1[1] * r1[1]], "rr_1")
    assert_bits([rz[1]], [r1[0] * (r1[0] / 4.0) + r1[1] * (r1[1] / 2.0)], "rho_1 = r_1 . (r_1 ./ m)")
    full = pcg.run(M.spmv, b, None, m, 10, 1e-12)                                   # two steps solve a 2 x 2 system
    assert full[2] == pcg.CONVERGED and full[0] == 2
    assert np.allclose(full[6], np.linalg.solve(cg.dense(M), b), rtol=1e-14, atol=0.0)


# --------------------------------------------------------------------------------------------------- what the diagonal buys
@pytest.mark.parametrize("name,n", [("spd", 1003), ("spd", 300), ("spd_long", None)])
def test_jacobi_converges_where_plain_cg_runs_out_of_steps(name, n):
    M = pcg.scaled(cg.spd(n) if n else cg.spd_long(), 2)
    A, b = cg.dense(M), cg.rhs(M.n)
    m = pcg.diagonal(M)
    assert (m > 0.0).all()
    steps, updates, reason, rr, rz, sigma, x = pcg.run(M.spmv, b, None, m, 60, 1e-8)
    plain = cg.run(M.spmv, b, None, 60, 1e-8)
    print("%s(%s) scaled by 10^U[-2, 2]: Jacobi PCG %d steps, reason %d; plain CG reason %d, rr %g of thr %g" % (
        name, n, steps, reason, plain[2], plain[3][-1], 1e-16 * cg.dot(b, b)))
    assert reason == pcg.CONVERGED and steps == updates <= 30
    assert plain[:3] == (60, 60, cg.MAX_STEPS)
    assert cg.run(M.spmv, b, None, 400, 1e-8)[:3] == (400, 400, cg.MAX_STEPS)      # still unconverged at 400
    # the file's only tolerance: 10 x the stop rule, for the gap between the recursive and the true residual
    assert np.linalg.norm(b - A @ x) <= 1e-7 * np.linalg.norm(b)


# ------------------------------------------------------------------------------------------------------------- the stop rules
def test_a_zero_in_m_where_r0_is_not_zero_is_nonfinite_at_step_zero():
    M = cg.spd(300)
    m = np.ones(300)
    m[17] = 0.0
    steps, updates, reason, rr, rz, sigma, x = pcg.run(M.spmv, cg.rhs(300), None, m, 10, 1e-10)
    assert (steps, updates, reason) == (0, 0, pcg.NONFINITE) and np.isinf(rz[0]) and np.isfinite(rr[0]) and len(sigma) == 0
    assert_bits(x, np.zeros(300), "x stays zero")


def test_a_negative_m_breaks_down_at_step_zero():
    M = cg.spd(300)
    steps, updates, reason, rr, rz, sigma, x = pcg.run(M.spmv, cg.rhs(300), None, -np.ones(300), 10, 1e-10)
    assert (steps, updates, reason) == (0, 0, pcg.BREAKDOWN) and rz[0] == -rr[0] < 0.0 and len(sigma) == 0
    assert_bits(x, np.zeros(300), "x stays zero")


def test_rule_a_breaks_down_on_a_matrix_that_is_not_positive_definite():
    b = cg.rhs(300, 5)
    steps, updates, reason, rr, rz, sigma, x = pcg.run(cg.minus_identity(300).spmv, b, None, np.ones(300), 10, 1e-10)
    assert (steps, updates, reason) == (1, 0, pcg.BREAKDOWN) and sigma[0] < 0.0 and len(rr) == len(rz) == 1
    assert_bits(x, np.zeros(300), "x is unchanged")


def test_rule_b_breaks_down_when_rho_turns_negative():
    """A = I (2 x 2), m = (1, -1), b = (2, 1): z_0 = (2, -1), rho_0 = 3, sigma_1 = 5, alpha_1 = 0.6, r_1 ~ (0.8, 1.6), rr_1 ~ 3.2 and
    rho_1 ~ 0.64 - 2.56 < 0: rule B, and the update is kept."""
    steps, updates, reason, rr, rz, sigma, x = pcg.run(cg.identity(2).spmv, np.array([2.0, 1.0]), None, np.array([1.0, -1.0]), 10, 1e-10)
    assert (steps, updates, reason) == (1, 1, pcg.BREAKDOWN)
    assert rz[0] == 3.0 and sigma[0] == 5.0 and rz[1] < -1.9 and rr[1] > 3.1 and len(rr) == len(rz) == 2
    alpha = np.float64(3.0) / np.float64(5.0)
    assert_bits(x, [alpha * 2.0, alpha * -1.0], "x_1")


def test_the_remaining_rules():
    M = cg.spd(300)
    m = pcg.diagonal(M)
    b = cg.rhs(300)
    steps, updates, reason, rr, rz, sigma, x = pcg.run(M.spmv, b, None, m, 5, 1e-300)
    assert (steps, updates, reason) == (5, 5, pcg.MAX_STEPS) and len(rr) == len(rz) == 6 and len(sigma) == 5
    full = pcg.run(M.spmv, b, None, m, 40, 1e-300)
    assert_bits(rr, full[3][:6], "the first steps of a longer run")
    got = pcg.run(M.spmv, np.zeros(300), None, m, 10, 1e-10)
    assert got[:3] == (0, 0, pcg.CONVERGED) and got[3][0] == 0.0 and got[4][0] == 0.0
    got = pcg.run(M.spmv, np.zeros(300), None, m, 10, 0.0)
    assert got[:3] == (0, 0, pcg.CONVERGED)
    N = cg.nan_value()
    steps, updates, reason, rr, rz, sigma, x = pcg.run(N.spmv, cg.rhs(N.n), None, np.ones(N.n), 10, 1e-10)
    assert (steps, updates, reason) == (1, 0, pcg.NONFINITE) and np.isnan(sigma[0]) and len(rr) == 1
    assert_bits(x, np.zeros(N.n), "x is unchanged")
    inf = cg.rhs(300)
    inf[17] = np.inf
    assert pcg.run(M.spmv, inf, None, m, 10, 1e-10)[:3] == (0, 0, pcg.NONFINITE)
    one = pcg.run(cg.identity(300).spmv, cg.rhs(300, 5), None, np.full(300, 0.5), 10, 0.0)
    assert one[:3] == (1, 1, pcg.CONVERGED) and one[3][1] == 0.0                     # z = 2 r, alpha = 1/2: x_1 = b exactly
    assert_bits(one[6], cg.rhs(300, 5), "identity: x is b")


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_pcg_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    assert re.search(r"\}\s*smvp_pcg_result_t\s*;", header)
    assert C.sizeof(sm.PcgResult) == 40 and sm.PcgResult.rr.offset == 16 and sm.PcgResult.rz.offset == 24 and sm.PcgResult.bb.offset == 32


def call(fn, h, o, b, m, result):
    r = sm.PcgResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    rc = getattr(sm.lib(), fn)(h, C.byref(o) if o is not None else None, b, None, None, m, C.byref(r) if result else None, None, None,
                               None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", ["smvp_csr_pcg", "smvp_tjds_pcg"])
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """K12's checks in K12's order, d_m after d_b: they come before the handle is looked at and before any HIP call, so a block of
    zeros stands in for a handle."""
    fake = C.create_string_buffer(4096)
    h, b = C.cast(fake, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.cg_opts(5)
    assert call(fn, None, ok, b, b, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    assert call(fn, h, None, b, b, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ok, b, b, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ok, None, b, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    assert call(fn, h, ok, b, None, True) == (sm.ERR_INVALID, b"%s: null d_m" % fn.encode())
    assert call(fn, None, None, None, None, False)[1] == b"%s: null handle" % fn.encode()
    for field, value in (("struct_size", 20), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf"))):
        o = sm.cg_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, o, b, b, True)
        assert rc == sm.ERR_INVALID and (b"smvp_cg_opts_t" in msg if field == "struct_size" else b"tol" in msg), (field, value, msg)


@pytest.mark.parametrize("fn", ["smvp_csr_diagonal", "smvp_tjds_diagonal"])
def test_the_diagonal_refuses_a_null_handle_without_a_device(fn):
    out = C.cast(C.create_string_buffer(64), C.c_void_p)
    assert getattr(sm.lib(), fn)(None, out, None) == sm.ERR_INVALID
    assert sm.lib().smvp_last_error() == b"%s: null handle" % fn.encode()


def test_the_python_calls_refuse_cpu_tensors():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm._pcg("smvp_csr_pcg", None, v, v, v, None, 5, 1e-10, 1, None)
    with pytest.raises(ValueError):
        sm._diagonal("smvp_csr_diagonal", None, 4, v, None)
