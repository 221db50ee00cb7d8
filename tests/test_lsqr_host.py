"""Host checks of tests/lsqr_method.py, the numpy restatement of LSQR as include/smvp_amd.h defines it (K22): hand-computed runs,
the run against numpy.linalg.lstsq on dense copies, what the firing rule claims held in true quantities, and the step counts
test_gpu_lsqr.py compares with -- so that the GPU test compares the library with a reference that is what it claims.  And what of
the C ABI needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lsqr_method as lm
import smvp_toolkit_amd as sm
from transposed import assert_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_lsqr", "smvp_tjds_lsqr")
TOL = ATOL = 1e-10
U = 2.0 ** -53
# the restatement's step counts on lsqr_method.NAMED with the host products, tol = atol = 1e-10, from x0 = None
STEPS_ON_NAMED = {"tall(257, 131), inconsistent": 19, "tall(257, 131), consistent": 21, "wide(131, 257)": 21, "nonsym(257)": 40}
REASON_ON_NAMED = {"tall(257, 131), inconsistent": lm.LEAST_SQUARES, "tall(257, 131), consistent": lm.CONVERGED,
                   "wide(131, 257)": lm.CONVERGED, "nonsym(257)": lm.CONVERGED}


def run(A, b, x0=None, max_steps=100, tol=TOL, atol=ATOL):
    return lm.run(A.spmv, A.spmv_t, b, x0, max_steps, tol, atol)


@pytest.fixture(scope="module")
def solved():
    """{name: the run's tuple} on the named constructions: computed once."""
    return {name: run(*lm.named(name), max_steps=400) for name in lm.NAMED}


# ------------------------------------------------------------------------------------------------------- the hand-computed runs
def test_one_by_one_by_hand():
    """A = (2), b = (6).  bnorm = beta_1 = 6, p = 12, vh_1 = 2, alpha_1 = 2, phibar = 6, rhobar = 2, A2 = 4, arnorm_0 = 12,
    w_1 = 1.  Step 1: q = 4, uh_2 = 4 / 2 - 2 * (6 / 6) = 0, beta_2 = 0: vh_2 is not formed, alpha_2 = 0; rho = 2, c = 1, s = 0,
    phi = 6, tx = 3, x = 3; rnorm_1 = arnorm_1 = 0, anorm_1 = 2: CONVERGED, at tol = 0 too."""
    A = lm.dense_rect([[2.0]])
    for tol in (0.0, 1e-10):
        steps, updates, reason, rn, arn, x, res = run(A, np.array([6.0]), tol=tol, atol=0.0)
        assert (steps, updates, reason) == (1, 1, lm.CONVERGED)
        assert_bits(rn, [6.0, 0.0], "rnorm_each")
        assert_bits(arn, [12.0, 0.0], "arnorm_each")
        assert_bits(x, [3.0], "x")
        assert_bits(res, [0.0, 0.0, 2.0, 6.0], "rnorm, arnorm, anorm, bnorm")
    # max_steps = 1 changes nothing: CONVERGED comes before MAX_STEPS
    assert run(A, np.array([6.0]), max_steps=1)[:3] == (1, 1, lm.CONVERGED)


def test_a_two_by_two_diagonal_matrix_ends_by_a_zero_beta_with_the_exact_x():
    """A = diag(2, 2), b = (3, 4).  beta_1 = 5, p = (6, 8), vh_1 = (1.2, 1.6), alpha_1 = sqrt(1.44 + 2.56) = 2, w_1 = (0.6, 0.8).
    Step 1: q = (2.4, 3.2), uh_2 = q / 2 - 2 * (b / 5) = (1.2 - 1.2, 1.6 - 1.6) = 0 (a power of two scales exactly): beta_2 = 0,
    alpha_2 = +0.0, rho = 2, c = 1, s = 0, tx = 5 / 2, x = 2.5 * (0.6, 0.8) = (1.5, 2) = A^-1 b exactly, rnorm_1 = 0."""
    A = lm.dense_rect([[2.0, 0.0], [0.0, 2.0]])
    steps, updates, reason, rn, arn, x, res = run(A, np.array([3.0, 4.0]), tol=0.0, atol=0.0)
    assert (steps, updates, reason) == (1, 1, lm.CONVERGED)
    assert_bits(rn, [5.0, 0.0], "rnorm_each")
    assert_bits(arn, [10.0, 0.0], "arnorm_each")
    assert_bits(x, [1.5, 2.0], "x")
    assert_bits(res, [0.0, 0.0, 2.0, 5.0], "rnorm, arnorm, anorm, bnorm")
    # two distinct singular values take two steps; the second ends the Krylov space up to rounding
    B = lm.dense_rect([[1.0, 0.0], [0.0, 3.0]])
    steps, updates, reason, rn, arn, x, res = run(B, np.array([1.0, 1.0]), tol=1e-14, atol=0.0)
    assert (steps, updates, reason) == (2, 2, lm.CONVERGED)
    assert np.abs(x - [1.0, 1.0 / 3.0]).max() <= 8 * U


def test_b_orthogonal_to_the_range_ends_at_step_zero_as_least_squares():
    """A = (1; 0), b = (0, 5): p = A^T b = 0, vh_1 = 0, alpha_1 = 0: x_0 already is the least-squares solution.  The same from
    x_0 = (7) with b = (7, 5): uh_1 = (0, 5)."""
    A = lm.dense_rect([[1.0], [0.0]])
    for b, x0, want in ((np.array([0.0, 5.0]), None, 0.0), (np.array([7.0, 5.0]), np.array([7.0]), 7.0)):
        steps, updates, reason, rn, arn, x, res = run(A, b, x0, atol=0.0)
        assert (steps, updates, reason) == (0, 0, lm.LEAST_SQUARES)
        assert_bits(rn, [5.0], "rnorm_each")
        assert_bits(arn, [0.0], "arnorm_each")
        assert_bits(x, [want], "x = x0")
        assert_bits(res[:3], [5.0, 0.0, 0.0], "rnorm, arnorm, anorm")


def test_a_zero_b_converges_at_step_zero_with_x_zero():
    A = lm.tall(9, 4)
    steps, updates, reason, rn, arn, x, res = run(A, np.zeros(9), tol=0.0, atol=0.0)
    assert (steps, updates, reason) == (0, 0, lm.CONVERGED)
    assert_bits(rn, [0.0], "rnorm_each")
    assert_bits(arn, [0.0], "arnorm_each")
    assert_bits(x, np.zeros(4), "x")
    assert_bits(res, np.zeros(4), "every norm +0.0")


def test_a_zero_alpha_in_mid_run_ends_as_least_squares_with_the_update_done():
    """A = (1 0; 0 0; 0 0) stored as one entry, b = (3, 4, 0): beta_1 = 5, p = (3, 0), vh_1 = (0.6, 0), alpha_1 = 0.6, w_1 = (1, 0).
    Step 1: q = (0.6, 0, 0), uh_2 = (1 - 0.6 * 0.6, -0.6 * 0.8, 0) is not zero, p = A^T uh_2 is parallel to vh_1 and vh_2
    vanishes up to rounding: the step's x is (3, 0) up to rounding and the reason LEAST_SQUARES, whatever atol."""
    A = lm.Rect(3, 2, [0], [0], [1.0])
    steps, updates, reason, rn, arn, x, res = run(A, np.array([3.0, 4.0, 0.0]), tol=0.0, atol=1e-12)
    assert (steps, updates, reason) == (1, 1, lm.LEAST_SQUARES)
    assert abs(x[0] - 3.0) <= 8 * U * 3.0 and x[1] == 0.0
    assert abs(res[0] - 4.0) <= 8 * U * 4.0


def test_nonfinite_operands_end_the_run_and_leave_x():
    A = lm.tall(40, 17)
    b = lm.rhs(40)
    for bad in (np.nan, np.inf):
        c = b.copy()
        c[11] = bad
        steps, updates, reason, rn, arn, x, res = run(A, c)
        assert (steps, updates, reason) == (0, 0, lm.NONFINITE) and len(rn) == 1
        assert_bits(x, np.zeros(17), "x stays")
    assert run(A, np.full(40, 1e200))[:3] == (0, 0, lm.NONFINITE)                      # the square overflows
    # a NaN value in the matrix shows in p = A^T b already: step 0
    rows, cols, vals = (np.array(A.coo[f]) for f in ("row", "col", "val"))
    nan = vals.copy()
    nan[3] = np.nan
    assert run(lm.Rect(40, 17, rows, cols, nan), b)[:3] == (0, 0, lm.NONFINITE)
    # values of 5e153: A2 gains about 2 |A|^2 a step and overflows in the third -- rule N leaves x_2 and three history elements
    steps, updates, reason, rn, arn, x, res = run(lm.Rect(40, 17, rows, cols, vals * 5e153), b)
    assert (steps, updates, reason) == (3, 2, lm.NONFINITE) and len(rn) == len(arn) == 3
    assert np.isfinite(x).all() and np.isfinite(res).all()
    assert_bits(res[:2], [rn[-1], arn[-1]], "the result holds step 2's estimates")


def test_max_steps_and_the_histories_lengths():
    A, b = lm.named("tall(257, 131), inconsistent")
    steps, updates, reason, rn, arn, x, res = run(A, b, max_steps=5, tol=0.0, atol=0.0)
    assert (steps, updates, reason) == (5, 5, lm.MAX_STEPS) and len(rn) == len(arn) == 6
    assert_bits(res[:2], [rn[-1], arn[-1]], "the result holds the last history elements")
    assert run(A, b, max_steps=1, tol=0.0, atol=0.0)[:3] == (1, 1, lm.MAX_STEPS)
    # the residual estimate never rises: s <= 1 in rounded arithmetic too
    assert (np.diff(rn) <= 0).all()


# ----------------------------------------------------------------------------------------------- against an independent reference
@pytest.mark.parametrize("name", ["tall(257, 131)", "wide(131, 257)", "tall(1003, 517)"])
def test_the_well_conditioned_constructions_are_well_conditioned(name):
    A = {"tall(257, 131)": lm.tall(257, 131), "wide(131, 257)": lm.wide(131, 257), "tall(1003, 517)": lm.tall(1003, 517)}[name]
    cond = np.linalg.cond(A.dense())
    print("%s: cond %.3f" % (name, cond))
    assert cond <= 100
    assert np.linalg.matrix_rank(lm.rank_deficient(257, 131).dense()) == 130


@pytest.mark.parametrize("name", lm.NAMED)
def test_the_run_reaches_lstsq_and_the_firing_rule_holds_in_true_quantities(solved, name):
    """After CONVERGED |b - A x| <= 2 tol |b|; after LEAST_SQUARES |A^T (b - A x)| <= 2 atol |A|_F |b - A x|.  The factor 2 is the
    margin for the recurrences phibar and alpha |c| drifting from the true norms.  Largest ratios observed against tol |b| and
    atol |A|_F |r| (so: against 1, the bound being 2): 0.36 (tall, consistent), 0.57 (wide), 0.54 (nonsym), 0.32 (tall,
    inconsistent).  Then x against numpy.linalg.lstsq on the dense copy (for the wide matrix: the minimum-norm solution, which
    x_0 = 0 selects): |x - x*| <= |r - r*| / sigma_min for a consistent system, <= |A^T r| / sigma_min^2 for the normal
    equations, plus the rounding of `steps` updates for the part of x that A does not see."""
    A, b = lm.named(name)
    steps, updates, reason, rn, arn, x, res = solved[name]
    D = A.dense()
    assert reason == REASON_ON_NAMED[name] and steps == updates < 400
    r = b - D @ x
    true_r, true_ar, fro = np.linalg.norm(r), np.linalg.norm(D.T @ r), np.linalg.norm(D)
    sigma_min = np.linalg.svd(D, compute_uv=False).min()
    best = np.linalg.lstsq(D, b, rcond=None)[0]
    apart = np.linalg.norm(x - best)
    if reason == lm.CONVERGED:
        ratio = true_r / (TOL * np.linalg.norm(b))
        bound = 2 * TOL * np.linalg.norm(b) / sigma_min
    else:
        ratio = true_ar / (ATOL * fro * true_r)
        bound = 2 * ATOL * fro * true_r / sigma_min ** 2
    bound += 100 * steps * U * np.linalg.norm(best)
    print("%s: steps %d, reason %d, |r| = %.17g (estimate %.17g), |A^T r| = %.3g (estimate %.3g), ratio %.3f, |x - lstsq| = %.3g, "
          "bound %.3g" % (name, steps, reason, true_r, res[0], true_ar, res[1], ratio, apart, bound))
    assert ratio <= 2.0
    assert apart <= bound
    assert abs(res[3] - np.linalg.norm(b)) <= 4 * U * A.m * res[3]
    assert res[2] <= 1.01 * np.sqrt(steps + 1) * fro                                   # the Frobenius estimate grows with the steps


def test_the_step_counts_on_the_named_constructions_are_the_pinned_ones(solved):
    got = {name: solved[name][0] for name in lm.NAMED}
    print(got)
    assert got == STEPS_ON_NAMED


def test_the_rank_deficient_matrix_reaches_a_least_squares_solution():
    """A repeated column: lstsq's minimum-norm solution is what x_0 = 0 gives, because every iterate lies in range(A^T)."""
    A = lm.rank_deficient(257, 131)
    b = lm.rhs(257)
    D = A.dense()
    steps, updates, reason, rn, arn, x, res = run(A, b, max_steps=400)
    assert reason == lm.LEAST_SQUARES
    best = np.linalg.lstsq(D, b, rcond=None)[0]
    r = b - D @ x
    assert np.linalg.norm(D.T @ r) <= 2 * ATOL * np.linalg.norm(D) * np.linalg.norm(r)
    assert np.linalg.norm(x - best) <= 1e-7 * np.linalg.norm(best) and abs(x[0] - x[130]) <= 1e-9


def test_x0_is_where_the_run_starts():
    A, b = lm.named("tall(257, 131), consistent")
    x0 = lm.rhs(131, 9)
    steps, updates, reason, rn, arn, x, res = run(A, b, x0)
    assert reason == lm.CONVERGED
    uh = b - A.spmv(x0)
    assert_bits(rn[:1], [np.sqrt(lm.dot(uh, uh))], "rnorm_0 = |b - A x_0|")
    assert np.linalg.norm(b - A.dense() @ x) <= 2 * TOL * np.linalg.norm(b)
    assert run(A, b, lm.rhs(131, 5), tol=1e-12)[:3] == (0, 0, lm.CONVERGED)           # started at the solution


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_lsqr_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS + ("smvp_lsqr_opts_default",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
    assert len(sm.lib().smvp_csr_lsqr.argtypes) == 10 and len(sm.lib().smvp_tjds_lsqr.argtypes) == 9
    assert callable(sm.CsrMatrix.lsqr) and callable(sm.TjdsMatrix.lsqr)
    o = sm.lsqr_opts()
    assert (o.struct_size, o.max_steps, o.check_every, o.tol, o.atol) == (C.sizeof(sm.LsqrOpts), 100, 10, 1e-10, 1e-10)
    assert C.sizeof(sm.LsqrOpts) == 32 and C.sizeof(sm.LsqrResult) == 48
    assert (sm.LSQR_CONVERGED, sm.LSQR_LEAST_SQUARES, sm.LSQR_MAX_STEPS, sm.LSQR_NONFINITE) == (
        lm.CONVERGED, lm.LEAST_SQUARES, lm.MAX_STEPS, lm.NONFINITE)
    for word in ("SMVP_LSQR_CONVERGED = 0", "SMVP_LSQR_LEAST_SQUARES = 1", "SMVP_LSQR_MAX_STEPS = 2", "SMVP_LSQR_NONFINITE = 3"):
        assert word in header
    counted = os.path.join(os.path.dirname(sm.LIB_PATH), "libsmvp_amd_counted.so")
    out = subprocess.check_output(["nm", "-D", "--defined-only", counted], text=True)
    for name in FUNCTIONS:
        assert re.search(r" T %s$" % name, out, flags=re.M), "%s in the counted build" % name


def call(fn, h, ht, o, b, result):
    r = sm.LsqrResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    handles = (h, ht) if fn == "smvp_csr_lsqr" else (h,)
    rc = getattr(sm.lib(), fn)(*handles, C.byref(o) if o is not None else None, b, None, None, C.byref(r) if result else None,
                               None, None, None)
    assert bytes(r) == before, "*result was written although the call was refused"
    return rc, sm.lib().smvp_last_error()


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_bad_arguments_are_refused_before_any_device_call(fn):
    """The argument checks come before the handles are looked at and before any HIP call: blocks of zeros stand in for handles."""
    fake, fake_t = C.create_string_buffer(4096), C.create_string_buffer(4096)
    h, ht, b = C.cast(fake, C.c_void_p), C.cast(fake_t, C.c_void_p), C.cast(C.create_string_buffer(64), C.c_void_p)
    ok = sm.lsqr_opts(5)
    assert call(fn, None, ht, ok, b, True) == (sm.ERR_INVALID, b"%s: null handle" % fn.encode())
    if fn == "smvp_csr_lsqr":
        rc, msg = call(fn, h, None, ok, b, True)
        assert rc == sm.ERR_INVALID and msg.startswith(b"smvp_csr_lsqr: null ht")
    assert call(fn, h, ht, None, b, True) == (sm.ERR_INVALID, b"%s: null opts" % fn.encode())
    assert call(fn, h, ht, ok, b, False) == (sm.ERR_INVALID, b"%s: null result" % fn.encode())
    assert call(fn, h, ht, ok, None, True) == (sm.ERR_INVALID, b"%s: null d_b" % fn.encode())
    for field, value in (("struct_size", 24), ("struct_size", 0), ("max_steps", 0), ("check_every", 0), ("tol", -1e-300),
                         ("tol", float("nan")), ("tol", float("inf")), ("atol", -1e-300), ("atol", float("nan")),
                         ("atol", float("inf"))):
        o = sm.lsqr_opts(5)
        setattr(o, field, value)
        rc, msg = call(fn, h, ht, o, b, True)
        want = b"smvp_lsqr_opts_t" if field == "struct_size" else b"atol"
        assert rc == sm.ERR_INVALID and want in msg, (field, value, msg)


def test_the_python_call_refuses_cpu_tensors_and_what_is_no_matrix():
    import torch
    v = torch.ones(4, dtype=torch.float64)
    with pytest.raises(ValueError):
        sm._lsqr("smvp_csr_lsqr", (None, None), v, v, None, 5, 1e-10, 1e-10, 1, None)
    A = sm.CsrMatrix.__new__(sm.CsrMatrix)
    A._h = None
    with pytest.raises(ValueError):
        A.lsqr(v, v, at="a matrix")
    A._borrowed = True
