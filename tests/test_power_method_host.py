"""Host checks of tests/power_method.py, the numpy restatement of the scaled power method (include/smvp_amd.h): its iterates are the
oracle's iterate + normalize bits, it gives the known answers, the tie and stop rules are what the header says -- so that
test_gpu_power_method.py compares the library with a reference that is what it claims.  And what of the C ABI needs no device: the
symbols, the defaults, a NULL handle refused before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import power_iteration as pi
import power_method as pm
import smvp_toolkit_amd as sm
from transposed import assert_bits

ORDINARY = {"short": pi.short, "long": pi.long, "shuffled": pi.shuffled}
NAN = np.nan


def swap():
    return pi.Matrix(2, [0, 1], [1, 0], [1.0, 1.0])


# ------------------------------------------------------------------------------------------------- absmax and the tie rule
def test_absmax_by_cases():
    assert pm.absmax([1.0, -4.0, 2.0]) == (4.0, 1)
    assert pm.absmax([NAN, 3.0, -1.5]) == (3.0, 1)
    assert pm.absmax([NAN, NAN]) == (0.0, -1)
    assert pm.absmax([]) == (0.0, -1)
    assert pm.absmax([0.0, -0.0, 0.0]) == (0.0, 0)
    assert pm.absmax([NAN, -0.0]) == (0.0, 1)
    assert pm.absmax([1.0, np.inf, -np.inf]) == (np.inf, 1)
    assert pm.absmax([5e-324, -10e-324]) == (10e-324, 1)


def test_equal_magnitudes_of_both_signs_go_to_the_smallest_index():
    v = np.full(1003, 0.5)
    v[[1000, 261, 69, 5]] = (2.0, -2.0, 2.0, -2.0)
    assert pm.absmax(v) == (2.0, 5)
    v[5] = NAN
    assert pm.absmax(v) == (2.0, 69)
    for sign in (-1.0, 1.0):
        M, x0 = pm.tie_case(sign)
        steps, reason, index, lam, res, scale, x = pm.run(M.spmv, x0, 4)
        assert (steps, reason, index, scale) == (4, pm.MAX_STEPS, 5, 2.0)
        assert (lam == 2.0 * sign).all(), "lambda is read at index 5 and carries that entry's sign"
        assert (np.abs(x[list(pm.TIE_AT)]) == 1.0).all() and res[-1] == 4.0


# --------------------------------------------------------------------------------- the iterates are the oracle's iterate + normalize
@pytest.mark.parametrize("name", sorted(ORDINARY))
def test_iterates_are_the_oracle_iteration_with_normalize(name):
    M = ORDINARY[name]()
    for x0 in (pi.ones(M), pi.random_x(M)):
        for k in pi.STEPS:
            steps, reason, index, lam, res, scale, x = pm.run(M.spmv, x0, k)
            assert steps == k and reason == pm.MAX_STEPS and len(lam) == len(res) == k
            assert_bits(x, M.iterate(x0, k, normalize=True), "%s, %d steps" % (name, k))


# ------------------------------------------------------------------------------------------------------------- known answers
@pytest.mark.parametrize("p", pi.PEAK_SMALL[1])
@pytest.mark.parametrize("sign", [1, -1])
def test_peak_gives_plus_or_minus_three_exactly(p, sign):
    """Row p holds (p, p) = +-3 alone and x_k[p] = +-1 is the largest magnitude: lambda is exact from step 1, only the residual
    converges, at a ratio of 0.5 a step at the worst."""
    M = pi.peak(pi.PEAK_SMALL[0], p, sign)
    at = {}
    for tol in (1e-3, 1e-9, 1e-14):
        steps, reason, index, lam, res, scale, x = pm.run(M.spmv, pi.ones(M), 25, tol)
        assert reason == pm.CONVERGED and (lam[1:] == 3.0 * sign).all() and index == p and scale == 3.0
        assert res[-1] <= tol * 3.0 and (steps == 1 or res[-2] > tol * 3.0)
        at[tol] = steps
    assert at[1e-3] <= 6 and at[1e-9] <= 13 and at[1e-14] <= 19, at


def test_sym_converges_gradually_to_the_largest_eigenvalue():
    M, A = pm.sym(dense=True)
    assert M.n == 1003 and np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    top = w[np.abs(w).argmax()]
    assert top > 5.0 and np.sort(np.abs(w))[-2] < 0.4 * top                          # real, simple, well ahead of the rest
    steps, reason, index, lam, res, scale, x = pm.run(M.spmv, pi.ones(M), pm.SYM_STEPS, 1e-9)
    assert reason == pm.CONVERGED and 5 < steps < 25
    assert abs(lam[-1] - top) <= 1e-9 * abs(top)
    err = np.abs(lam - top)
    assert (np.diff(err) < 0).all() and err[1] > 1e-3 and err[4] > 1e-6 * top, "lambda itself converges gradually: %r" % err


def test_the_swap_matrix():
    M = swap()
    steps, reason, index, lam, res, scale, x = pm.run(M.spmv, [1.0, -1.0], 10)
    assert (steps, reason, index, lam[0], res[0], scale) == (1, pm.CONVERGED, 0, -1.0, 0.0, 1.0)
    assert_bits(x, [-1.0, 1.0], "the swap matrix from (1, -1)")
    steps, reason, index, lam, res, scale, x = pm.run(M.spmv, [1.0, 0.5], 10, 1e-3)
    assert (steps, reason) == (10, pm.MAX_STEPS) and (lam == 0.5).all() and (res == 0.75).all()     # (0.5, 1) and (1, 0.5) in turn


def test_vanished_and_nonfinite_iterates():
    M = pi.square_zero()
    steps, reason, index, lam, res, scale, x = pm.run(M.spmv, pi.ones(M), 10)
    assert (steps, reason, scale) == (2, pm.ZERO, 0.0) and lam[1] == 0.0 and (x.view(np.int64) == 0).all()
    S = pi.short()
    steps, reason, index, lam, res, scale, x = pm.run(S.spmv, np.zeros(S.n), 10)
    assert (steps, reason, index) == (1, pm.NONFINITE, 0) and np.isnan(lam[0]) and res[0] == 0.0
    steps, reason, index, lam, res, scale, x = pm.run(S.spmv, np.full(S.n, NAN), 10)
    assert (steps, reason, index, scale) == (1, pm.NONFINITE, -1, 0.0) and np.isnan(lam[0]) and res[0] == 0.0
    assert (np.isnan(x) == (S.terms > 0)).all(), "the product of an all-NaN operand: NaN wherever a row has entries, left as it is"


def test_check_every_changes_only_where_the_run_stops():
    M = pi.peak(pi.PEAK_SMALL[0], 63, -1)
    base = pm.run(M.spmv, pi.ones(M), 25, 1e-9, 1)
    for every in (2, 4, 7, 100):
        steps, reason, index, lam, res, scale, x = pm.run(M.spmv, pi.ones(M), 25, 1e-9, every)
        want = min(-(-base[0] // every) * every, 25)
        assert steps == want and reason == pm.CONVERGED
        assert_bits(lam[:base[0]], base[3], "check_every %d: lambda history" % every)
        assert_bits(res[:base[0]], base[4], "check_every %d: residual history" % every)
        assert_bits(x, M.iterate(pi.ones(M), steps, normalize=True), "check_every %d: the iterate" % every)
    Z = pi.square_zero()                                                           # a vanished iterate at an unlooked step carries on
    steps, reason, index, lam, res, scale, x = pm.run(Z.spmv, pi.ones(Z), 10, 0.0, 3)
    assert (steps, reason) == (3, pm.NONFINITE) and index == 0 and np.isnan(lam[2])


# ------------------------------------------------------------------------------------------------ the C ABI without a device
def test_the_library_has_the_symbols_and_the_defaults():
    L = sm.lib()
    for name in ("smvp_power_opts_default", "smvp_csr_power_method", "smvp_tjds_power_method"):
        assert name in sm.EXPORTS and getattr(L, name)
    o = sm.PowerOpts()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    L.smvp_power_opts_default(C.byref(o))
    assert o.struct_size == C.sizeof(sm.PowerOpts) == 24 and o.check_every == 1 and o.tol == 0.0 and o.max_steps >= 1
    assert C.sizeof(sm.PowerResult) == 40
    assert (sm.POWER_CONVERGED, sm.POWER_MAX_STEPS, sm.POWER_ZERO, sm.POWER_NONFINITE) == (pm.CONVERGED, pm.MAX_STEPS, pm.ZERO, pm.NONFINITE)
    assert C.sizeof(sm.RunOpts) == 64, "smvp_run_opts_t's mirror has not moved"


@pytest.mark.parametrize("fn", ["smvp_csr_power_method", "smvp_tjds_power_method"])
def test_a_null_handle_is_refused_before_any_device_call(fn):
    o = sm.power_opts(5)
    r = sm.PowerResult()
    C.memset(C.byref(r), 0x5a, C.sizeof(r))
    before = bytes(r)
    assert getattr(sm.lib(), fn)(None, C.byref(o), None, None, C.byref(r), None, None, None) == sm.ERR_INVALID
    assert bytes(r) == before and b"null handle" in sm.lib().smvp_last_error()
