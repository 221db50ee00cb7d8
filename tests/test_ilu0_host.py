"""CPU: the ILU(0) restatement tests/ilu0_method.py and the library's two host calls (smvp_csr_ilu0_check, smvp_csr_ilu0_host,
kernel K17): hand-computed factors, the host loop against the restatement bit for bit on every case the GPU tests use, the check's
refusals, the defining property (L U)_ij = a_ij on the pattern within a derived bound, and what the factor buys conjugate gradients.

The bound.  Every stored element is computed as fl(a_ij - sum of rounded products), below the diagonal followed by one division: by
Higham, Accuracy and Stability of Numerical Algorithms, Lemma 8.4, |a_ij - sum_k l_ik u_kj| <= gamma_m sum_k |l_ik| |u_kj| with m
the number of terms of the sum, the one with l_ii = 1 or with u_jj included.  The tests allow gamma_(m + 1), u = 2^-53, and
evaluate both sides in exact integer arithmetic, so nothing of the check's own rounding enters."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import cg_method as cg
import ilu0_method as im
import pcg_method as pcg
import pcg_tri_method as tri
import smvp_toolkit_amd as sm
import trsv_method as trsv
from transposed import assert_bits

W = 256                                                                              # the chain width the CPU cases are built for
TOL = 1e-8
ALL = list(range(im.N_CONSTRUCTED + im.N_MORE))
UNIT_ROUNDOFF = Fraction(1, 2 ** 53)


def gamma(m):
    return m * UNIT_ROUNDOFF / (1 - m * UNIT_ROUNDOFF)


# ------------------------------------------------------------------------------------------------------------ computed by hand
def test_a_hand_computed_three_by_three_case():
    """A = [[4, 2, 0], [2, 5, 2], [0, 2, 2]], every value dyadic.  Row 0: 4, 2.  Row 1: l_10 = 2/4 = 0.5; u_11 = 5 - 0.5 * 2 = 4;
    u_12 = 2 (row 0 stores no column 2: nothing to subtract).  Row 2: l_21 = 2/4 = 0.5; u_22 = 2 - 0.5 * 2 = 1.  F = [4, 2 | 0.5, 4, 2 | 0.5, 1]."""
    M = trsv.Case("3 x 3", 3, [0, 0, 1, 1, 1, 2, 2], [0, 1, 0, 1, 2, 1, 2], [4.0, 2.0, 2.0, 5.0, 2.0, 2.0, 2.0])
    want = [4.0, 2.0, 0.5, 4.0, 2.0, 0.5, 1.0]
    assert_bits(im.ilu0(M).csr[2], want, "the restatement")
    assert_bits(sm.ilu0_host(3, *M.csr), want, "smvp_csr_ilu0_host")
    assert im.diag_positions(M).tolist() == sm.ilu0_check(3, M.csr[0], M.csr[1]).tolist() == [0, 3, 6]


def test_a_missing_update_is_skipped_not_multiplied():
    """[[0, 1], [1, 1]] stored in full: l_10 = 1/0 = Inf, u_11 = 1 - Inf * 1 = -Inf.  With (0, 1) NOT stored the update does not
    exist: u_11 stays 1, where subtracting Inf * 0 for the missing entry would have made it NaN."""
    full = trsv.Case("2 x 2", 2, [0, 0, 1, 1], [0, 1, 0, 1], [0.0, 1.0, 1.0, 1.0], finite_stored=False)
    assert_bits(im.ilu0(full, finite=False).csr[2], [0.0, 1.0, np.inf, -np.inf], "the restatement")
    assert_bits(sm.ilu0_host(2, *full.csr), [0.0, 1.0, np.inf, -np.inf], "smvp_csr_ilu0_host")
    hole = trsv.Case("2 x 2 without (0, 1)", 2, [0, 1, 1], [0, 0, 1], [0.0, 1.0, 1.0], finite_stored=False)
    assert_bits(im.ilu0(hole, finite=False).csr[2], [0.0, np.inf, 1.0], "the restatement")
    assert_bits(sm.ilu0_host(2, *hole.csr), [0.0, np.inf, 1.0], "smvp_csr_ilu0_host")


def test_the_order_dependent_case_against_its_hand_value():
    M = im.order_dependent()
    F = im.ilu0(M).csr[2]
    assert_bits(F, [1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1e16, 1e16, 1.0, 1.0], "((1 - 1e16) + 1e16) + 1 = 1")
    assert ((1.0 + 1.0) - 1e16) + 1e16 == 2.0 and ((1.0 - 1e16) + 1.0) + 1e16 == 0.0, "another order, another value"
    assert_bits(sm.ilu0_host(4, *M.csr), F, "smvp_csr_ilu0_host")


# ------------------------------------------------------------------------------------------- the host loop is the restatement
@pytest.mark.parametrize("i", ALL)
def test_the_host_loop_is_the_restatement_bit_for_bit(i):
    M = im.case(W, i)
    F = im.factor(M)
    row_ptr, col_ind, val = M.csr
    assert_bits(sm.ilu0_host(M.n, row_ptr, col_ind, val), F.csr[2], M.name)
    assert sm.ilu0_check(M.n, row_ptr, col_ind).tolist() == im.diag_positions(M).tolist()
    in_place = np.array(val, dtype=np.float64)
    assert sm.lib().smvp_csr_ilu0_host(M.n, sm._p(row_ptr), sm._p(col_ind), sm._p(in_place), sm._p(in_place)) == sm.OK
    assert_bits(in_place, F.csr[2], M.name + ": val_out is val")
    f = M.facts(im.LOWER, im.UNIT)
    print("%s: %d rows, %d entries, %d pivots, %d levels (widest %d)" % (M.name, M.n, M.nnz, f["off"], f["levels"], f["max_level_width"]))


def test_the_cases_cover_what_they_were_chosen_for():
    names = [im.case(W, i).name.split(",")[0] for i in ALL]
    facts = {n: im.case(W, i).facts(im.LOWER, im.UNIT) for i, n in enumerate(names)}
    assert facts["wide_thin_wide(256)"]["levels"] == 9 and facts["wide_thin_wide(256)"]["max_level_width"] == 768
    assert facts["adjacent(256)"]["widths"].tolist() == [256, 257, 256, 257, 256]
    assert facts["interleaved(1036)"]["widths"].tolist() == [259] * 4
    assert facts["dense_lower(70)"]["levels"] == 70 and facts["bidiagonal(1003)"]["levels"] == 1003
    assert facts["identity(1)"]["levels"] == 1
    assert np.diff(im.case(W, names.index("spd_long")).csr[0]).max() >= 700
    assert np.diff(im.case(W, names.index("memplus")).csr[0]).max() == 574 and facts["memplus"]["levels"] == 174
    dense = im.case(W, names.index("dense_lower(70)"))
    assert int((dense.csr[2] != im.factor(dense).csr[2]).sum()) >= 4000, "dense_lower(70): thousands of values changed"


# -------------------------------------------------------------------------------------------------------------------- the check
def check(rows, row_ptr, col_ind):
    """(status, bad_row, diag_pos as left by the call) of smvp_csr_ilu0_check on arrays poisoned with -7."""
    rp, ci = np.asarray(row_ptr, dtype=np.int32), np.asarray(col_ind, dtype=np.int32)
    dp, bad = np.full(max(rows, 1), -7, dtype=np.int32), C.c_int(-7)
    rc = sm.lib().smvp_csr_ilu0_check(rows, sm._p(rp), sm._p(ci), sm._p(dp), C.byref(bad))
    return rc, bad.value, dp[:rows].tolist()


def test_the_check_returns_diag_pos_or_the_first_bad_row_and_leaves_diag_pos_alone():
    rp, ci = [0, 2, 5, 7], [0, 1, 0, 1, 2, 1, 2]
    assert check(3, rp, ci) == (sm.OK, -1, [0, 3, 6])
    assert sm.lib().smvp_csr_ilu0_check(3, sm._p(np.array(rp, np.int32)), sm._p(np.array(ci, np.int32)), None, None) == sm.OK
    for what, rp_, ci_, code, row, word in (
            ("an unsorted row", rp, [0, 1, 1, 0, 2, 1, 2], sm.ERR_UNSUPPORTED, 1, "not sorted"),
            ("a repeated column", rp, [0, 1, 0, 1, 1, 1, 2], sm.ERR_UNSUPPORTED, 1, "repeated"),
            ("a missing diagonal", rp, [0, 1, 0, 1, 2, 0, 1], sm.ERR_UNSUPPORTED, 2, "no diagonal"),
            ("a column out of range", rp, [0, 1, 0, 1, 3, 1, 2], sm.ERR_INVALID, 1, "outside"),
            ("a negative column", rp, [0, 1, -1, 1, 2, 1, 2], sm.ERR_INVALID, 1, "outside"),
            ("a decreasing row_ptr", [0, 5, 2, 7], ci, sm.ERR_INVALID, 1, "decreases"),
            ("a row_ptr that does not start at 0", [1, 2, 5, 7], ci, sm.ERR_INVALID, 0, "row_ptr[0]")):
        rc, bad, dp = check(3, rp_, ci_)
        msg = sm.lib().smvp_last_error().decode()
        assert (rc, bad, dp) == (code, row, [-7, -7, -7]), "%s: %r (%s)" % (what, (rc, bad, dp), msg)
        assert word in msg and ("row %d" % row in msg or "row_ptr" in msg), "%s: %s" % (what, msg)
        out = np.full(7, -7.0)
        assert sm.lib().smvp_csr_ilu0_host(3, sm._p(np.array(rp_, np.int32)), sm._p(np.array(ci_, np.int32)), sm._p(np.ones(7)),
                                           sm._p(out)) == code
        assert (out == -7.0).all(), what + ": smvp_csr_ilu0_host wrote although it refused"
    assert sm.lib().smvp_csr_ilu0_check(-1, None, None, None, None) == sm.ERR_INVALID
    assert sm.lib().smvp_csr_ilu0_check(3, None, None, None, None) == sm.ERR_INVALID
    assert sm.lib().smvp_csr_ilu0_check(0, None, None, None, None) == sm.OK
    assert sm.ilu0_host(0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0)).tolist() == []
    with pytest.raises(sm.SmvpError) as e:
        sm.ilu0_check(3, rp, [0, 1, 0, 1, 2, 0, 1])
    assert e.value.code == sm.ERR_UNSUPPORTED and e.value.bad_row == 2


def test_what_the_suite_stores_with_repeats_unsorted_or_without_a_diagonal_is_refused():
    for M, word in ((trsv.of_matrix("spd(1003)", cg.spd(1003)), "repeated"),
                    (trsv.of_matrix("spd_shuffled", cg.spd_shuffled(), as_stored=True), "column"),
                    (trsv.sample("pdp08-pg4"), "no diagonal")):
        with pytest.raises(sm.SmvpError) as e:
            sm.ilu0_check(M.n, M.csr[0], M.csr[1])
        assert e.value.code == sm.ERR_UNSUPPORTED and word in str(e.value), str(e.value)


def test_the_symbols_are_declared_bound_and_exported():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "smvp_amd.h")).read()
    for name in ("smvp_csr_ilu0_create", "smvp_ilu0_factor", "smvp_ilu0_matrix", "smvp_ilu0_info", "smvp_ilu0_destroy",
                 "smvp_csr_ilu0_check", "smvp_csr_ilu0_host"):
        assert name + "(" in header and name in sm.EXPORTS and getattr(sm.lib(), name)
    assert C.sizeof(sm.Ilu0Info) == 64


# ------------------------------------------------------------------------------------------------- L U against A on the pattern
@pytest.mark.parametrize("i", ALL)
def test_l_times_u_matches_a_on_the_pattern_within_the_derived_bound(i):
    M = im.case(W, i)
    assert_l_times_u_is_a_on_the_pattern(M, im.factor(M))


def assert_l_times_u_is_a_on_the_pattern(M, F):
    """|a_ij - (L U)_ij| <= gamma_(m + 1) (|L| |U|)_ij at every stored position of M, for the factor F (a Case on M's pattern)."""
    total, mag, terms, S = im.product_terms(M, F)                                    # integers times 2^(2 S)
    worst = 0.0
    for p, a in enumerate(M.csr[2].tolist()):
        n, d = a.as_integer_ratio()
        err = abs(n * (1 << (2 * S)) - total[p] * d)                                 # |a - (L U)| times d 2^(2 S), exact
        m = terms[p] + 1                                                             # gamma_m = m u / (1 - m u) = m / (2^53 - m)
        assert err * (2 ** 53 - m) <= m * mag[p] * d, "%s: position %d: |a - (L U)| = %g > gamma_%d |L| |U| = %g" % (
            M.name, p, err / d / 4.0 ** S, m, float(gamma(m)) * mag[p] / 4.0 ** S)
        if mag[p]:
            worst = max(worst, err * (2 ** 53 - m) / (m * mag[p] * d))
    print("%s: the largest share of the bound used is %.3g, the most terms %d" % (M.name, worst, max(terms)))


@pytest.mark.parametrize("name", ["tridiagonal(300)", "dense_lower(70)"])
def test_without_fill_l_times_u_is_all_of_a(name):
    """A tridiagonal and a dense pattern admit no fill: every product l_ik u_kj lands on a stored position, so the bound on the
    pattern is the bound on the whole of A - L U.  Held here on what the LIBRARY's host loop returns, not on the restatement."""
    M = [im.case(W, i) for i in ALL if im.case(W, i).name.startswith(name)][0]
    row_ptr, col_ind, val = M.csr
    F = trsv.Case.of_csr("smvp_csr_ilu0_host(%s)" % M.name, M.n, row_ptr, col_ind, sm.ilu0_host(M.n, row_ptr, col_ind, val))
    assert (F.csr[1] == col_ind).all()
    assert_l_times_u_is_a_on_the_pattern(M, F)
    dp = im.diag_positions(M)
    stored = set(zip(np.repeat(np.arange(M.n), np.diff(row_ptr)).tolist(), col_ind.tolist()))
    for i in range(M.n):
        for p in range(row_ptr[i], dp[i]):
            k = int(col_ind[p])
            assert all((i, int(col_ind[q])) in stored for q in range(dp[k] + 1, row_ptr[k + 1])), "fill at row %d" % i


# ------------------------------------------------------------------------------------------- what the factor buys conjugate gradients
SYSTEMS = {"lap2d(16)": lambda: im.grid(16), "lap2d(32)": lambda: im.grid(32),
           "scaled(1003)": lambda: im.of_matrix("scaled(1003)", pcg.scaled(cg.spd(1003), 2)),
           "spd(3001)": lambda: im.of_matrix("spd(3001)", cg.spd(3001))}


@pytest.mark.parametrize("name", list(SYSTEMS))
def test_cg_preconditioned_with_the_factor_converges_and_beats_sgs_on_the_grids(name):
    """|b - A x| <= 2 tol |b| as in test_pcg_tri_host.py: the rule stops on the recurrence's r, hence the factor 2."""
    Cs = SYSTEMS[name]()
    A = im.as_matrix(Cs)
    b = cg.rhs(Cs.n)
    first, m, second = im.plans(im.factor(Cs))
    steps, updates, reason, rr, rz, sigma, x = tri.run(A.spmv, b, None, first, m, second, 200, TOL)
    true = np.linalg.norm(b - A.spmv(x)) / np.linalg.norm(b)
    sgs = tri.run(A.spmv, b, None, *tri.sgs(Cs), 200, TOL)
    print("%s: ILU(0) %d steps, SGS %d; |b - A x| / |b| = %.3g" % (name, steps, sgs[0], true))
    assert reason == tri.CONVERGED and steps == updates < 200 and sgs[2] == tri.CONVERGED
    assert true <= 2.0 * TOL
    if name.startswith("lap2d"):
        assert steps < sgs[0]
