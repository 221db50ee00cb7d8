"""CPU: the restatement of the sparse triangular solves (tests/trsv_method.py, kernel K15) against hand-computed exact cases and a
derived backward-error bound, and the library's host analysis smvp_csr_trsv_levels against the restatement's levels.  No GPU."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import smvp_toolkit_amd as sm
import trsv_method as tm
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_trsv_create", "smvp_trsv_solve", "smvp_trsv_info", "smvp_trsv_schedule", "smvp_trsv_destroy", "smvp_csr_trsv_levels")
W = 8   # a chain width for the constructed schedules here: the restatement takes it as an argument, the library's is not mirrored
BOTH = [(u, d) for u in (LOWER, UPPER) for d in (STORED, UNIT)]


def all_cases():
    return tm.existing_cases() + tm.constructed_cases(W) + (tm.order_dependent(),)


# ------------------------------------------------------------------------------------------- hand-computed, dyadic: exact
def three():
    """Other-triangle entries in every row, a repeated diagonal entry in row 1, unsorted columns.
         [ 2    .    8 ]
         [ .5  1+1   4 ]      b = (1, 3, 2)
         [ .25 -2    4 ]"""
    r = [0, 0, 1, 1, 1, 1, 2, 2, 2]
    c = [2, 0, 1, 0, 1, 2, 1, 2, 0]
    v = [8.0, 2.0, 1.0, 0.5, 1.0, 4.0, -2.0, 4.0, 0.25]
    return tm.Case("three", 3, r, c, v, b=[1.0, 3.0, 2.0])


def four():
    """A repeated off-diagonal entry in row 2, a repeated diagonal entry in row 3, unsorted columns.
         [ 4    2    .    1  ]
         [ 1    2    .   -1  ]      b = (4, 2, 8, 1)
         [ 2+2 -4    8    .  ]
         [ -1   .5   1  .5+.5]"""
    r = [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 3]
    c = [0, 3, 1, 0, 1, 3, 2, 0, 1, 0, 1, 2, 3, 3, 0]
    v = [4.0, 1.0, 2.0, 1.0, 2.0, -1.0, 8.0, 2.0, -4.0, 2.0, 0.5, 1.0, 0.5, 0.5, -1.0]
    return tm.Case("four", 4, r, c, v, b=[4.0, 2.0, 8.0, 1.0])


HAND = [
    # x0 = 1/2; x1 = (3 - .5 * .5) / 2; x2 = (2 - (-2 * 1.375 + .25 * .5)) / 4
    (three, LOWER, STORED, [0.5, 1.375, 1.15625]),
    # x0 = 1; x1 = 3 - .5; x2 = 2 - (-2 * 2.5 + .25)
    (three, LOWER, UNIT, [1.0, 2.5, 6.75]),
    # x2 = 2/4; x1 = (3 - 4 * .5) / 2; x0 = (1 - 8 * .5) / 2
    (three, UPPER, STORED, [-1.5, 0.5, 0.5]),
    # x2 = 2; x1 = 3 - 4 * 2; x0 = 1 - 8 * 2
    (three, UPPER, UNIT, [-15.0, -5.0, 2.0]),
    # x0 = 4/4; x1 = (2 - 1) / 2; x2 = (8 - (2 - 2 + 2)) / 8; x3 = (1 - (.25 + .75 - 1)) / 1
    (four, LOWER, STORED, [1.0, 0.5, 0.75, 1.0]),
    # x0 = 4; x1 = 2 - 4; x2 = 8 - (8 + 8 + 8); x3 = 1 - (-1 - 16 - 4)
    (four, LOWER, UNIT, [4.0, -2.0, -16.0, 22.0]),
    # x3 = 1/1; x2 = 8/8; x1 = (2 + 1) / 2; x0 = (4 - (1 + 3)) / 4
    (four, UPPER, STORED, [0.0, 1.5, 1.0, 1.0]),
    # x3 = 1; x2 = 8; x1 = 2 + 1; x0 = 4 - (1 + 6)
    (four, UPPER, UNIT, [-3.0, 3.0, 8.0, 1.0]),
]


@pytest.mark.parametrize("make,uplo,diag,want", HAND)
def test_hand_computed_exact_cases(make, uplo, diag, want):
    M = make()
    assert_bits(M.reference(uplo, diag)[1], np.array(want), "%s, uplo %d, diag %d" % (M.name, uplo, diag))


def test_hand_computed_levels_and_schedules():
    assert tm.levels(3, *three().csr[:2], LOWER).tolist() == [0, 1, 2]
    assert tm.levels(3, *three().csr[:2], UPPER).tolist() == [1, 1, 0]
    assert tm.levels(4, *four().csr[:2], LOWER).tolist() == [0, 1, 2, 3]
    assert tm.levels(4, *four().csr[:2], UPPER).tolist() == [2, 1, 0, 0]
    level_ptr, order = tm.schedule([2, 1, 0, 0, 1])
    assert level_ptr.tolist() == [0, 2, 4, 5] and order.tolist() == [2, 3, 1, 4, 0]
    level_ptr, order = tm.schedule([])
    assert level_ptr.tolist() == [0] and order.tolist() == []
    assert tm.launches([], 4) == 0 and tm.launches([1], 4) == 1 and tm.launches([5], 4) == 1
    assert tm.launches([4, 4, 5, 1, 5, 5, 2, 2], 4) == 6 and tm.chains([4, 4, 5, 1, 5, 5, 2, 2], 4) == 3
    f = four().facts(LOWER, STORED)
    assert (f["entries"], f["missing_diagonals"]) == (7 + 5, 0) and four().facts(LOWER, UNIT)["entries"] == 7
    assert four().facts(UPPER, STORED)["entries"] == 3 + 5


def test_the_cases_are_what_their_names_say():
    w = W
    by = {M.name: M for M in tm.constructed_cases(w)}
    assert by["bidiagonal(%d)" % (w + 1)].facts(LOWER, STORED)["widths"].tolist() == [1] * (w + 1)
    assert by["bidiagonal(1003), flipped"].facts(UPPER, STORED)["widths"].tolist() == [1] * 1003
    assert by["dense_lower(70)"].facts(LOWER, STORED)["levels"] == 70 and np.diff(by["dense_lower(70)"].csr[0]).max() == 70
    assert by["wide_thin_wide(%d)" % w].facts(LOWER, STORED)["widths"].tolist() == [3 * w, w, 1, w - 1, 7, w, w + 1, 3, 1]
    assert tm.launches(by["wide_thin_wide(%d)" % w].facts(LOWER, STORED)["widths"], w) == 4
    assert by["wide_thin_wide(%d), flipped" % w].facts(UPPER, STORED)["widths"].tolist() == [3 * w, w, 1, w - 1, 7, w, w + 1, 3, 1]
    assert by["adjacent(%d)" % w].facts(LOWER, STORED)["widths"].tolist() == [w, w + 1, w, w + 1, w]
    D = by["divergent(%d)" % w]
    inside = np.bincount(D.entries()[0][D.entries()[1] < D.entries()[0]], minlength=D.n)
    assert sorted(set(inside.tolist())) == [0, 1, 300]
    assert abs(np.diff(inside[6:]).astype(int)).max() == 299, "neighbouring lanes take a short and a long row"
    I = by["interleaved(%d)" % (2 * w)]
    assert (I.facts(LOWER, STORED)["level_of_row"] == np.arange(2 * w) % 4).all()
    assert tm.launches(I.facts(LOWER, STORED)["widths"], w) == 1 and tm.launches(by["interleaved(%d)" % (4 * w + 12)].facts(LOWER, STORED)["widths"], w) == 4
    for M in tm.constructed_cases(w):
        r, c, v = M.entries()
        off = np.bincount(r[r != c], weights=np.abs(v[r != c]), minlength=M.n)
        assert off.max() <= 0.5 and ((v[r == c] >= 1.0) & (v[r == c] <= 2.0)).all(), M.name
    S = tm.existing_cases()[2]
    r, c, _ = S.entries()
    assert S.name == "spd_shuffled" and (np.diff(c)[np.diff(r) == 0] < 0).any() and len(set(zip(r.tolist(), c.tolist()))) < S.nnz


def test_dominant_values_bound_the_solution():
    for M in all_cases()[4:]:
        if M.name == "order_dependent":
            continue
        for uplo, diag in BOTH:
            if diag == UNIT or M.finite_stored:
                b, x = M.reference(uplo, diag)
                assert np.abs(x).max() <= 2.0 * np.abs(b).max(), "%s, uplo %d, diag %d" % (M.name, uplo, diag)


def test_storage_order_shows_in_the_restatement():
    O = tm.order_dependent()
    assert_bits(O.reference(LOWER, STORED)[1], [1.0, 1.0, 1.0, 1.0], "the stored order: (1e16 + 1) - 1e16 = 0")
    assert_bits(tm.sorted_copy(O).reference(LOWER, STORED)[1], [1.0, 1.0, 1.0, 0.0], "sorted columns: (-1e16 + 1e16) + 1 = 1")
    S = tm.existing_cases()[2]
    a, b = S.reference(LOWER, STORED)[1], tm.sorted_copy(S).reference(LOWER, STORED)[1]
    assert (a.view(np.int64) != b.view(np.int64)).any(), "spd_shuffled: a sorted copy gives other bits"


def test_the_other_triangle_is_ignored_and_explicit_zeros_only_add_levels():
    for M in (tm.existing_cases()[0], tm.existing_cases()[2]):
        for uplo, diag in BOTH:
            want = M.reference(uplo, diag)[1]
            assert_bits(tm.triangle_of(M, uplo).reference(uplo, diag)[1], want, "%s: the triangle alone" % M.name)
            Z = tm.triangle_of(M, uplo, zeros=True)
            assert_bits(Z.reference(uplo, diag)[1], want, "%s: zeros in the other triangle" % M.name)
            assert_bits(Z.reference(1 - uplo, UNIT)[1], Z.reference(1 - uplo, UNIT)[0], "T = I + stored zeros: x = b")
            assert Z.facts(1 - uplo, UNIT)["levels"] == M.facts(1 - uplo, UNIT)["levels"] > 1, "stored zeros are structure"


def test_nonfinite_cases_are_nonfinite_where_the_diagonal_says_so():
    P = tm.existing_cases()[-1]
    assert P.name == "pdp08-pg4" and P.facts(LOWER, STORED)["missing_diagonals"] == 1 and not P.finite_stored
    x = tm.solve(P, LOWER, STORED, tm.rhs(P.n), finite=False)
    r, c, _ = P.entries()
    missing = np.setdiff1d(np.arange(P.n), r[r == c])
    assert not np.isfinite(x[missing]).any() and np.isfinite(P.reference(LOWER, UNIT)[1]).all()
    with pytest.raises(AssertionError):
        tm.solve(P, LOWER, STORED, tm.rhs(P.n), finite=True)


# -------------------------------------------------------------------------------- a derived bound on the backward error
def gamma(m):
    u = Fraction(1, 2 ** 53)
    return m * u / (1 - m * u)


@pytest.mark.parametrize("i", [i for i, M in enumerate(all_cases()) if M.n <= 300])
def test_the_backward_error_is_within_highams_bound(i):
    """|b - T x^|_i <= gamma_{k_i + 2} (|T| |x^|)_i, the residual evaluated exactly in fractions.  Derivation: the computed s^ is a
    sum of k_off products added from +0.0 (exact), so each term carries at most k_off roundings (one product, k_off - 1 further
    additions): s^ = sum v x^_c (1 + theta_{k_off}).  Likewise d^ = sum d_p (1 + theta_{k_d - 1}).  Then x^_i = (b_i - s^)(1 + e1) /
    d^ (1 + e2), so b_i = s^ + d^ x^_i / ((1 + e1)(1 + e2)): every term of T x^ carries at most max(k_off, k_d + 1) <= k_i + 2
    factors (1 + e)^+-1 with |e| <= u, and |theta_m| <= gamma_m (Higham, Accuracy and Stability, lemma 3.1 and theorem 8.5 with
    two operations to spare).  No underflow or overflow on these values."""
    M = all_cases()[i]
    row_ptr, col_ind, val = M.csr
    for uplo, diag in BOTH:
        if diag == STORED and not M.finite_stored:
            continue
        b, x = M.reference(uplo, diag)
        xf = [Fraction(float(t)) for t in x]
        for r in range(M.n):
            tx, scale, k = Fraction(0), Fraction(0), 0
            for p in range(row_ptr[r], row_ptr[r + 1]):
                c, v = int(col_ind[p]), Fraction(float(val[p]))
                if (c == r and diag == STORED) or ((c < r) if uplo == LOWER else (c > r)):
                    tx += v * xf[c]
                    scale += abs(v) * abs(xf[c])
                    k += 1
            if diag == UNIT:
                tx += xf[r]
                scale += abs(xf[r])
                k += 1
            assert abs(Fraction(float(b[r])) - tx) <= gamma(k + 2) * scale, "%s, uplo %d, diag %d, row %d of %d entries" % (
                M.name, uplo, diag, r, k)


# --------------------------------------------------------------------------------------- the library's host analysis
def library_levels(M, uplo):
    row_ptr, col_ind, _ = M.csr
    return sm.trsv_levels(M.n, row_ptr, col_ind, uplo)


@pytest.mark.parametrize("i", range(len(all_cases())))
def test_the_librarys_levels_are_the_restatements(i):
    M = all_cases()[i]
    for uplo in (LOWER, UPPER):
        level, count = library_levels(M, uplo)
        f = M.facts(uplo, STORED)
        assert count == f["levels"], "%s, uplo %d" % (M.name, uplo)
        assert (level == f["level_of_row"]).all(), "%s, uplo %d" % (M.name, uplo)


PINNED = {"ibm32": (7, 8), "curtis54": (39, 34), "memplus": (174, 174), "pwt": (237, 1), "pdp08-pg4": (3, 4)}


@pytest.mark.parametrize("name", tm.SAMPLES)
def test_known_level_counts_of_the_golden_samples(name):
    M = {c.name: c for c in tm.existing_cases()}[name]
    assert (library_levels(M, LOWER)[1], library_levels(M, UPPER)[1]) == PINNED[name]
    assert (M.facts(LOWER, STORED)["levels"], M.facts(UPPER, STORED)["levels"]) == PINNED[name]
    if name == "memplus":
        assert (M.facts(LOWER, STORED)["max_level_width"], M.facts(UPPER, STORED)["max_level_width"]) == (1587, 7419)
        widths = np.bincount(library_levels(M, LOWER)[0])
        assert widths.max() == 1587 and (widths <= 256).sum() == 160 and widths[widths <= 256].sum() == 7578


def test_an_empty_matrix_and_one_row():
    level, count = sm.trsv_levels(0, np.zeros(1, np.int32), np.zeros(0, np.int32), LOWER)
    assert count == 0 and len(level) == 0
    for cols in ([], [0], [0, 0]):
        level, count = sm.trsv_levels(1, np.array([0, len(cols)], np.int32), np.array(cols, np.int32), UPPER)
        assert count == 1 and level.tolist() == [0]


def test_refusals_that_need_no_device():
    L = sm.lib()
    M = four()
    row_ptr, col_ind, _ = M.csr
    level, count = np.full(4, -7, np.int32), C.c_int(-7)

    def refused(rows, rp, ci, uplo, lv, cnt, word):
        assert L.smvp_csr_trsv_levels(rows, rp, ci, uplo, lv, cnt) == sm.ERR_INVALID
        assert word in L.smvp_last_error(), L.smvp_last_error()
        assert (level == -7).all() and count.value == -7, "outputs touched"

    for uplo in (-1, 2, 7):
        refused(4, sm._p(row_ptr), sm._p(col_ind), uplo, sm._p(level), C.byref(count), b"uplo")
    refused(4, None, sm._p(col_ind), LOWER, sm._p(level), C.byref(count), b"row_ptr")
    refused(4, sm._p(row_ptr), None, LOWER, sm._p(level), C.byref(count), b"col_ind")
    refused(4, sm._p(row_ptr), sm._p(col_ind), LOWER, None, C.byref(count), b"level_of_row")
    refused(4, sm._p(row_ptr), sm._p(col_ind), LOWER, sm._p(level), None, b"levels")
    refused(-1, sm._p(row_ptr), sm._p(col_ind), LOWER, sm._p(level), C.byref(count), b"rows")
    bad = col_ind.copy()
    bad[5] = 4
    refused(4, sm._p(row_ptr), sm._p(bad), UPPER, sm._p(level), C.byref(count), b"col_ind[5]")
    bad[5] = -1
    refused(4, sm._p(row_ptr), sm._p(bad), LOWER, sm._p(level), C.byref(count), b"col_ind[5]")
    down = row_ptr.copy()
    down[2] = down[1] - 1
    refused(4, sm._p(down), sm._p(col_ind), LOWER, sm._p(level), C.byref(count), b"row_ptr")
    assert L.smvp_csr_trsv_levels(0, None, None, LOWER, None, C.byref(count)) == sm.OK and count.value == 0
    # the calls on a handle or a plan refuse a null one before any device call
    out = C.c_void_p()
    assert L.smvp_csr_trsv_create(None, None, LOWER, STORED, None) == sm.ERR_INVALID and b"out" in L.smvp_last_error()
    assert L.smvp_csr_trsv_create(C.byref(out), None, LOWER, STORED, None) == sm.ERR_INVALID and b"handle" in L.smvp_last_error()
    assert out.value is None
    assert L.smvp_trsv_solve(None, None, None, None) == sm.ERR_INVALID and b"plan" in L.smvp_last_error()
    assert L.smvp_trsv_info(None, C.byref(sm.TrsvInfo())) == sm.ERR_INVALID
    assert L.smvp_trsv_schedule(None, None, None) == sm.ERR_INVALID
    L.smvp_trsv_destroy(None)


def test_trsv_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    assert re.search(r"\}\s*smvp_trsv_info_t\s*;", header)
    assert C.sizeof(sm.TrsvInfo) == 56 and sm.TrsvInfo.entries.offset == 32 and sm.TrsvInfo.build_ms.offset == 48
    for i, name in enumerate(("LOWER", "UPPER")):
        assert re.search(r"\bSMVP_TRSV_%s\s*=\s*%d\b" % (name, i), header) and getattr(sm, "TRSV_" + name) == i == getattr(tm, name)
    for i, name in enumerate(("STORED", "UNIT")):
        assert re.search(r"\bSMVP_TRSV_DIAG_%s\s*=\s*%d\b" % (name, i), header) and getattr(sm, "TRSV_DIAG_" + name) == i == getattr(tm, name)
    for method in ("solve", "info", "schedule", "close"):
        assert callable(getattr(sm.TrsvPlan, method)), method
    assert callable(sm.CsrMatrix.trsv_plan) and callable(sm.trsv_levels)
