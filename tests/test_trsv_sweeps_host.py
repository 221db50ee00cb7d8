"""CPU: the restatement of the Jacobi-sweep triangular solves (tests/trsv_sweeps_method.py, kernel K21) against hand-computed exact
cases, against trsv_method.solve (levels - 1 sweeps are the exact solve, bit for bit) and against a derived contraction bound; the
storage ranges; and the refusals of smvp_csr_trsv_create_sweeps / smvp_trsv_sweeps that need no device.  No GPU."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import smvp_toolkit_amd as sm
import trsv_method as tm
import trsv_sweeps_method as ts
from test_trsv_host import four, three
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("smvp_csr_trsv_create_sweeps", "smvp_trsv_sweeps")
BOTH = [(u, d) for u in (LOWER, UPPER) for d in (STORED, UNIT)]


# ------------------------------------------------------------------------------------------- hand-computed, dyadic: exact
# three (test_trsv_host.py):  [ 2 . 8 ; .5 1+1 4 ; .25 -2 4 ],  b = (1, 3, 2);   four:  [ 4 2 . 1 ; 1 2 . -1 ; 2+2 -4 8 . ; -1 .5 1 .5+.5 ],
# b = (4, 2, 8, 1).  Every diagonal sum is a power of two, so every iterate is dyadic and the floats below are exact.
HAND = [
    # x(0) = (1/2, 3/2, 2/4); x(1) = (., (3 - .5 * .5) / 2, (2 - (-2 * 1.5 + .25 * .5)) / 4); x(2)_2 = (2 - (-2 * 1.375 + .125)) / 4
    (three, LOWER, STORED, [[0.5, 1.5, 0.5], [0.5, 1.375, 1.21875], [0.5, 1.375, 1.15625]]),
    # x(0) = b; x(1) = (1, 3 - .5, 2 - (-2 * 3 + .25)); x(2)_2 = 2 - (-2 * 2.5 + .25)
    (three, LOWER, UNIT, [[1.0, 3.0, 2.0], [1.0, 2.5, 7.75], [1.0, 2.5, 6.75]]),
    # x(1) = ((1 - 8 * .5) / 2, (3 - 4 * .5) / 2, .5): two levels, exact after one sweep
    (three, UPPER, STORED, [[0.5, 1.5, 0.5], [-1.5, 0.5, 0.5], [-1.5, 0.5, 0.5]]),
    # x(1) = (1 - 8 * 2, 3 - 4 * 2, 2)
    (three, UPPER, UNIT, [[1.0, 3.0, 2.0], [-15.0, -5.0, 2.0], [-15.0, -5.0, 2.0]]),
    # x(0) = (4/4, 2/2, 8/8, 1/1); x(1) = (1, (2 - 1) / 2, (8 - (2 - 4 + 2)) / 8, 1 - (.5 + 1 - 1));
    # x(2) = (1, .5, (8 - (2 - 2 + 2)) / 8, 1 - (.25 + 1 - 1))
    (four, LOWER, STORED, [[1.0, 1.0, 1.0, 1.0], [1.0, 0.5, 1.0, 0.5], [1.0, 0.5, 0.75, 0.75]]),
    # x(1) = (4, 2 - 4, 8 - (8 - 8 + 8), 1 - (1 + 8 - 4)); x(2) = (4, -2, 8 - (8 + 8 + 8), 1 - (-1 + 0 - 4))
    (four, LOWER, UNIT, [[4.0, 2.0, 8.0, 1.0], [4.0, -2.0, 0.0, -4.0], [4.0, -2.0, -16.0, 6.0]]),
    # x(1) = ((4 - (1 + 2)) / 4, (2 + 1) / 2, 1, 1); x(2)_0 = (4 - (1 + 3)) / 4
    (four, UPPER, STORED, [[1.0, 1.0, 1.0, 1.0], [0.25, 1.5, 1.0, 1.0], [0.0, 1.5, 1.0, 1.0]]),
    # x(1) = (4 - (1 + 4), 2 + 1, 8, 1); x(2)_0 = 4 - (1 + 6)
    (four, UPPER, UNIT, [[4.0, 2.0, 8.0, 1.0], [-1.0, 3.0, 8.0, 1.0], [-3.0, 3.0, 8.0, 1.0]]),
]


def in_fractions(M, uplo, diag, sweeps):
    """The iteration in exact rationals from the entries (the order of a sum does not matter there)."""
    r, c, v = (a.tolist() for a in M.entries())
    b = [Fraction(t) for t in M.b]
    d = [sum((Fraction(v[p]) for p in range(M.nnz) if r[p] == i and c[p] == i), Fraction(0)) if diag == STORED else Fraction(1) for i in range(M.n)]
    x = [b[i] / d[i] for i in range(M.n)]
    for _ in range(sweeps):
        s = [Fraction(0)] * M.n
        for p in range(M.nnz):
            if (c[p] < r[p]) if uplo == LOWER else (c[p] > r[p]):
                s[r[p]] += Fraction(v[p]) * x[c[p]]
        x = [(b[i] - s[i]) / d[i] for i in range(M.n)]
    return x


@pytest.mark.parametrize("make,uplo,diag,want", HAND)
def test_hand_computed_exact_cases(make, uplo, diag, want):
    M = make()
    for sweeps in (0, 1, 2):
        got = ts.solve(M, uplo, diag, M.b, sweeps)
        assert_bits(got, np.array(want[sweeps]), "%s, uplo %d, diag %d, %d sweeps" % (M.name, uplo, diag, sweeps))
        assert [Fraction(t) for t in got.tolist()] == in_fractions(M, uplo, diag, sweeps)


def test_hand_computed_ranges():
    assert [a.tolist() for a in ts.ranges(three(), LOWER, STORED)] == [[1, 2, 6], [2, 5, 9]]     # rows: columns 2 0 | 1 0 1 2 | 1 2 0
    assert [a.tolist() for a in ts.ranges(three(), LOWER, UNIT)] == [[0, 3, 6], [0, 4, 9]]       # row 0 has none: empty at its start
    assert [a.tolist() for a in ts.ranges(three(), UPPER, STORED)] == [[0, 2, 7], [2, 6, 8]]
    assert [a.tolist() for a in ts.ranges(three(), UPPER, UNIT)] == [[0, 5, 6], [1, 6, 6]]
    assert [a.tolist() for a in ts.ranges(four(), LOWER, STORED)] == [[0, 3, 6, 10], [1, 5, 10, 15]]
    assert ts.entries(three(), LOWER, STORED) == 1 + 3 + 3 and ts.entries(four(), UPPER, UNIT) == 2 + 1 + 0 + 0
    E = tm.Case("empty", 0, [], [], [])
    assert [a.tolist() for a in ts.ranges(E, LOWER, STORED)] == [[], []] and len(ts.solve(E, LOWER, STORED, [], 3)) == 0


# --------------------------------------------------------------------------------- levels - 1 sweeps are the exact solve
def all_cases():
    return tm.existing_cases() + tm.constructed_cases(256)


def shaped(M):
    """The triangles of a case that hold more than a diagonal (both for the existing cases)."""
    return [u for u in (LOWER, UPPER) if M.facts(u, STORED)["levels"] > 1] or [LOWER]


@pytest.mark.parametrize("i", range(len(all_cases())))
def test_levels_less_one_sweeps_have_the_exact_solves_bits(i):
    """A row of level l reads rows of levels below l only, by the same rule in the same order: by induction x(m)_i is the exact
    solve's x_i for every row of level <= m."""
    M = all_cases()[i]
    for uplo in shaped(M):
        for diag in (STORED, UNIT):
            b, want = M.reference(uplo, diag)
            got = ts.solve(M, uplo, diag, b, max(M.facts(uplo, diag)["levels"] - 1, 0))
            if diag == STORED and not M.finite_stored:
                assert (np.isnan(got) == np.isnan(want)).all()
                assert_bits(got[~np.isnan(want)], want[~np.isnan(want)], "%s, uplo %d: where the exact solve is no NaN" % (M.name, uplo))
            else:
                assert_bits(got, want, "%s, uplo %d, diag %d" % (M.name, uplo, diag))


def test_one_sweep_fewer_is_not_the_exact_solve_and_rows_settle_level_by_level():
    """bidiagonal(257) has 257 levels, but its dominant values contract the error by 1/2 a sweep: after 255 sweeps the last row is
    2^-255 |b| from the exact solve's, which no double shows.  So the structure is kept and the values are chosen so that row 0's
    b has to travel the whole chain: -1 below a diagonal of 1 and b = e_0 give x = (1, ..., 1) exactly, and x(m) is 1 in the rows
    0 .. m and 0 below them.  levels - 2 sweeps then miss exactly the last row."""
    B = tm.bidiagonal(257)
    r, c, _ = B.entries()
    M = tm.Case("bidiagonal(257), a carry", 257, r, c, np.where(r == c, 1.0, -1.0), b=np.eye(257)[0])
    for diag in (STORED, UNIT):
        b, want = M.reference(LOWER, diag)
        assert M.facts(LOWER, diag)["levels"] == 257 and (want == 1.0).all()
        got = ts.solve(M, LOWER, diag, b, 255)
        assert got[-1].view(np.int64) != want[-1].view(np.int64) and got[-1] == 0.0, "the last row (level 256) after 255 sweeps"
        assert_bits(got[:-1], want[:-1], "every row of level <= 255")
        assert_bits(ts.solve(M, LOWER, diag, b, 256), want, "levels - 1 sweeps")
    W = tm.wide_thin_wide(8)
    level = W.facts(LOWER, STORED)["level_of_row"]
    b, want = W.reference(LOWER, STORED)
    for m in range(W.facts(LOWER, STORED)["levels"]):
        got = ts.solve(W, LOWER, STORED, b, m)
        assert_bits(got[level <= m], want[level <= m], "rows of level <= %d after %d sweeps" % (m, m))


# ------------------------------------------------------------------------------------------- the derived contraction bound
def test_the_error_halves_with_every_sweep_on_dominant_values():
    """trsv_method.dominant: a row's off-diagonal magnitudes sum to at most 1/2 and every stored diagonal is at least 1 (a unit
    one is 1), so |x|_inf <= 2 |b|_inf.  e(m) = x(m) - x obeys e(m+1)_i = -(sum of t_ic e(m)_c) / d_i, hence |e(m+1)|_inf <=
    |e(m)|_inf / 2; and e(0)_i = (sum of t_ic x_c) / d_i, so |e(0)|_inf <= (1/2) * 2 |b|_inf = |b|_inf.  In floating point
    every operation adds a relative 2^-53 on numbers bounded by 2 |b|_inf: 1e-12 covers rows of thousands of entries."""
    seen = 0
    for M in tm.existing_cases()[4:]:
        for uplo, diag in BOTH:
            if diag == STORED and not M.finite_stored:
                continue
            b, x = M.reference(uplo, diag)
            top = np.abs(b).max()
            for m in range(11):
                err = np.abs(ts.solve(M, uplo, diag, b, m) - x).max()
                assert err <= 2.0 ** -m * top * (1 + 1e-12), "%s, uplo %d, diag %d, %d sweeps: %g" % (M.name, uplo, diag, m, err)
            seen += 1
    assert seen == 5 * 4 - 2, "the five samples; pdp08-pg4's stored diagonal is not finite"


# -------------------------------------------------------------------------------------------------------------- the ranges
@pytest.mark.parametrize("i", range(len(all_cases())))
def test_ranges_are_tight_for_ascending_rows_and_hold_every_entry_that_counts(i):
    M = all_cases()[i]
    r, c, _ = M.entries()
    row_ptr = M.csr[0]
    ascending = np.ones(M.n, dtype=bool)
    same_row = np.diff(r) == 0
    np.logical_and.at(ascending, r[1:][same_row], np.diff(c)[same_row] >= 0)
    for uplo, diag in BOTH:
        begin, end = ts.ranges(M, uplo, diag)
        k = ts.kinds(M, uplo, diag)
        count = np.bincount(r[k != 0], minlength=M.n)
        assert (begin >= row_ptr[:-1]).all() and (end <= row_ptr[1:]).all() and (begin <= end).all()
        assert ((end - begin)[ascending] == count[ascending]).all(), "%s: a sorted row's range is tight" % M.name
        assert ((end - begin) >= count).all()
        p = np.arange(M.nnz)
        assert not (k[(p < begin[r]) | (p >= end[r])]).any(), "%s: an entry that counts lies outside its row's range" % M.name
        assert ts.entries(M, uplo, diag) == int((end - begin).sum()) >= M.facts(uplo, diag)["entries"]
        if ascending.all():
            assert ts.entries(M, uplo, diag) == M.facts(uplo, diag)["entries"]


def test_summing_over_the_range_alone_gives_the_whole_rows_bits():
    S = tm.existing_cases()[2]
    L = tm.leveled("leveled, shuffled", [40, 9, 33, 5], lambda l, k: 1 + (3 * k + l) % 9, 20321, shuffle=True)
    assert S.name == "spd_shuffled"
    for M in (S, L):
        r, c, _ = M.entries()
        assert (np.diff(c)[np.diff(r) == 0] < 0).any(), "%s holds unsorted rows" % M.name
        loose = 0
        for uplo, diag in BOTH:
            within = ts.ranges(M, uplo, diag)
            loose += ts.entries(M, uplo, diag) - M.facts(uplo, diag)["entries"]
            b = tm.rhs(M.n, 21)
            for sweeps in (0, 1, 3):
                assert_bits(ts.solve(M, uplo, diag, b, sweeps, within=within), ts.solve(M, uplo, diag, b, sweeps),
                            "%s, uplo %d, diag %d, %d sweeps" % (M.name, uplo, diag, sweeps))
        assert loose > 0, "%s: some range holds skipped entries" % M.name


# ------------------------------------------------------------------------------------------------ the library, no device
def test_refusals_that_need_no_device():
    L = sm.lib()
    out = C.c_void_p()
    # (the ranges of uplo, diag and sweeps are checked before the handle is looked at)
    assert L.smvp_csr_trsv_create_sweeps(None, None, LOWER, STORED, 3, None) == sm.ERR_INVALID and b"out" in L.smvp_last_error()
    assert L.smvp_csr_trsv_create_sweeps(C.byref(out), None, LOWER, STORED, 3, None) == sm.ERR_INVALID and b"handle" in L.smvp_last_error()
    for uplo, diag, sweeps, word in ((-1, STORED, 3, b"uplo"), (2, STORED, 3, b"uplo"), (LOWER, -1, 3, b"diag"), (LOWER, 2, 3, b"diag"),
                                     (LOWER, STORED, -1, b"sweeps"), (UPPER, UNIT, 4097, b"sweeps"), (UPPER, UNIT, -(2 ** 31), b"sweeps")):
        assert L.smvp_csr_trsv_create_sweeps(C.byref(out), None, uplo, diag, sweeps, None) == sm.ERR_INVALID
        assert word in L.smvp_last_error(), L.smvp_last_error()
        assert b"smvp_csr_trsv_create_sweeps" in L.smvp_last_error()
    for sweeps in (0, 4096):                                                          # the ends of the range pass that check
        assert L.smvp_csr_trsv_create_sweeps(C.byref(out), None, LOWER, STORED, sweeps, None) == sm.ERR_INVALID and b"handle" in L.smvp_last_error()
    assert out.value is None
    n = C.c_int(-7)
    assert L.smvp_trsv_sweeps(None, C.byref(n)) == sm.ERR_INVALID and b"plan" in L.smvp_last_error() and n.value == -7
    assert L.smvp_trsv_sweeps(None, None) == sm.ERR_INVALID


def test_the_symbols_are_declared_bound_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", sm.LIB_PATH], text=True)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS, name
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert getattr(sm.lib(), name).argtypes is not None, name
    assert re.search(r"\bSMVP_TRSV_MAX_SWEEPS\s*=\s*4096\b", header) and ts.MAX_SWEEPS == 4096
    assert C.sizeof(sm.TrsvInfo) == 56 and sm.TrsvInfo.entries.offset == 32 and sm.TrsvInfo.build_ms.offset == 48
    assert isinstance(sm.TrsvPlan.sweeps, property)
    import inspect
    for fn in (sm.CsrMatrix.trsv_plan, sm.TrsvPlan.__init__, sm.Ilu0.plans):
        assert inspect.signature(fn).parameters["sweeps"].default is None, fn
