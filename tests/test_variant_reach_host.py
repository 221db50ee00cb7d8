"""CPU: which variant of K15 and K17 every case of the suite runs (tests/variant_reach.py), the cases built to run the others
(tests/variant_cases.py), and the two tables the union must cover.  Nothing here runs a kernel: the rules are pinned to hand-computed
values, every new case to its intended shape, lane count and references, and the coverage is a condition on the restated rules --
test_gpu_trsv_variants.py and test_gpu_ilu0_variants.py pin the rules' constants to what the library reports."""
from fractions import Fraction

import numpy as np
import pytest

import ilu0_method as im
import smvp_toolkit_amd as sm
import trsv_method as trsv
import variant_cases as vc
import variant_reach as vr
from test_trsv_host import gamma, three
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

W = 256                                                                              # the chain width the CPU cases are built for
BOTH = [(u, d) for u in (LOWER, UPPER) for d in (STORED, UNIT)]
TRSV_CASES = vc.trsv_cases(W)
ILU0_CASES = vc.ilu0_cases(W)


# ------------------------------------------------------------------------------------------------------ the rules, by hand
def test_the_lane_rule_at_both_sides_of_every_power_of_two():
    assert [vr.pow2(x) for x in (0.0, 1.9, 2.0)] == [2, 2, 2]
    for p in (2, 4, 8, 16, 32):
        assert (vr.pow2(float(p)), vr.pow2(p + 1e-9), vr.pow2(2.0 * p)) == (p, 2 * p, 2 * p)
    assert vr.pow2(64.5) == vr.pow2(1e9) == 64
    # sqrt(mean * longest) / 4 with mean * 64 a square: 8 sqrt(mean) / 4 = 2 sqrt(mean) exactly; one entry more is the next power
    for mean, p in ((1.0, 2), (4.0, 4), (16.0, 8), (64.0, 16), (256.0, 32)):
        assert (vr.lanes_rule(mean, 64), vr.lanes_rule(mean, 65)) == (p, 2 * p)
    assert vr.lanes_rule(0.0, 0) == 2 and vr.lanes_rule(1024.0, 65) == 64


def test_the_rule_counts_the_triangle_with_its_diagonal_or_the_whole_rows():
    M = three()                                                                      # rows: columns 2 0 | 1 0 1 2 | 1 2 0
    assert vr.triangle_lengths(M, LOWER).tolist() == [1, 3, 3] and vr.triangle_lengths(M, UPPER).tolist() == [2, 3, 1]
    # dense_lower(k): mean (k + 1) / 2, longest k.  k = 10: sqrt(55) / 4 = 1.85; k = 11: sqrt(66) / 4 = 2.03; k = 15: sqrt(120) / 4 =
    # 2.74; k = 22: sqrt(253) / 4 = 3.98; k = 23: sqrt(276) / 4 = 4.15.  Its upper triangle is the diagonal: 1 / 4
    for k, p in ((10, 2), (11, 4), (15, 4), (22, 4), (23, 8)):
        D = trsv.dense_lower(k)
        assert (vr.wide_lanes_trsv(D, LOWER), vr.wide_lanes_trsv(D, UPPER), vr.wide_lanes_ilu0(D)) == (p, 2, p)
    # the whole rows where the triangle is half of them, a full 9 x 9: 9 / 4 = 2.25, the triangles' sqrt(5 * 9) / 4 = 1.68
    S = im.symmetrised(trsv.dense_lower(9), 1)
    assert (vr.wide_lanes_ilu0(S), vr.wide_lanes_trsv(S, LOWER), vr.wide_lanes_trsv(S, UPPER)) == (4, 2, 2)


def test_the_lanes_of_a_chains_level_and_the_hand_off_by_hand():
    got = {width: vr.chain_lanes(width) for width in (0, 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024)}
    assert got == {0: 64, 1: 64, 4: 64, 5: 32, 8: 32, 9: 16, 16: 16, 17: 8, 32: 8, 33: 4, 64: 4, 65: 2, 128: 2, 129: 1, 256: 1, 257: 1, 1024: 1}
    for T in (1, 2, 4, 8, 16, 32):
        assert not vr.ilu0_is_long(64 * T, T) and vr.ilu0_is_long(64 * T + 1, T)
    assert not vr.ilu0_is_long(10 ** 6, 64)


def test_passes_and_cells_by_hand():
    assert [vr.passes(n, 2) for n in (0, 7, 8, 9, 16, 17, 24, 25, 32, 33, 4000)] == [
        "1 partial", "1 partial", "1 full", "2", "2", "3", "3", "4", "4", "5+", "5+"]
    assert [vr.passes(n, 64) for n in (255, 256, 257, 1024, 1025, 1281)] == ["1 partial", "1 full", "2", "4", "5+", "5+"]
    assert vr.trsv_cell("chain", 1, 8) == ("chain", 1, "<=8") and vr.trsv_cell("chain", 1, 9) == ("chain", 1, ">8")
    assert vr.trsv_cell("wide", 32, 129) == ("wide", 32, "2")
    cell = vr.ilu0_cell
    assert cell(300, 16, 256, 2) == ("wide", 2, "regs") and cell(300, 17, 256, 2) == ("wide", 2, "mem")
    assert cell(300, 16, 512, 2) == ("chain", 1, "mem"), "inside a chain under the wider option: a lane takes the row alone"
    assert cell(200, 8, 256, 2) == ("chain", 1, "regs") and cell(200, 64, 256, 2) == ("chain", 1, "mem")
    assert cell(200, 65, 256, 2) == ("handed", 1, "regs") and cell(200, 513, 256, 2) == ("handed", 1, "mem")
    assert cell(40, 256, 256, 2) == ("chain", 4, "mem") and cell(40, 257, 256, 2) == ("handed", 4, "regs")
    assert cell(4, 512, 256, 2) == ("chain", 64, "regs") and cell(4, 5000, 256, 2) == ("chain", 64, "mem")


def test_the_reach_of_small_cases_by_hand():
    B = trsv.bidiagonal(5)                                                           # LOWER: five levels of one row; UPPER: one of five
    assert vr.reach_trsv(B, LOWER, 8) == {("chain", 64, "1 partial")} and vr.reach_trsv(B, UPPER, 8) == {("chain", 32, "1 partial")}
    assert vr.reach_trsv(B, UPPER, 4) == {("wide", 2, "1 partial")}
    D = trsv.dense_lower(40)                                                         # 40 levels of one row; rows of 1 .. 40 entries
    assert vr.reach_trsv(D, LOWER, 8) == {("chain", 64, "1 partial")}
    assert vr.reach_trsv(D, UPPER, 8) == {("wide", 2, p) for p in ("1 partial", "1 full", "2", "3", "4", "5+")}
    S = im.symmetrised(trsv.bidiagonal(5), 1)
    assert vr.reach_ilu0(S, 8) == {("chain", 64, "regs")}
    I = trsv.identity(300)
    assert vr.reach_ilu0(I, 256) == {("wide", 2, "regs")} and vr.reach_ilu0(I, 512) == {("chain", 1, "regs")}
    assert vr.handed_places(I, 512) == []


def test_updates_off_the_diagonal_by_hand():
    """A dense 3 x 3: row 1's pivot on row 0 (upper part 1, 2) updates (1, 1) and (1, 2); row 2's on row 0 updates (2, 1) and (2, 2),
    its pivot on row 1 (upper part 2) only the diagonal.  A tridiagonal matrix: every update lands on a diagonal."""
    assert vr.updates_off_the_diagonal(im.symmetrised(trsv.dense_lower(3), 1)).tolist() == [0, 1, 1]
    assert vr.updates_off_the_diagonal(im.symmetrised(trsv.bidiagonal(6), 1)).tolist() == [0] * 6


# ---------------------------------------------------------------------------------------------------------- the new cases' shape
@pytest.mark.parametrize("T", vc.TIERS_T)
def test_tiers_has_its_three_levels_its_lengths_and_its_lanes(T):
    M, Fl = vc.tiers(T, W), vc.tiers_flipped(T, W)
    nA = vc.KNOBS_TRSV[T][0]
    assert M.facts(LOWER, STORED)["widths"].tolist() == Fl.facts(UPPER, STORED)["widths"].tolist() == [nA, vc.N_B, W + 7]
    assert M.facts(UPPER, STORED)["levels"] == Fl.facts(LOWER, STORED)["levels"] == 1
    assert all((W + 7) % (4 * 64 // t) for t in vr.LANES), "the last wavefront's groups have no row, whatever T"
    assert vr.wide_lanes_trsv(M, LOWER) == vr.wide_lanes_trsv(Fl, UPPER) == T
    lengths = np.diff(M.csr[0])[nA + vc.N_B:]
    assert set(vc.special_lengths(T)) <= set(lengths.tolist())
    assert (vr.triangle_lengths(M, LOWER) == np.diff(M.csr[0])).all(), "lower triangular: a row's passes are its triangle's"
    want = {("wide", T, p) for p in vr.PASSES}
    assert want <= vr.reach_trsv(M, LOWER, W) and want <= vr.reach_trsv(Fl, UPPER, W)
    r, c, _ = M.entries()
    assert (np.diff(c)[np.diff(r) == 0] < 0).any(), "the storage order inside a row is shuffled"
    assert len(set(zip(r.tolist(), c.tolist()))) == M.nnz and M.nnz <= 50000
    # under the option that puts the last level into a chain a lane walks each of its rows alone: both of its loops
    assert {("chain", 1, "<=8"), ("chain", 1, ">8")} <= vr.reach_trsv(M, LOWER, 2 * W)


@pytest.mark.parametrize("T", vc.TIERS_T)
def test_the_ilu0_twin_of_tiers_has_its_lanes_both_paths_and_updates_that_matter(T):
    M = vc.tiers_ilu0(T, W)
    nA = vc.KNOBS_ILU0[T][0]
    assert M.facts(LOWER, UNIT)["widths"].tolist() == [nA, vc.N_B, W + 7]
    assert vr.wide_lanes_ilu0(M) == T and M.nnz <= 50000
    assert set(vc.special_lengths(T)) <= set(np.diff(M.csr[0])[nA + vc.N_B:].tolist())
    assert {("wide", T, "regs"), ("wide", T, "mem")} <= vr.reach_ilu0(M, W)
    hit = vr.updates_off_the_diagonal(M)[nA + vc.N_B:] > 0
    assert 4 * int(hit.sum()) >= W + 7, "a quarter of the last level's rows or more take an update off their diagonal"
    F = im.factor(M)
    assert int((F.csr[2] != M.csr[2]).sum()) >= W + 7


@pytest.mark.parametrize("T", vc.CHAIN_TAIL_T)
def test_chain_tail_gives_long_rows_to_groups_of_32_and_64_lanes(T):
    M = vc.chain_tail(T, W)
    widths = M.facts(LOWER, STORED)["widths"].tolist()
    assert widths[1:] == list(vc.CHAIN_TAIL_WIDTHS[T]) and all(vr.chain_lanes(x) == T for x in widths[1:]) and widths[0] > W
    assert (trsv.launches(widths, W), trsv.chains(widths, W)) == (2, 1)
    lengths = np.diff(M.csr[0])[widths[0]:].tolist()
    assert set(lengths) == set(vc.chain_tail_lengths(T)) and 8 * T + 1 in lengths and M.nnz <= 50000
    assert sorted({-(-n // (4 * T)) for n in lengths}) == [1, 2, 3, 4, 5, 7]
    assert {("chain", T, p) for p in vr.PASSES} <= vr.reach_trsv(M, LOWER, W)


@pytest.mark.parametrize("w", (W, 2 * W, 4 * W))
@pytest.mark.parametrize("T", vc.HANDED_T)
def test_handed_has_the_rows_and_levels_the_hand_off_is_tested_on(T, w):
    M = vc.handed(T, w)
    widths = M.facts(LOWER, UNIT)["widths"].tolist()
    assert all(vr.chain_lanes(x) == T for x in widths[1:]) and widths[0] > w and M.nnz <= 50000
    assert (trsv.launches(widths, w), trsv.chains(widths, w)) == (2, 1)
    if T == 1:
        assert widths[1] == w - 3, "as many rows as a chain's level may hold, less three: %d a lane" % (w // 256)
    sm.ilu0_check(M.n, M.csr[0], M.csr[1])                                           # ascending columns, a diagonal each: accepted
    r, c, _ = M.entries()
    assert (c > r).sum() > 5 * (c < r).sum(), "few pivots, long upper parts"
    lengths = np.diff(M.csr[0])
    order, level_ptr = M.facts(LOWER, UNIT)["order"], M.facts(LOWER, UNIT)["level_ptr"]
    one = set(lengths[order[level_ptr[1]:level_ptr[2]]].tolist())
    assert 64 * T in one and 64 * T + 1 in one and 8 * T + 1 in one and any(n > 512 for n in one) and any(n > 1024 + 512 for n in one)
    assert T > 4 or any(64 * T < n <= 512 for n in one)
    reach = vr.reach_ilu0(M, w)
    assert {("chain", T, "regs"), ("chain", T, "mem"), ("handed", T, "mem")} <= reach and (T > 4 or ("handed", T, "regs") in reach)
    (_, w1, p1), (_, w2, p2), (_, w3, p3), (_, w4, p4) = vr.handed_places(M, w)
    assert len(p2) >= 6, "the deal wraps round the four wavefronts"
    assert p3 == list(range(w3)), "a level of long rows only"
    assert p4 == [w4 - 1] and w4 - 1 >= 64 // T, "the lone long row, dealt to wavefront 0, stands in a later wavefront's group"
    if T <= 2:
        assert w1 > 64 and min(p1) >= 64 and max(p2) >= 64, "found in a second ballot round"
    hit = vr.updates_off_the_diagonal(M)[vc.HEAD:vc.HEAD + sum(widths[1:])] > 0
    assert hit.all(), "every thin row's first pivot updates a position off the diagonal"


# ------------------------------------------------------------------------------------------------------ the new cases' references
@pytest.mark.parametrize("i", range(len(TRSV_CASES)))
def test_the_trsv_references_are_finite_and_within_highams_bound(i):
    """test_trsv_host.py's bound, derived there: |b - T x^|_i <= gamma_(k_i + 2) (|T| |x^|)_i, the residual exact in fractions."""
    M = TRSV_CASES[i]
    row_ptr, col_ind, val = (a.tolist() for a in M.csr)
    for uplo, diag in BOTH:
        b, x = M.reference(uplo, diag)
        assert np.isfinite(x).all() and np.abs(x).max() <= 2.0 * np.abs(b).max()
        xf = [Fraction(t) for t in x.tolist()]
        for r in range(M.n):
            tx, scale, k = Fraction(0), Fraction(0), 0
            for p in range(row_ptr[r], row_ptr[r + 1]):
                c = col_ind[p]
                if (c == r and diag == STORED) or ((c < r) if uplo == LOWER else (c > r)):
                    t = Fraction(val[p]) * xf[c]
                    tx += t
                    scale += abs(t)
                    k += 1
            if diag == UNIT:
                tx += xf[r]
                scale += abs(xf[r])
                k += 1
            assert abs(Fraction(float(b[r])) - tx) <= gamma(k + 2) * scale, "%s, uplo %d, diag %d, row %d of %d entries" % (
                M.name, uplo, diag, r, k)


ALL_ILU0 = ILU0_CASES + tuple(vc.handed(T, w) for w in (2 * W, 4 * W) for T in vc.HANDED_T)


@pytest.mark.parametrize("i", range(len(ALL_ILU0)))
def test_the_ilu0_references_are_finite_and_the_host_loops_bit_for_bit(i):
    M = ALL_ILU0[i]
    F = im.factor(M)
    assert np.isfinite(F.csr[2]).all()
    assert_bits(sm.ilu0_host(M.n, *M.csr), F.csr[2], M.name)
    b = trsv.rhs(M.n)
    y = trsv.solve(F, LOWER, UNIT, b)                                                # what the GPU test solves with: finite
    assert np.isfinite(trsv.solve(F, UPPER, STORED, y)).all()


# ------------------------------------------------------------------------------------------------------------------ the coverage
def old_reach_trsv():
    out = set()
    for M in trsv.existing_cases() + trsv.constructed_cases(W):
        for uplo in (LOWER, UPPER):
            out |= vr.reach_trsv(M, uplo, W)
    return out


def old_reach_ilu0():
    out = set()
    for i in range(im.N_CONSTRUCTED + im.N_MORE):
        out |= vr.reach_ilu0(im.case(W, i), W)
    return out


def test_old_and_new_cases_together_reach_every_required_cell():
    got = old_reach_trsv()
    for M in TRSV_CASES:
        for uplo in (LOWER, UPPER):
            got |= vr.reach_trsv(M, uplo, W)
    assert not vr.REQUIRED_TRSV - got, sorted(vr.REQUIRED_TRSV - got, key=str)
    got = old_reach_ilu0()
    for M in ILU0_CASES:
        got |= vr.reach_ilu0(M, W)
    assert not vr.REQUIRED_ILU0 - got, sorted(vr.REQUIRED_ILU0 - got, key=str)


# What test_gpu_trsv.py and test_gpu_ilu0.py leave out, as the rules say on their cases (existing_cases(), constructed_cases(256),
# ilu0_method.case(256, 0 .. 21)).  An equality: a case added there that fills one of these cells has to be taken out here.
OLD_MISSES_TRSV = ({("wide", 2, p) for p in ("3", "4", "5+")} | {("wide", 4, p) for p in vr.PASSES[1:]}
                   | {("wide", 8, p) for p in ("1 full", "2", "3", "4")} | {("wide", 16, p) for p in vr.PASSES[1:]}
                   | {("wide", T, p) for T in (32, 64) for p in vr.PASSES} | {("chain", T, p) for T in (32, 64) for p in ("1 full", "4", "5+")})
OLD_MISSES_ILU0 = ({("wide", T, "mem") for T in (2, 4, 8)} | {("wide", T, p) for T in (32, 64) for p in ("regs", "mem")}
                   | {("handed", T, "mem") for T in (1, 2, 8, 16, 32)} | {("handed", 4, "regs")})


def test_the_old_cases_alone_miss_exactly_these_cells():
    assert vr.REQUIRED_TRSV - old_reach_trsv() == OLD_MISSES_TRSV
    assert vr.REQUIRED_ILU0 - old_reach_ilu0() == OLD_MISSES_ILU0
    # and the hand-off's deal: only memplus hands rows over; one of its levels holds seven long rows (the deal wraps there), none
    # holds a long row at place 64 or beyond (the second ballot round), none is made of long rows only
    deals = [(im.case(W, i).name, T, width, places) for i in range(im.N_CONSTRUCTED + im.N_MORE)
             for T, width, places in vr.handed_places(im.case(W, i), W)]
    assert {name for name, _, _, _ in deals} == {"memplus"}
    assert [(T, width, places) for _, T, width, places in deals if len(places) > 4] == [(2, 71, [0, 1, 2, 3, 4, 5, 6])]
    assert max(max(places) for _, _, _, places in deals) < 64 and all(len(places) < width for _, _, width, places in deals)
