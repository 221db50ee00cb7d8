"""GPU: every lanes-per-row variant of K15 (trsv_level_rows<2 .. 64>, and trsv_chain's groups of 32 and 64 lanes on rows of up to
seven passes) against the restatement tests/trsv_method.py, on the cases of tests/variant_cases.py that were built to run them.

No tolerance anywhere: every x_i is the serial substitution loop's bits (test_gpu_trsv.py's check_plan, with its calls again, on a
stream and in place).  Which variant a case runs is restated in tests/variant_reach.py from the library's constants; every test
here pins them -- lanes_per_row and chain_width as smvp_trsv_info reports them must be the restatement's -- and builds its case
from the reported chain width, so a drift in the library fails here instead of moving a case to another variant unseen."""
import pytest

import smvp_toolkit_amd as sm
import trsv_method as tm
import variant_cases as vc
import variant_reach as vr
from test_gpu_trsv import BOTH, chain_width, check_plan, handle_of
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check_case(torch, M, shaped, T, counts, cells):
    """check_plan on both triangles and both diag settings; on the triangle that holds the constructed schedule (`shaped`) the wide
    lanes are T (None: whatever the rule says), the launches and chains are `counts` and the restated reach holds `cells`."""
    w = chain_width()
    H = handle_of(M)
    for uplo, diag in BOTH:
        info, f = check_plan(torch, H, M, uplo, diag), M.facts(uplo, diag)
        assert info["chain_width"] == w, "%s: built for a chain width of %d, the plan reports %d" % (M.name, w, info["chain_width"])
        assert info["lanes_per_row"] == vr.wide_lanes_trsv(M, uplo), "%s, uplo %d: %d lanes a row, the restated rule says %d" % (
            M.name, uplo, info["lanes_per_row"], vr.wide_lanes_trsv(M, uplo))
        if uplo == shaped:
            assert T is None or info["lanes_per_row"] == T, "%s: %d lanes a row, built for %d" % (M.name, info["lanes_per_row"], T)
            assert (info["launches"], info["chains"]) == counts == (tm.launches(f["widths"], w), tm.chains(f["widths"], w)), M.name
            assert cells <= vr.reach_trsv(M, uplo, w), "%s: not reached: %r" % (M.name, sorted(cells - vr.reach_trsv(M, uplo, w)))
        else:
            assert (info["levels"], info["launches"], info["chains"]) == (1, 1, 0), "the other triangle: the diagonal, one wide level"
    H.close()


@pytest.mark.parametrize("T", vc.TIERS_T)
def test_every_wide_variant_on_rows_of_one_to_six_passes(torch, T):
    """tiers(T): trsv_level_rows<T> on rows of 2 and 3 entries and of both sides of 4 T, 8 T, 12 T, 16 T and 20 T."""
    M = vc.tiers(T, chain_width())
    check_case(torch, M, LOWER, T, (3, 1), {("wide", T, p) for p in vr.PASSES})


@pytest.mark.parametrize("T", vc.TIERS_T)
def test_every_wide_variant_on_the_upper_triangle(torch, T):
    M = vc.tiers_flipped(T, chain_width())
    check_case(torch, M, UPPER, T, (3, 1), {("wide", T, p) for p in vr.PASSES})


@pytest.mark.parametrize("T", vc.CHAIN_TAIL_T)
def test_a_chains_widest_groups_on_rows_of_up_to_seven_passes(torch, T):
    """chain_tail(T): trsv_chain's thin levels with 32 or 64 lanes a row; further passes take a second and a third turn."""
    M = vc.chain_tail(T, chain_width())
    check_case(torch, M, LOWER, None, (2, 1), {("chain", T, p) for p in vr.PASSES})


def test_a_lone_lane_walks_rows_of_1281_entries_under_the_wider_chain_option(torch):
    """tiers(64) once more with trsv_chain_width = 512: its last level of 263 rows is now a chain's, two rows to some lanes, a lane
    walks each row alone -- 1281 entries 32 at a time.  Two launches instead of three; no bit changes."""
    w = chain_width()
    M = vc.tiers(64, w)
    H = handle_of(M)
    for diag in (STORED, UNIT):
        with sm.option("trsv_chain_width", 2 * w):
            info = check_plan(torch, H, M, LOWER, diag, calls=("alias",))
        widths = M.facts(LOWER, diag)["widths"]
        assert info["chain_width"] == 2 * w and widths[2] > w
        assert info["lanes_per_row"] == vr.wide_lanes_trsv(M, LOWER) == 64, "the first level is still a launch of trsv_level_rows<64>"
        assert (info["launches"], info["chains"]) == (2, 1) == (tm.launches(widths, 2 * w), tm.chains(widths, 2 * w))
        assert {("chain", 1, "<=8"), ("chain", 1, ">8")} <= vr.reach_trsv(M, LOWER, 2 * w)
    H.close()
