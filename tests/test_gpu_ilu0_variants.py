"""GPU: every lanes-per-row variant of K17 (ilu0_level_rows<2 .. 64> on both of its paths) and ilu0_chain's hand-off of a long row
to a whole wavefront from a level of every width class, against the restatement tests/ilu0_method.py, on the cases of
tests/variant_cases.py that were built to run them.

No tolerance anywhere: every element of F is the serial loop's bits, after create and after factor() over NaNs; then one solve with
each of F's two plans against trsv_method.solve on the restated factor -- K15 at these widths on K17's patterns.  Which variant a
case runs is restated in tests/variant_reach.py from the library's constants; every test here pins them (lanes_per_row and
chain_width as smvp_ilu0_info reports them) and builds its case from the reported chain width."""
import pytest

import ilu0_method as im
import smvp_toolkit_amd as sm
import trsv_method as trsv
import variant_cases as vc
import variant_reach as vr
from test_gpu_ilu0 import chain_width, handle_of, solve_once, values_of, values_tensor
from transposed import assert_bits
from trsv_method import LOWER, STORED, UNIT, UPPER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def check_factor(torch, M, w, T, counts, cells, option=None):
    """Create (under trsv_chain_width = option, if given), the factor's bits, factor() again over NaNs, info against the
    restatement, and a solve with each of F's plans."""
    want = im.factor(M)
    H = handle_of(M)
    if option is None:
        f = H.ilu0()
    else:
        with sm.option("trsv_chain_width", option):
            f = H.ilu0()
    assert_bits(values_of(torch, f), want.csr[2], M.name + ": after create")
    info, facts = f.info(), M.facts(LOWER, UNIT)
    assert info["chain_width"] == w, "%s: built for a chain width of %d, the factorisation reports %d" % (M.name, w, info["chain_width"])
    assert info["lanes_per_row"] == vr.wide_lanes_ilu0(M), "%s: %d lanes a row, the restated rule says %d" % (
        M.name, info["lanes_per_row"], vr.wide_lanes_ilu0(M))
    assert T is None or info["lanes_per_row"] == T, "%s: %d lanes a row, built for %d" % (M.name, info["lanes_per_row"], T)
    assert (info["launches"], info["chains"]) == counts == (trsv.launches(facts["widths"], w), trsv.chains(facts["widths"], w)), M.name
    assert (info["levels"], info["max_level_width"], info["entries"], info["pivots"]) == (
        facts["levels"], facts["max_level_width"], M.nnz, facts["off"]), M.name
    assert cells <= vr.reach_ilu0(M, w), "%s: not reached: %r" % (M.name, sorted(cells - vr.reach_ilu0(M, w)))
    values_tensor(torch, f).fill_(float("nan"))
    assert f.factor() is f
    assert_bits(values_of(torch, f), want.csr[2], M.name + ": factor() again, over NaNs")
    L, U = f.plans()
    b = trsv.rhs(M.n, 19)
    y = trsv.solve(want, LOWER, UNIT, b)
    assert_bits(solve_once(torch, L, M.n, b), y, M.name + ": F's LOWER / UNIT plan")
    assert_bits(solve_once(torch, U, M.n, y), trsv.solve(want, UPPER, STORED, y), M.name + ": F's UPPER / STORED plan")
    for X in (L, U, f, H):
        X.close()


@pytest.mark.parametrize("T", vc.TIERS_T)
def test_every_wide_variant_on_its_register_and_its_memory_path(torch, T):
    """The symmetrised twin of tiers(T): ilu0_level_rows<T> on rows of up to 8 T entries (registers) and beyond (w kept in F),
    every row of the last level updated at a position other lanes own."""
    w = chain_width()
    check_factor(torch, vc.tiers_ilu0(T, w), w, T, (3, 1), {("wide", T, "regs"), ("wide", T, "mem")})


def handed_cells(T):
    return {("chain", T, "regs"), ("chain", T, "mem"), ("handed", T, "mem")} | ({("handed", T, "regs")} if T <= 4 else set())


@pytest.mark.parametrize("T", vc.HANDED_T)
def test_long_rows_of_a_chains_level_are_handed_to_a_wavefront(torch, T):
    """handed(T): levels whose rows get T lanes, with rows of 64 T entries (kept) and 64 T + 1 (handed over), handed rows on the
    register path (T <= 4) and the memory path, seven long rows in a level, a level of long rows only, a lone long row."""
    w = chain_width()
    check_factor(torch, vc.handed(T, w), w, None, (2, 1), handed_cells(T))


@pytest.mark.parametrize("times", (2, 4))
@pytest.mark.parametrize("T", vc.HANDED_T)
def test_the_hand_off_under_the_wider_chain_options(torch, T, times):
    """The same at trsv_chain_width = 512 and 1024: handed(1)'s first thin level then holds 2 or 4 rows a lane; for T >= 2 the
    matrix is the one of the default width and the bits are unchanged."""
    w = times * chain_width()
    M = vc.handed(T, w)
    if T > 1:
        assert_bits(M.csr[2], vc.handed(T, chain_width()).csr[2], "the same matrix")
    check_factor(torch, M, w, None, (2, 1), handed_cells(T), option=w)
