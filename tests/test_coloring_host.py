"""Host checks of the multicolour ordering (K23): tests/coloring_method.py, the restatement, against hand-computed values, and the
library's smvp_csr_color_host against the restatement, colour for colour.  Then what follows from the definition: the bound on the
number of colours, no colour unused, a proper colouring wherever N is symmetric, and at most `colors` levels in both triangles of
the matrix renumbered colour by colour -- the reason the reordering exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coloring_method as cm
import smvp_toolkit_amd as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mix32_is_pinned_to_hand_computed_words():
    # by hand: 0 stays 0 through every line.  1: the first line leaves 1, the second makes 0x7feb352d, the third folds in
    # 0x7feb352d >> 15 = 0xffd6 -> 0x7febcafb; the last two lines in exact integer arithmetic
    assert cm.mix32(0) == 0
    x = 0x7feb352d ^ 0xffd6
    assert x == 0x7febcafb
    y = (x * 0x846ca68b) % 2 ** 32
    assert cm.mix32(1) == y ^ (y >> 16) == 0x688990c0
    assert [cm.mix32(v) for v in (2, 0x12345678, 0xffffffff)] == [0xd1132181, 0xf5e71c96, 0x6768824a]
    assert cm.keys(1000, 12345).tolist() == [cm.mix32(v ^ 12345) for v in range(1000)]
    assert len(set(cm.keys(100000, 0xffffffff).tolist())) == 100000
    # the library's: a lone vertex pair (0 -> 1 and back) is coloured by the order of the two keys
    rp, ci = np.array([0, 1, 2], np.int32), np.array([1, 0], np.int32)
    for seed in (0, 1, 2, 0x12345678, 0xffffffff):
        col = sm.color_host(2, rp, ci, seed=seed)[0].tolist()
        assert col == ([1, 0] if cm.mix32(1 ^ seed) > cm.mix32(0 ^ seed) else [0, 1])


def test_the_restatement_on_cases_worked_by_hand():
    # a path of three: whatever the keys, the middle vertex differs from both ends, two colours, and depth <= 3
    P = cm.path(3)
    for seed in cm.SEEDS:
        col, colors, depth = cm.color(P.n, P.csr[0], P.csr[1], seed=seed)
        key = cm.keys(3, seed).tolist()
        top = int(np.argmax(key))
        assert col[top] == 0 and colors == 2 and col[1] != col[0] and col[1] != col[2]
        want_depth = 3 if (key[0] > key[1] > key[2] or key[2] > key[1] > key[0]) else 2
        assert depth == want_depth
    # a triangle: the colours are the ranks by descending key
    T = cm.complete(3)
    key = cm.keys(3, 7).tolist()
    col, colors, depth = cm.color(3, T.csr[0], T.csr[1], seed=7)
    assert col.tolist() == [sorted(key, reverse=True).index(k) for k in key] and colors == depth == 3
    # (0 -> 1) stored in one direction only: without the transposed pattern vertex 1 does not see vertex 0
    rp, ci = np.array([0, 1, 1], np.int32), np.array([1], np.int32)
    for seed in cm.SEEDS:
        key = cm.keys(2, seed).tolist()
        col, colors, _ = cm.color(2, rp, ci, seed=seed)
        assert col.tolist() == ([1, 0] if key[1] > key[0] else [0, 0])
        trp, tci = cm.transposed_pattern(2, rp, ci)
        assert (trp.tolist(), tci.tolist()) == ([0, 0, 1], [0])
        col, colors, _ = cm.color(2, rp, ci, trp, tci, seed)
        assert sorted(col.tolist()) == [0, 1] and colors == 2


def host(P, at, seed):
    t = P.transposed() if at else (None, None)
    return sm.color_host(P.n, P.csr[0], P.csr[1], t[0], t[1], seed)


def held_to_the_restatement(P, at, seed, symmetric):
    col, colors, depth = host(P, at, seed)
    want = P.reference(at, seed)
    what = "%s, %s the transposed pattern, seed %#x" % (P.name, "with" if at else "without", seed)
    assert (col == want[0]).all() and (colors, depth) == want[1:], what
    t = P.transposed() if at else (None, None)
    assert colors <= 1 + cm.max_degree(P.n, P.csr[0], P.csr[1], *t), what
    assert (np.bincount(col, minlength=colors) > 0).all() and (colors == 0 or col.max() == colors - 1), what + ": a colour is unused"
    if symmetric or at:
        assert cm.proper(P.n, P.csr[0], P.csr[1], col), what + ": not proper"
        lower, upper = cm.levels_after(P.n, P.csr[0], P.csr[1], col, colors)
        assert lower <= colors and upper <= colors, "%s: %d / %d levels with %d colours" % (what, lower, upper, colors)
    return col, colors, depth


@pytest.mark.parametrize("seed", cm.SEEDS)
def test_the_host_loop_is_the_restatement_on_the_constructed_cases(seed):
    for P, symmetric in cm.small_cases():
        assert cm.symmetric(P.n, P.csr[0], P.csr[1]) == symmetric, P.name
        for at in (False, True):
            col, colors, depth = held_to_the_restatement(P, at, seed, symmetric)
            if P.name.startswith("diagonal"):
                assert colors == 1 and depth == 1 and not col.any()
            if P.name.startswith("K"):
                assert colors == depth == P.n                     # 65 and 129: the mask's window boundaries
            if P.name.startswith("star"):
                assert colors == 2
            if P.name.startswith(("path", "ring")):
                assert 2 <= colors <= 3
    assert sm.color_host(0, np.zeros(1, np.int32), np.zeros(0, np.int32), seed=seed)[1:] == (0, 0)


@pytest.mark.parametrize("name", cm.SAMPLES)
def test_the_host_loop_is_the_restatement_on_the_samples(name):
    P = cm.sample(name)
    symmetric = cm.symmetric(P.n, P.csr[0], P.csr[1])
    for seed in cm.SEEDS:
        for at in (False, True):
            col, colors, depth = held_to_the_restatement(P, at, seed, symmetric)
            print("%-8s %s at, seed %#10x: %3d colours, depth %3d" % (name, "with" if at else "no  ", seed, colors, depth))


def test_lap2d_gets_four_or_five_colours_and_as_many_levels():
    P = cm.lap2d(32)
    assert sm.trsv_levels(P.n, P.csr[0], P.csr[1], sm.TRSV_LOWER)[1] == 63
    for seed in cm.SEEDS:
        col, colors, _ = host(P, False, seed)
        assert 4 <= colors <= 5                                   # (degree 4: at most 5; the grid is bipartite, the greedy rule is not optimal)
        assert max(cm.levels_after(P.n, P.csr[0], P.csr[1], col, colors)) <= colors


def test_pwt_stores_one_triangle_so_its_colouring_without_the_transpose_is_not_proper():
    P = cm.sample("pwt")
    assert not cm.symmetric(P.n, P.csr[0], P.csr[1])
    for seed in cm.SEEDS:
        col, colors, _ = host(P, False, seed)
        assert (col == P.reference(False, seed)[0]).all()
        assert not cm.proper(P.n, P.csr[0], P.csr[1], col)
        lower, upper = cm.levels_after(P.n, P.csr[0], P.csr[1], col, colors)
        print("pwt without at, seed %#x: %d colours, %d / %d levels" % (seed, colors, lower, upper))
        col, colors, _ = host(P, True, seed)
        assert cm.proper(P.n, P.csr[0], P.csr[1], col)


def test_the_permutation_and_the_permuted_arrays():
    P = cm.messy()
    col, colors, _ = host(P, True, 0)
    old_of_new, new_of_old, class_ptr = cm.perm_from_classes(col, colors)
    assert (new_of_old[old_of_new] == np.arange(P.n)).all() and (np.diff(col[old_of_new]) >= 0).all()
    for c in range(colors):
        block = old_of_new[class_ptr[c]:class_ptr[c + 1]]
        assert (col[block] == c).all() and (np.diff(block) > 0).all()
    rp, ci, v = cm.permuted_csr(P.n, *P.csr, new_of_old)
    dense = np.zeros((P.n, P.n))
    r = np.repeat(np.arange(P.n), np.diff(P.csr[0]))
    np.add.at(dense, (new_of_old[r], new_of_old[P.csr[1]]), P.csr[2])
    back = np.zeros((P.n, P.n))
    rb = np.repeat(np.arange(P.n), np.diff(rp))
    np.add.at(back, (rb, ci), v)
    assert (np.diff(ci)[np.diff(rb) == 0] >= 0).all()              # ascending columns inside every row
    # (sums of repeats in another order may differ in the last bit: the structure and the multiset of values are what is exact)
    assert ((dense != 0) == (back != 0)).all() and np.allclose(dense, back, rtol=1e-15, atol=0)
    L = cm.lap2d(32)
    rp, ci, v = cm.permuted_csr(L.n, *L.csr, np.arange(L.n, dtype=np.int32))
    assert (rp == L.csr[0]).all() and (ci == L.csr[1]).all() and v.tobytes() == L.csr[2].tobytes()


def refused(*args):
    color = np.full(8, -7, dtype=np.int32)
    colors, depth = C.c_int(-7), C.c_int(-7)
    full = list(args) + [sm._p(color), C.byref(colors), C.byref(depth)]
    rc = sm.lib().smvp_csr_color_host(*full)
    assert (color == -7).all() and colors.value == depth.value == -7, "a refused call wrote its outputs"
    return rc


def test_every_argument_error_of_the_host_call():
    rp, ci = np.array([0, 2, 3, 4], np.int32), np.array([0, 1, 0, 2], np.int32)
    p = sm._p
    ok = np.zeros(3, np.int32)
    colors, depth = C.c_int(), C.c_int()
    L = sm.lib()
    assert L.smvp_csr_color_host(3, p(rp), p(ci), None, None, 0, p(ok), C.byref(colors), C.byref(depth)) == sm.OK
    assert refused(-1, p(rp), p(ci), None, None, 0) == sm.ERR_INVALID and b"rows" in L.smvp_last_error()
    assert refused(3, None, p(ci), None, None, 0) == sm.ERR_INVALID and b"row_ptr" in L.smvp_last_error()
    assert refused(3, p(rp), None, None, None, 0) == sm.ERR_INVALID and b"col_ind" in L.smvp_last_error()
    assert refused(3, p(rp), p(ci), p(rp), None, 0) == sm.ERR_INVALID and b"both" in L.smvp_last_error()
    assert refused(3, p(rp), p(ci), None, p(ci), 0) == sm.ERR_INVALID and b"both" in L.smvp_last_error()
    for bad_rp in ([1, 2, 3, 4], [0, 3, 2, 4]):
        b = np.array(bad_rp, np.int32)
        assert refused(3, p(b), p(ci), None, None, 0) == sm.ERR_INVALID and b"row_ptr" in L.smvp_last_error()
        assert refused(3, p(rp), p(ci), p(b), p(ci), 0) == sm.ERR_INVALID and b"t_row_ptr" in L.smvp_last_error()
    for bad in (3, -1):
        b = np.array([0, 1, bad, 2], np.int32)
        assert refused(3, p(rp), p(b), None, None, 0) == sm.ERR_INVALID and b"col_ind[2]" in L.smvp_last_error()
        assert refused(3, p(rp), p(ci), p(rp), p(b), 0) == sm.ERR_INVALID and b"t_col_ind[2]" in L.smvp_last_error()
    assert L.smvp_csr_color_host(3, p(rp), p(ci), None, None, 0, None, C.byref(colors), C.byref(depth)) == sm.ERR_INVALID
    assert L.smvp_csr_color_host(3, p(rp), p(ci), None, None, 0, p(ok), None, C.byref(depth)) == sm.ERR_INVALID
    assert L.smvp_csr_color_host(3, p(rp), p(ci), None, None, 0, p(ok), C.byref(colors), None) == sm.ERR_INVALID
    assert L.smvp_csr_color_host(0, None, None, None, None, 5, None, C.byref(colors), C.byref(depth)) == sm.OK
    assert (colors.value, depth.value) == (0, 0)


def test_the_defaults_the_struct_layouts_and_the_declarations():
    o = sm.ColorOpts()
    sm.lib().smvp_color_opts_default(C.byref(o))
    sm.lib().smvp_color_opts_default(None)
    assert (o.struct_size, o.seed, o.max_rounds) == (C.sizeof(sm.ColorOpts), 0, 4096) and C.sizeof(sm.ColorOpts) == 12
    assert C.sizeof(sm.ColorInfo) == 40 and sm.ColorInfo.entries.offset == 24 and sm.ColorInfo.build_ms.offset == 32
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "smvp_amd.h")).read(), flags=re.S)
    for name in ("smvp_color_opts_default", "smvp_csr_color", "smvp_csr_color_host", "smvp_perm_from_classes", "smvp_csr_create_permuted",
                 "smvp_vector_gather"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in sm.EXPORTS and getattr(sm.lib(), name)
