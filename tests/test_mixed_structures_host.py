"""Host checks of tests/mixed_structures.py: every structure meets the conditions that give the blocked plans something to get
wrong (assert_regime) and is the same on a second build; the int64 references are the oracle's serial loop bit for bit; and --
the point of the file -- numpy models of the wrong kernels these inputs are for (an entry dropped or counted twice at a window
end, a column-block edge, a tile's last position, the first or last copy of the repeated pair, the band's edge; x read one column
off; a block's diagonal taken at r instead of first_row + r) never give the exact reference, so test_gpu_mixed_structures.py
cannot pass on such a kernel.  On the real operands the order of a column's ties shows in the bits of A^T x."""
import numpy as np
import pytest

import adopted
import mixed_structures as ms
import oracle_binding as ob
import special_values as sv
import transposed
from transposed import same_bits


# ----------------------------------------------------------------------------------------------------------- the structures
@pytest.mark.parametrize("name", ms.NAMES)
def test_structure_meets_its_regime_and_is_deterministic(name):
    g = ms.assert_regime(name)
    print("mixed structures: %s: %r" % (name, g))
    rows, cols, row0, coo = ms.structure(name)
    again = ms._generate(name)
    assert again[:3] == (rows, cols, row0) and again[3].tobytes() == coo.tobytes()
    assert coo["row"].min() >= 0 and coo["row"].max() < rows and coo["col"].min() >= 0 and coo["col"].max() < cols
    rp, ci, v = ms.csr_of(name)
    assert rp[-1] == len(coo) and np.count_nonzero(v) == len(v)
    # csr_of keeps a row's entries in input order: the stable sort by (row, col) of it is smvp_csr_from_coo, array for array
    srp, sci, sv_ = ms.sm.csr_from_coo(coo, rows)
    order = np.lexsort((ci, sv.row_of_entries(rp)))
    assert np.array_equal(srp, rp) and np.array_equal(sci, ci[order]) and sv_.tobytes() == v[order].tobytes()
    if ms.kind_of(name) != "square":
        assert not np.array_equal(sci, ci)


@pytest.mark.parametrize("name", ms.NAMES)
def test_exact_references_are_the_serial_loop_bit_for_bit(name):
    rows, cols, row0, _ = ms.structure(name)
    coo, x, xr = ms.operands(name, "exact")
    assert np.array_equal(coo["row"], ms.structure(name)[3]["row"]) and np.array_equal(coo["col"], ms.structure(name)[3]["col"])
    assert (np.abs(coo["val"]) >= 1).all() and (np.abs(coo["val"]) <= 1024).all() and (np.abs(x) >= 1).all() and (np.abs(x) <= 2 ** 20).all()
    rp, ci, v = ms.csr_of(name, coo)
    scale = ob.csr_spmv(rp, ci, np.abs(v), np.abs(x))
    assert scale.max() < 2.0 ** 53
    ref = ms.reference(name)
    assert same_bits(ref, ob.csr_spmv(rp, ci, v, x)) and np.count_nonzero(ref) > 0.5 * np.count_nonzero(np.diff(rp))
    assert same_bits(ms.reference_t(name), transposed.reference(coo, rows, cols, xr))


# ------------------------------------------------------------------------------------------------- models of wrong kernels
def product(rp, ci, v, x, weight=None, col_shift=None):
    """The exact product with entry weights (0: dropped, 2: counted twice) and column shifts (x read `shift` columns off)."""
    v = np.asarray(v) if weight is None else np.asarray(v) * weight
    ci = np.asarray(ci) if col_shift is None else (np.asarray(ci, dtype=np.int64) + col_shift).astype(np.int32)
    return adopted.reference(rp, ci, v, x)


def one_entry_models(name, rp, ci, row0):
    """{label: entry positions}: one wrong kernel per position, where the structure has such an entry."""
    rows, cols = ms.KINDS[ms.kind_of(name)][:2]
    row_of = sv.row_of_entries(rp)
    c = ci.astype(np.int64)
    d = c - (row0 + row_of)
    out = {}
    for b, (wb, we) in enumerate(ms.windows(rows, cols, row0)):
        in_block = (row_of // ms.K6_ROWS == b) & (np.abs(d) <= ms.K6_BAND)
        for label, col in (("first column of window %d" % b, wb), ("last column of window %d" % b, we - 1)):
            hit = np.flatnonzero(in_block & (c == col))
            if 0 <= col < cols and len(hit):
                out[label] = hit[:1]
    for col in (sv.BIN_COL_BLOCK - 1, sv.BIN_COL_BLOCK):
        out["column %d, near" % col] = np.flatnonzero((c == col) & (np.abs(d) <= ms.K6_BAND))[:1]
        out["column %d, far" % col] = np.flatnonzero((c == col) & (np.abs(d) > ms.K6_BAND))[:1]
    for tile in (256, 1024, 2048):
        out["last entry of tile 0 (%d)" % tile] = np.array([tile - 1])
        out["last entry of a middle tile (%d)" % tile] = np.array([(len(ci) // (2 * tile)) * tile + tile - 1])
        out["first entry of the last tile (%d)" % tile] = np.array([(len(ci) - 1) // tile * tile])
    out["last entry"] = np.array([len(ci) - 1])
    for off in ms.EDGE_OFFSETS:
        out["offset %d" % off] = np.flatnonzero(d == off)[:1]
    if ms.kind_of(name) != "square":
        flat = row_of * cols + c
        values, counts = np.unique(flat, return_counts=True)
        copies = np.flatnonzero(flat == values[np.argmax(counts)])
        assert len(copies) == rows + ms.PAIR_EXTRA
        out["first copy of the repeated pair"], out["last copy of the repeated pair"] = copies[:1], copies[-1:]
        twice = np.flatnonzero(flat == values[np.flatnonzero(counts == 2)[0]])
        out["first of two copies"], out["second of two copies"] = twice[:1], twice[1:]
    return {k: p for k, p in out.items() if len(p)}


@pytest.mark.parametrize("name", ms.NAMES)
def test_the_exact_reference_rejects_the_wrong_kernels(name):
    rows, cols, row0, _ = ms.structure(name)
    coo, x, _ = ms.operands(name, "exact")
    rp, ci, v = ms.csr_of(name, coo)
    ref = ms.reference(name)
    models = one_entry_models(name, rp, ci, row0)
    kind = ms.kind_of(name)
    wanted = {"last entry", "column 16383, far", "column 16384, far", "last entry of tile 0 (1024)"}
    if kind != "block_off":
        wanted |= {"offset %d" % off for off in ms.EDGE_OFFSETS} | {"last column of window 0"}
        wanted |= {"first column of window 1"}
    if kind in ("square", "repeats", "tall"):                           # (rows whose diagonal lies within 4096 of column 16383)
        wanted |= {"column 16383, near"}
    if kind != "square":
        wanted |= {"first copy of the repeated pair", "last copy of the repeated pair", "second of two copies"}
    assert wanted <= set(models), (name, sorted(wanted - set(models)))
    checked = 0
    for label, pos in models.items():
        for what, w in (("dropped", 0), ("counted twice", 2)):
            weight = np.ones(len(ci), dtype=np.int64)
            weight[pos] = w
            bad = product(rp, ci, v, x, weight=weight)
            assert not same_bits(bad, ref), "%s: %s %s goes unnoticed" % (name, label, what)
            assert (bad != ref).sum() == 1
            checked += 1
        for shift in (-1, 1):                                           # x read one column off for this entry
            if 0 <= ci[pos[0]] + shift < cols:
                s = np.zeros(len(ci), dtype=np.int64)
                s[pos] = shift
                assert not same_bits(product(rp, ci, v, x, col_shift=s), ref), "%s: %s read %+d column off goes unnoticed" % (name, label, shift)
                checked += 1
    # the band's edge taken on the wrong side by one of the two parts of a split product
    near, row_of = ms.near_mask(rows, row0, rp, ci)
    d = np.abs(ci.astype(np.int64) - (row0 + row_of))
    if kind != "block_off":
        for what, weight in (("4096 from the diagonal in neither part", (d != ms.K6_BAND)), ("4096 in both parts", 1 + (d == ms.K6_BAND)),
                             ("4097 in both parts", 1 + (d == ms.K6_BAND + 1))):
            bad = product(rp, ci, v, x, weight=np.asarray(weight, dtype=np.int64))
            assert (bad != ref).sum() >= 50, "%s: %s" % (name, what)
            checked += 1
    print("mixed structures: %s: %d wrong kernels rejected" % (name, checked))


@pytest.mark.parametrize("name", [n for n in ms.BLOCKS if ms.kind_of(n) != "block_off"])
def test_a_block_whose_diagonal_is_taken_at_the_local_row_is_rejected(name):
    """K6 with row0 = 0 on a block: the near entries (by the true diagonal) that fall outside the window [R0 - 4096, R0 + 8192 +
    4096) of the LOCAL rows are left out."""
    rows, cols, row0, _ = ms.structure(name)
    coo, x, _ = ms.operands(name, "exact")
    rp, ci, v = ms.csr_of(name, coo)
    near, row_of = ms.near_mask(rows, row0, rp, ci)
    r0 = row_of // ms.K6_ROWS * ms.K6_ROWS
    in_misplaced = (ci >= r0 - ms.K6_BAND) & (ci < r0 + ms.K6_ROWS + ms.K6_BAND)
    lost = near & ~in_misplaced
    assert lost.sum() >= 100
    bad = product(rp, ci, v, x, weight=(~lost).astype(np.int64))
    assert (bad != ms.reference(name)).sum() >= 20
    # and the split by the local diagonal alone moves the far share, which the GPU test compares with the host's count
    far_local = float((np.abs(ci.astype(np.int64) - row_of) > ms.K6_BAND).mean())
    assert abs(far_local - ms.regime(name)["far_share"]) > 0.01


# ------------------------------------------------------------------------------------------------------ the order of ties
@pytest.mark.parametrize("name", [n for n in ms.WHOLE if ms.kind_of(n) == "repeats"])
def test_the_order_of_a_columns_ties_shows_in_the_bits(name):
    """A^T x with the ties of every column summed in the reverse of storage order (the entry list reversed: the sort by (column,
    row) is the same, the ties' order is not) differs in bits -- so the bit checks of K8, K9 and the transposed handle see it."""
    rows, cols, row0, _ = ms.structure(name)
    coo, _, xr = ms.operands(name, "real")
    ref = transposed.reference(coo, rows, cols, xr)
    rev = transposed.reference(coo[::-1].copy(), rows, cols, xr)
    differs = int((ref.view(np.int64) != rev.view(np.int64)).sum())
    print("mixed structures: %s: %d columns of A^T x change bits with the order of ties" % (name, differs))
    assert differs >= 10
    rp, ci, v = ms.csr_of(name, coo)                                    # the same for the rows of A x
    rrp, rci, rv = ms.csr_of(name, coo[::-1].copy())
    x = ms.operands(name, "real")[1]
    assert (ob.csr_spmv(rp, ci, v, x).view(np.int64) != ob.csr_spmv(rrp, rci, rv, x).view(np.int64)).sum() >= 10


# ---------------------------------------------------------------------------------------------------------- the converter
@pytest.mark.parametrize("name", [n for n in ms.WHOLE if ms.kind_of(n) == "repeats"])
def test_host_converter_refuses_a_start_pos_too_short_for_the_repeats(name):
    """start_pos_capacity = rows + 1 suffices only when no pair repeats: SMVP_ERR_INVALID, nothing written around start_pos."""
    import ctypes as C

    sm = ms.sm
    rows, cols, _, coo = ms.structure(name)
    nnz, cap, g, guard = len(coo), rows + 1, 64, 0x5A17C0DE
    assert ms.regime(name)["num_diag"] + 1 > cap
    nd = C.c_int(-1)
    perm, ri, val = np.zeros(cols, np.int32), np.zeros(nnz, np.int32), np.zeros(nnz)
    sp = np.full(cap + 2 * g, guard, dtype=np.int32)
    rc = sm.lib().smvp_tjds_from_coo(sm._p(coo), rows, cols, nnz, sm._p(perm), C.c_void_p(sp.ctypes.data + 4 * g), cap, sm._p(ri), sm._p(val),
                                     C.byref(nd), None, None)
    assert rc == sm.ERR_INVALID and (sp[:g] == guard).all() and (sp[g + cap:] == guard).all()
    t = sm.tjds_from_coo(coo, rows, cols)                               # (capacity max(rows, nnz) + 2)
    assert t.num_diag == np.bincount(coo["col"]).max() == ms.regime(name)["num_diag"] > rows
    assert t.start_pos[0] == 0 and t.start_pos[-1] == nnz and (np.diff(t.start_pos) >= 1).all()
