"""Host checks of tests/adopted.py: the structure `mixed` meets the conditions that give every plan something to get wrong, the
int64 references are the oracle's serial loop bit for bit, and -- the point of the file -- a product made with stale entries
(the old values or columns in half of the matrix, in the tile-overflow positions, in one single tile) never has the bits of the
reference of the new arrays, so test_gpu_adopted.py cannot pass on a stale copy."""
import numpy as np
import pytest

import adopted as ad
import oracle_binding as ob
import parity
import transposed

M = ad.mixed()
COLUMN_ARRAYS = ("cols_a", "cols_b", "cols_c")
TILES = (256, 1024, 2048)
CHANGES = [("val0", "val1", "cols_a", "cols_a"), ("val1", "val0", "cols_a", "cols_a"),     # (old val, new val, old columns, new columns)
           ("val0", "val0", "cols_a", "cols_b"), ("val0", "val0", "cols_b", "cols_c"), ("val0", "val0", "cols_c", "cols_a")]


# ------------------------------------------------------------------------------------------------------------ the structure
def test_shape_and_row_lengths():
    lens = np.diff(M.row_ptr)
    assert (M.rows, M.cols) == (ad.ROWS, ad.COLS) and 250_000 <= M.nnz <= 350_000
    assert (lens[:ad.EMPTY_FRONT] == 0).all() and (lens[-ad.EMPTY_BACK:] == 0).all() and lens[ad.EMPTY_FRONT:-ad.EMPTY_BACK].any()
    assert ((lens >= 0) & (lens <= 40)).mean() > 0.99
    assert ((lens >= 33) & (lens <= 64)).sum() >= len(ad.MEDIUM) and ((lens > 40) & (lens <= 64)).sum() >= 5
    assert ((lens > 1024) & (lens <= 2048)).sum() == 1 and (lens > 2048).sum() == 1
    r2, n2 = ad.LONG_2                                                  # the longest row crosses tiles of every size
    assert all(M.row_ptr[r2] // t != (M.row_ptr[r2 + 1] - 1) // t for t in TILES)


@pytest.mark.parametrize("name", COLUMN_ARRAYS)
def test_columns_ascend_and_every_row_has_near_and_far_entries(name):
    c = getattr(M, name).astype(np.int64)
    row = ad.row_of_entries(M.row_ptr)
    assert c.min() >= 0 and c.max() < M.cols
    assert (np.diff(c)[np.diff(row) == 0] > 0).all(), "strictly ascending inside every row"
    dist = np.abs(c - row)
    lens = np.diff(M.row_ptr)
    for band in (ad.CLOSE, ad.MID):                                      # the binned plan at band 100 and at band 0 (= 4096)
        near, far = np.bincount(row[dist <= band], minlength=M.rows), np.bincount(row[dist > band], minlength=M.rows)
        assert ((near > 0) & (far > 0))[lens >= 2].all()
        assert 0.1 <= (dist <= band).mean() <= 0.9 and 0.1 <= (dist > band).mean() <= 0.9
        g = parity.binned_regime(M.row_ptr, c, M.cols, band)
        assert g["nf"] > 0 and g["long_rows"] >= 3 and g["capped_rows"] >= 1, g     # rows of > 32 far entries; one kept near


def test_narrow_share_of_the_three_column_arrays():
    for tile in (1024, 2048):
        a, b, c = (ad.narrow_tiles(M.nnz, getattr(M, n), tile) for n in COLUMN_ARRAYS)
        share = {n: ad.narrow_share(M.nnz, getattr(M, n), tile) for n in COLUMN_ARRAYS}
        print("narrow share, tiles of %d: %r" % (tile, share))
        assert share["cols_a"] == a.mean()
        assert 0.6 <= share["cols_a"] <= 0.9 and 0.6 <= share["cols_b"] <= 0.9        # in use, both kinds of tile present
        assert 0.05 <= share["cols_c"] < 0.4                                           # dropped
        assert ad.offsets_used(M.nnz, M.cols_a, tile) and ad.offsets_used(M.nnz, M.cols_b, tile)
        assert not ad.offsets_used(M.nnz, M.cols_c, tile)
        # the wide tiles of the two are exchanged: none is wide in both, and most tiles change kind either way
        assert not (~a & ~b).any() and (~a).sum() >= 0.25 * len(a) and (~b).sum() >= 0.25 * len(b)
        assert (a != b).mean() >= 0.6 and (b != c).mean() >= 0.3 and (c != a).mean() >= 0.3
    for p, q in (("cols_a", "cols_b"), ("cols_b", "cols_c"), ("cols_c", "cols_a")):
        assert (getattr(M, p) != getattr(M, q)).mean() > 0.95


def test_narrow_tiles_mirrors_the_plan_builder_rule():
    c = np.array([5, 65540, 7, 7 + 65535, 0, 65536, 3], dtype=np.int32)             # tiles of 2: span 65535, 65535, 65536, 0
    assert ad.narrow_tiles(7, c, 2).tolist() == [True, True, False, True]
    assert ad.narrow_share(7, c, 2) == 0.75 and ad.offsets_used(7, c, 2)
    wide = np.array([0, 70000, 0, 70000, 0, 1], dtype=np.int32)
    assert ad.narrow_share(6, wide, 2) == pytest.approx(1 / 3) and not ad.offsets_used(6, wide, 2)
    assert ad.offsets_used(4, wide, 2) is False and ad.offsets_used(4, np.array([0, 70000, 1, 2], np.int32), 2)   # 2 * narrow >= ntiles


def test_operands():
    assert (M.val0 != M.val1).all()
    assert set(np.abs(M.val0)) == set(range(1, 9)) and set(np.abs(M.val1)) == set(range(9, 17))
    for v in (M.val0, M.val1, M.x, M.x_rows, M.X, M.X_rows):
        assert ((v > 0).mean() > 0.4) and ((v < 0).mean() > 0.4) and (v != 0).all()
    assert np.abs(M.x).max() == 8 and M.x.shape == (M.cols,) and M.X.shape == (M.cols, 3) and M.X_rows.shape == (M.rows, 3)
    r0 = ad.block_start(M.row_ptr, M.rows)
    assert 2 * M.rows // 3 <= r0 < 2 * M.rows // 3 + 50 and M.row_ptr[r0] % 4 == 0


def test_tile_overflow_positions_on_a_small_row_ptr():
    rp = np.array([0, 0, 3, 3, 9, 10, 10, 14])                        # tiles of 4: [0,4) owns rows 1, 3 -> reads on to 9; [4,8) owns none;
    assert ad.tile_overflow_positions(rp, 4).tolist() == [4, 5, 6, 7, 8, 12, 13]   # [8,12) owns rows 4, 6 -> to 14; [12,14) owns none
    for tile in TILES:
        ovf = ad.tile_overflow_positions(M.row_ptr, tile)
        assert 1000 <= len(ovf) < M.nnz // 4


# --------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize("name", COLUMN_ARRAYS)
def test_references_are_the_oracles_bits(name):
    c = getattr(M, name)
    for v in (M.val0, M.val1):
        ref = ad.reference(M.row_ptr, c, v, M.x)
        assert np.abs(ref).max() < 2 ** 53 and np.count_nonzero(ref) > 0.9 * (np.diff(M.row_ptr) > 0).sum()
        transposed.assert_bits(ref, ob.csr_spmv(M.row_ptr, c, v, M.x), "reference, %s" % name)
        coo = ad.coo(M.row_ptr, c, v)
        transposed.assert_bits(ad.reference_t(M.row_ptr, c, v, M.x_rows, M.cols), transposed.reference(coo, M.rows, M.cols, M.x_rows),
                               "reference_t, %s" % name)
    block, block_t = ad.reference(M.row_ptr, c, M.val0, M.X), ad.reference_t(M.row_ptr, c, M.val0, M.X_rows, M.cols)
    assert block.shape == (M.rows, 3) and block_t.shape == (M.cols, 3) and np.abs(block_t).max() < 2 ** 53
    coo = ad.coo(M.row_ptr, c, M.val0)
    for k in range(3):
        transposed.assert_bits(block[:, k], ob.csr_spmv(M.row_ptr, c, M.val0, np.ascontiguousarray(M.X[:, k])), "block, column %d" % k)
        transposed.assert_bits(block_t[:, k], transposed.reference(coo, M.rows, M.cols, np.ascontiguousarray(M.X_rows[:, k])),
                               "transposed block, column %d" % k)
    r0 = ad.block_start(M.row_ptr, M.rows)                             # the row block's product is the slice of the whole one
    e0 = int(M.row_ptr[r0])
    transposed.assert_bits(ad.reference(M.row_ptr[r0:] - e0, c[e0:], M.val0[e0:], M.x), ad.reference(M.row_ptr, c, M.val0, M.x)[r0:], "row block")


def test_auto_pair_and_its_references():
    P = ad.auto_pair()
    assert P.rows == P.cols == 1 << 21 and P.nnz >= 4 * 1024 * 1024 and P.cols * 8 >= 16 * 1024 * 1024 and P.rows >= 4096
    row = ad.row_of_entries(P.row_ptr)
    for c in (P.band3, P.scattered3):
        assert c.min() >= 0 and c.max() < P.cols and (np.diff(c.astype(np.int64))[np.diff(row) == 0] > 0).all()
        transposed.assert_bits(ad.reference(P.row_ptr, c, P.val, P.x), ob.csr_spmv(P.row_ptr, c, P.val, P.x), "auto pair")
    d = np.minimum(np.abs(P.band3 - row), P.cols - np.abs(P.band3 - row))
    assert d.max() == 1
    assert (np.abs(P.scattered3 - row) > 4096).mean() > 0.95                       # far share: BINNED's second condition
    assert not transposed.same_bits(ad.reference(P.row_ptr, P.band3, P.val, P.x), ad.reference(P.row_ptr, P.scattered3, P.val, P.x))


# ------------------------------------------------------------------------------- the assertions reject what they are for
def stale_rows(old_val, new_val, old_cols, new_cols, where):
    """Rows whose product changes when the entries `where` (positions) keep the old value and column."""
    v, c = new_val.copy(), new_cols.copy()
    v[where], c[where] = old_val[where], old_cols[where]
    want, got = ad.reference(M.row_ptr, new_cols, new_val, M.x), ad.reference(M.row_ptr, c, v, M.x)
    assert transposed.same_bits(got, want) == (not (got != want).any())
    return int((got != want).sum())


@pytest.mark.parametrize("change", CHANGES, ids=lambda c: "%s:%s->%s:%s" % (c[0], c[2], c[1], c[3]))
def test_a_stale_copy_never_has_the_new_references_bits(change):
    old_val, new_val, old_cols, new_cols = (getattr(M, n) for n in change)
    assert stale_rows(old_val, new_val, old_cols, new_cols, np.arange(0)) == 0            # (nothing stale: the reference itself)
    assert stale_rows(old_val, new_val, old_cols, new_cols, np.arange(M.nnz // 2, M.nnz)) > 1000
    for tile in TILES:
        assert stale_rows(old_val, new_val, old_cols, new_cols, ad.tile_overflow_positions(M.row_ptr, tile)) > 10
    # one stale tile, every tile of every size in turn: the change of every entry's product, summed per (tile, row)
    delta = ad._int(old_val) * ad._int(M.x)[old_cols] - ad._int(new_val) * ad._int(M.x)[new_cols]
    row = ad.row_of_entries(M.row_ptr)
    for tile in TILES:
        ntiles = -(-M.nnz // tile)
        key = (np.arange(M.nnz) // tile) * M.rows + row
        keys, inverse = np.unique(key, return_inverse=True)
        sums = np.zeros(len(keys), dtype=np.int64)
        np.add.at(sums, inverse, delta)
        changed = np.bincount(keys[sums != 0] // M.rows, minlength=ntiles)
        assert changed.min() >= 1, "a stale tile %d of %d entries would cancel out" % (int(changed.argmin()), tile)
    first = np.arange(0, 1024)
    assert stale_rows(old_val, new_val, old_cols, new_cols, first) == np.count_nonzero(
        np.bincount(row[first], weights=delta[first], minlength=M.rows))
