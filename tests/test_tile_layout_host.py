"""Host checks of tile_layout.py: the lane formula of the tile kernel's phase 1 tiles a tile exactly, and the test matrices hold the
structures test_gpu_tile_layout.py needs them for."""
import numpy as np
import pytest

from tile_layout import BLOCK, KINDS, LONG_ROW, OVER, TILES, WAVE, lane_entry, matrix, tile_spans

@pytest.mark.parametrize("vpt", (1, 4, 8))
def test_lane_entries_tile_the_tile(vpt):
    """Every entry of a full tile is owned by exactly one (thread, k) and its prod[] slot is its offset in the tile; a wavefront
    owns 64 * vpt consecutive entries; the lanes of one load / gather / store instruction hold neighbouring entries (pairs: 128
    consecutive entries per pair of k); in a partial tile the per-entry test offset < left keeps exactly the entries that exist."""
    tile = BLOCK * vpt
    owner = {}
    for t in range(BLOCK):
        for k in range(vpt):
            e = lane_entry(vpt, t, k)
            assert 0 <= e < tile and e not in owner, (t, k, e)
            owner[e] = (t, k)
    assert sorted(owner) == list(range(tile))
    for w in range(BLOCK // WAVE):
        held = sorted(lane_entry(vpt, t, k) for t in range(w * WAVE, (w + 1) * WAVE) for k in range(vpt))
        assert held == list(range(w * WAVE * vpt, (w + 1) * WAVE * vpt))
        for k in range(0, vpt, 2):
            slab = sorted(lane_entry(vpt, t, kk) for t in range(w * WAVE, (w + 1) * WAVE) for kk in range(k, min(k + 2, vpt)))
            assert slab == list(range(slab[0], slab[0] + len(slab))), "one instruction, one run of consecutive entries"
            if vpt > 1:
                assert all(lane_entry(vpt, t, k) % 2 == 0 and lane_entry(vpt, t, k + 1) == lane_entry(vpt, t, k) + 1
                           for t in range(w * WAVE, (w + 1) * WAVE)), "16-byte value loads and LDS stores are aligned pairs"
    for left in (1, 517 % tile, tile - 1):
        kept = sorted(lane_entry(vpt, t, k) for t in range(BLOCK) for k in range(vpt) if lane_entry(vpt, t, k) < left)
        assert kept == list(range(left))
    if vpt > 1:                               # 517 entries left: some thread owns entries that exist and entries that do not
        assert any(0 < sum(lane_entry(vpt, t, k) < 517 for k in range(vpt)) < vpt for t in range(BLOCK))


@pytest.mark.parametrize("tile", TILES)
def test_structures_hold_what_they_claim(tile):
    m = matrix("tail", tile)
    lens, rp = m["lens"], m["row_ptr"].astype(np.int64)
    first = rp[:-1]
    assert m["nnz"] == 3 * tile + 517
    assert matrix("exact", tile)["nnz"] == tile and matrix("exact_less_one", tile)["nnz"] == tile - 1
    # a row that starts in the last 3 entries of tile 0 and runs 40 into tile 1; rows of 33 and 574; more than 256 overflow entries
    assert ((first == tile - 3) & (lens == 43)).any() and (lens == 33).any() and (lens == 574).any()
    assert ((first == 3 * tile - 7) & (lens == 307)).any()
    # rows without entries at a tile boundary, at the front, at the back and in between
    assert ((first == 2 * tile) & (lens == 0)).sum() == 6 and (lens[first == 2 * tile] > 0).any()
    assert lens[0] == 0 and lens[-1] == 0
    assert (first[lens > 0] >= 3 * tile).any(), "rows start in the partial tile: its products are used"
    for kind in KINDS:
        mk = matrix(kind, tile)
        wide = tile_spans(mk, tile) >= 65536
        if kind == "tail_wide_one":
            assert list(wide) == [False, True, False, False]
        elif kind == "tail_wide_all":
            assert 2 * wide.sum() > len(wide)
        else:
            assert not wide.any()
        for r in range(mk["rows"]):
            c = mk["col_ind"][mk["row_ptr"][r]:mk["row_ptr"][r + 1]]
            assert (np.diff(c) > 0).all() and (not len(c) or (0 <= c[0] and c[-1] < mk["cols"]))
        assert np.array_equal(mk["serial"][mk["lens"] <= LONG_ROW], mk["oracle"][mk["lens"] <= LONG_ROW])
    g = matrix("giant", tile)
    lens, first = g["lens"], g["row_ptr"].astype(np.int64)[:-1]
    past = first + lens - (first // tile + 1) * tile
    assert ((first == tile - 10) & (past == 1500)).any(), "a row that runs 1500 entries past its tile"
    starts = np.bincount((first[lens > 0] // tile).astype(np.int64), minlength=-(-g["nnz"] // tile))
    assert (starts == 0).any() and g["nnz"] % tile != 0, "a tile in which no row starts; a partial last tile"
    assert (past > OVER).sum() == 2
