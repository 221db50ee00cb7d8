"""What the packed tile kernel (csr_stream_owner<8, 6, .>) reads of a tile's plan, restated in numpy as one row of eight words per
tile, its invariants, and the small structures at which those words or the kernel's one flight of loads can go wrong.  For
tests/test_tile_record_host.py (CPU) and tests/test_gpu_tile_record.py; tests/packed_values.py has the family's other structures, its
value sets and what the plan must find of them (packable_tiles, escapes_per_wavefront).

The kernel requests a tile's plan words together -- tile_row[b], tile_row[b + 1], tile_next[b], col_base[b] and its wavefront's two
words of esc_ptr -- and waits for them once.  The row of tile b here: first owned row, one past the last owned row, end of the last
owned row (zend), column base (< 0: the tile's columns span 65536 or more), start of the tile's escapes in esc_val, the four
wavefronts' padded escape counts as two pairs of 16-bit halves, flags (bit 0: packable -- esc_ptr marks the others by ~start).  One
more row stands behind the last tile, as esc_ptr's last word does.
"""
import numpy as np

import packed_values as pv

TILE, WAVE = pv.TILE, pv.WAVE
WORDS = 8
PACKABLE = 1


def records(rp, ci, val):
    """(ntiles + 1) x 8 int64: every tile's record and the pad's, from row_ptr, col_ind and the values."""
    rp = np.asarray(rp, dtype=np.int64)
    rows, nnz = len(rp) - 1, int(rp[-1])
    ntiles = max(1, -(-nnz // TILE))
    # the first row that starts at or behind the tile's first entry owns ... (rows past the last entry belong to the last tile)
    tile_row = np.array([min(rows, int(np.searchsorted(rp[:rows], b * TILE, side="left"))) for b in range(ntiles)] + [rows])
    ok = pv.packable_tiles(rp, ci)
    per = pv.escapes_per_wavefront(rp, ci, val)
    rec = np.zeros((ntiles + 1, WORDS), dtype=np.int64)
    start = 0
    for b in range(ntiles):
        c = np.asarray(ci[b * TILE:min((b + 1) * TILE, nnz)], dtype=np.int64)
        narrow = c.size > 0 and int(c.max() - c.min()) < 65536
        counts = (per[b] + 1) // 2 * 2 if b < len(per) and per[b] is not None else np.zeros(4, dtype=np.int64)
        rec[b] = [tile_row[b], tile_row[b + 1], rp[tile_row[b + 1]], int(c.min()) if narrow else -1, start,
                  int(counts[0]) | int(counts[1]) << 16, int(counts[2]) | int(counts[3]) << 16,
                  PACKABLE if b < len(ok) and ok[b] else 0]
        start += int(counts.sum())
    rec[ntiles] = [rows, rows, nnz, -1, start, 0, 0, 0]
    return rec


def counts_of(rec):
    """n x 4: the wavefronts' padded escape counts out of words 5 and 6."""
    return np.stack([rec[:, 5] & 0xffff, rec[:, 5] >> 16, rec[:, 6] & 0xffff, rec[:, 6] >> 16], axis=1)


def check_invariants(rec, rp, ci, val):
    """What holds of every plan's records whatever the matrix; -> the number of packable tiles."""
    rp = np.asarray(rp, dtype=np.int64)
    rows, nnz = len(rp) - 1, int(rp[-1])
    ntiles = len(rec) - 1
    assert ntiles == max(1, -(-nnz // TILE)) and rec.shape[1] == WORDS
    counts = counts_of(rec)
    assert np.all(np.diff(rec[:, 4]) >= 0), "the starts are not non-decreasing"
    assert np.all(rec[:, 4] % 2 == 0), "a run starts at an odd place: its pairs are not 16-byte aligned"
    assert np.all(counts % 2 == 0) and np.all(counts <= WAVE) and np.all(counts >= 0), "a count is odd or over 512"
    assert np.all(rec[1:, 4] == rec[:-1, 4] + counts[:-1].sum(axis=1)), "a tile's escapes do not follow its predecessor's"
    assert rec[0, 0] == 0 and rec[ntiles - 1, 1] == rows, "the first tile does not start at row 0 or the last does not end at the last row"
    assert np.all(rec[1:ntiles, 0] == rec[:ntiles - 1, 1]), "the owned-row ranges of successive tiles do not abut"
    assert np.all(rec[:, 0] <= rec[:, 1])
    ends = np.minimum((np.arange(ntiles) + 1) * TILE, nnz)
    owns = rec[:ntiles, 0] < rec[:ntiles, 1]
    assert np.all(rec[:ntiles, 2][owns] >= ends[owns]), "zend lies before the end of a tile that owns rows"
    assert np.all(rec[:ntiles, 2] == rp[rec[:ntiles, 1]])
    ok = pv.packable_tiles(rp, ci)
    flags = rec[:ntiles, 7]
    assert np.all((flags & ~PACKABLE) == 0)
    assert np.array_equal((flags & PACKABLE) != 0, np.concatenate([ok, np.zeros(ntiles - len(ok), dtype=bool)])), "packable differs from packable_tiles"
    assert np.all(rec[:ntiles, 3][(flags & PACKABLE) != 0] >= 0), "a packable tile without a column base"
    assert np.all(counts[:ntiles][(flags & PACKABLE) == 0] == 0), "a tile that is not packable has escapes"
    assert np.all(rec[ntiles, 5:] == 0) and rec[ntiles, 0] == rec[ntiles, 1] == rows
    per = pv.escapes_per_wavefront(rp, ci, val)
    for b, p in enumerate(per):
        if p is not None:
            assert np.all(counts[b] - p >= 0) and np.all(counts[b] - p <= 1), "a count is not the escapes rounded up to even"
    return int(((flags & PACKABLE) != 0).sum())


# ----------------------------------------------------------------------------------------------------------------- structures
def _of_lengths(lengths, cols, seed, band=400):
    lengths = np.asarray(lengths, dtype=np.int64)
    rp, ci = pv.structure(lengths, cols, seed, band=band)
    return len(lengths), cols, rp, ci


def one_tile(extra=0, seed=31, cols=900):
    """Exactly one full tile, or one full tile and `extra` entries more (a partial second tile that owns at most the last rows)."""
    return _of_lengths(pv.row_lengths(np.random.default_rng(seed), TILE + extra), cols, seed + 1)


def no_row_starts(seed=41, cols=6000):
    """Five full tiles and a tail; a row that starts 1000 entries into tile 1 and ends 300 entries into tile 3: no row starts in
    tile 2 (it leaves right after its plan words), tile 1 finishes the row from memory (it runs 2348 > kStreamOver entries past it)."""
    rng = np.random.default_rng(seed)
    head = pv.row_lengths(rng, TILE + 1000)
    rest = pv.row_lengths(rng, 5 * TILE + 600 - (3 * TILE + 300))
    rows, cols, rp, ci = _of_lengths(np.concatenate([head, [1048 + TILE + 300], rest]), cols, seed + 1, band=2500)
    b = np.array([int(np.searchsorted(rp[:rows], k * TILE, side="left")) for k in range(4)])
    assert b[2] == b[3] and rp[b[2]] == 3 * TILE + 300
    return rows, cols, rp, ci


def short_rows(seed=51, cols=2500):
    """Rows of one and two entries only, four full tiles and a tail: a tile owns some 1365 rows, more than the 512 whose bounds come
    with the tile, so the loop past a lane's two prefetched rows runs."""
    rng = np.random.default_rng(seed)
    lengths, total = [], 0
    while total < 4 * TILE + 333:
        n = min(int(rng.integers(1, 3)), 4 * TILE + 333 - total)
        lengths.append(n)
        total += n
    rows, cols, rp, ci = _of_lengths(lengths, cols, seed + 1, band=300)
    assert int(np.searchsorted(rp[:rows], TILE, side="left")) > 512 + 256
    return rows, cols, rp, ci


def empty_rows_at_the_edges(seed=61, cols=1200):
    """Two full tiles exactly.  Rows 0 and 1 are empty (the first owned rows of tile 0), two empty rows sit where tile 1 starts (its
    first owned rows, at offset 0) and three behind the last entry (the last owned rows of tile 1, a full packable tile: their
    16-bit offset is 2048, the tile's size)."""
    rng = np.random.default_rng(seed)
    a, b = pv.row_lengths(rng, TILE), pv.row_lengths(rng, TILE)
    rows, cols, rp, ci = _of_lengths(np.concatenate([[0, 0], a, [0, 0], b, [0, 0, 0]]), cols, seed + 1)
    assert rp[-1] == 2 * TILE and rp[2 + len(a)] == rp[2 + len(a) + 2] == TILE and rp[-4] == 2 * TILE
    return rows, cols, rp, ci


NEW_STRUCTURES = {
    "exactly one tile": lambda: one_tile(0),
    "one tile and one entry": lambda: one_tile(1),
    "a tile in which no row starts": no_row_starts,
    "rows of one and two entries": short_rows,
    "empty rows at the tiles' edges": empty_rows_at_the_edges,
}
STRUCTURES = dict({
    "six tiles and a tail": lambda: pv.base(),
    "a wide tile": lambda: pv.with_wide_tile(*pv.base()),
    "long and giant rows": lambda: pv.with_long_and_giant_rows(),
}, **NEW_STRUCTURES)
