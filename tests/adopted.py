"""What the tests of adopted device arrays (SMVP_MEM_DEVICE) multiply: one structure `mixed` with three column arrays and two
value arrays over one row_ptr, the two matrices of the AUTO test, and their exact references.

Plain functions (no fixtures, no GPU): test_gpu_adopted.py uses them on the GPU, test_adopted_host.py holds them to their
conditions and shows that a product made with stale entries never equals the reference of the new ones.

Exact operands (the choice of tests/ceiling.py): values and operands are non-zero integers stored as doubles, so every product
and every partial sum is exact in any order and every path -- TJDS ATOMIC included -- must give the int64 reference bit for
bit.  No tolerance appears anywhere.
  val0   magnitudes 1 ... 8            val1   magnitudes 9 ... 16, fresh signs: every entry differs from val0
  x      integers in [-8, 8] without 0: one stale entry changes its row's sum

`mixed`: ROWS x COLS, about 300 k entries.  Row lengths 0 ... 40 for most rows, MEDIUM rows of 33 ... 64, one row of LONG_1 >
1024 and one of LONG_2 > 2048 entries (it crosses tiles), empty rows in front and at the back.  A row of two entries or more
holds entries within 100 of the diagonal, entries 101 ... 4096 above it and entries further than 4096 from it, so the binned
plan at band 0 (= 4096) and at band 100 has a near part and a far part; the MEDIUM rows and LONG_1 have more than 32 far entries
(summed by a wavefront), LONG_2 more than 1024 (kept near).

The three column arrays differ in where the far entries of a row lie.  A "narrow" row keeps them in r + 4097 ... r + 50000: a
tile of such rows spans fewer than 65536 columns and takes the tile kernel's 16-bit column offsets.  A "wide" row spreads them
over all columns: its tile keeps 32-bit columns.  The kind goes by the stretch of GROUP = 8192 entries a row lies in (a row that
touches a narrow stretch is narrow, and so are the rows longer than 64), in a pattern of three stretches:
  cols_a   wide, narrow, narrow         cols_b   narrow, wide, narrow         cols_c   wide, wide, wide, narrow (period 4)
so about two thirds of the tiles of cols_a and of cols_b are narrow (the offsets are in use, both kinds of tile present), every
tile that is wide in one of the two is narrow in the other, and a quarter of cols_c's are (the offsets are dropped).  Both
arrays cannot have 60 % narrow tiles AND every narrow tile of cols_a wide in cols_b (at most 40 % would be left): the wide tiles
are exchanged, the columns of every tile differ, and the host test counts the tiles that change kind.
"""
import functools
from types import SimpleNamespace

import numpy as np

ROWS, COLS = 20_000, 200_000
EMPTY_FRONT, EMPTY_BACK = 5, 7
MEDIUM = {1500: 33, 4100: 40, 7777: 47, 9000: 56, 12001: 64, 15555: 50, 19000: 61}     # row: length
LONG_1, LONG_2 = (6000, 1200), (14000, 2500)                                            # (row, length)
GROUP = 8192                            # entries: 8 tiles of 1024, 4 of 2048
CLOSE, MID, NARROW_FAR = 100, 4096, 50_000
PATTERNS = {"cols_a": (True, False, False), "cols_b": (False, True, False), "cols_c": (True, True, True, False)}   # True: wide
SPAN16 = 65536                          # a tile whose columns span less takes 16-bit offsets (tile_column_spans)

AUTO_N = 1 << 21                        # test 7: the smallest matrix AUTO samples (nnz >= 4 Mi, rows >= 4096, cols * 8 >= 16 MiB)


# ------------------------------------------------------------------------------------------------------------- operands
def int_values(rng, n, lo, hi):
    """n non-zero integers of magnitude lo ... hi with random signs, as doubles."""
    return (rng.integers(lo, hi + 1, n) * rng.choice([-1, 1], n)).astype(np.float64)


def row_of_entries(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))


# ----------------------------------------------------------------------------------------------------------- the structure
def row_lengths(rng):
    lens = rng.integers(0, 41, ROWS)
    lens = np.where(rng.random(ROWS) < 0.5, lens // 2, lens)
    for r, n in MEDIUM.items():
        lens[r] = n
    for r, n in (LONG_1, LONG_2):
        lens[r] = n
    lens[:EMPTY_FRONT] = 0
    lens[ROWS - EMPTY_BACK:] = 0
    return lens


def class_counts(lens):
    """(close, mid, far) entries of every row: |column - row| <= 100, 101 ... 4096 above the diagonal, further than 4096."""
    lens = np.asarray(lens, dtype=np.int64)
    close = np.where(lens >= 2, np.maximum(1, (2 * lens) // 5), lens)
    far = np.where(lens >= 2, np.maximum(1, (2 * lens) // 5), 0)
    for r in MEDIUM:
        close[r], far[r] = 4, lens[r] - 7
    (r1, n1), (r2, n2) = LONG_1, LONG_2
    close[r1], far[r1] = 150, 700
    close[r2], far[r2] = 150, 1500
    return close, lens - close - far, far


def wide_rows(row_ptr, pattern):
    """The rows whose far entries spread over all columns: every stretch of GROUP entries the row touches is a wide one, and the
    row is no longer than 64."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    lens = np.diff(row_ptr)
    pat = np.asarray(pattern, dtype=bool)
    first = pat[(row_ptr[:-1] // GROUP) % len(pat)]
    last = pat[((np.maximum(row_ptr[1:], 1) - 1) // GROUP) % len(pat)]
    return first & last & (lens > 0) & (lens <= 64)


def columns(rng, row_ptr, pattern):
    """col_ind over row_ptr, strictly ascending inside every row.  Entry i of the n entries of a class takes one column out of
    the i-th of n equal parts of the class's range, so the columns of a row are distinct by construction."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    lens = np.diff(row_ptr)
    close, mid, far = class_counts(lens)
    wide = wide_rows(row_ptr, pattern)
    row = row_of_entries(row_ptr)
    j = np.arange(row_ptr[-1], dtype=np.int64) - row_ptr[row]
    cls = (j >= close[row]).astype(np.int64) + (j >= (close + mid)[row])
    i = j - np.where(cls == 0, 0, np.where(cls == 1, close[row], (close + mid)[row]))
    n = np.where(cls == 0, close[row], np.where(cls == 1, mid[row], far[row]))
    below = np.maximum(row - MID, 0)                                   # columns 0 ... row - 4097 of a wide row's far range
    lo = np.where(cls == 0, np.maximum(row - CLOSE, 0), np.where(cls == 1, row + CLOSE + 1, np.where(wide[row], 0, row + MID + 1)))
    width = np.where(cls == 0, row + CLOSE + 1 - lo, np.where(cls == 1, MID - CLOSE,
                     np.where(wide[row], below + (COLS - row - MID - 1), NARROW_FAR - MID)))
    seg = width // n
    assert (seg >= 1).all()
    u = i * seg + rng.integers(0, 1 << 31, len(row)) % seg
    col = lo + u
    jump = (cls == 2) & wide[row] & (u >= below)                       # the part of a wide row's far range above the diagonal
    col = np.where(jump, row + MID + 1 + (u - below), col)
    order = np.lexsort((col, row))
    return np.ascontiguousarray(col[order], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def mixed(seed=2026):
    """The structure and its operands -> namespace: rows, cols, nnz, row_ptr, cols_a / cols_b / cols_c, val0 / val1, x (COLS),
    x_rows (ROWS: the transposed product's operand), X (COLS x 3) and X_rows (ROWS x 3): the block products'."""
    rng = np.random.default_rng(seed)
    lens = row_lengths(rng)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    m = SimpleNamespace(rows=ROWS, cols=COLS, nnz=nnz, row_ptr=row_ptr)
    for name, pattern in PATTERNS.items():
        setattr(m, name, columns(rng, row_ptr, pattern))
    m.val0 = int_values(rng, nnz, 1, 8)
    m.val1 = int_values(rng, nnz, 9, 16)
    m.x, m.x_rows = int_values(rng, COLS, 1, 8), int_values(rng, ROWS, 1, 8)
    m.X, m.X_rows = int_values(rng, COLS * 3, 1, 8).reshape(COLS, 3), int_values(rng, ROWS * 3, 1, 8).reshape(ROWS, 3)
    for a in vars(m).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def block_start(row_ptr, rows):
    """First row of the row block that test 1 adopts: the first row of the last third whose entries start at a multiple of four,
    so that the views of col_ind and val from there are 16-byte aligned."""
    r = 2 * rows // 3
    while int(row_ptr[r]) % 4:
        r += 1
    return r


# ------------------------------------------------------------------------------------------------- the 16-bit column offsets
def narrow_tiles(row_ptr_end, col_ind, tile):
    """Which tiles of `tile` consecutive entries take 16-bit offsets: hi - lo < 65536 (tile_column_spans)."""
    nnz = int(row_ptr_end)
    c = np.asarray(col_ind[:nnz], dtype=np.int64)
    starts = np.arange(0, nnz, tile)
    return (np.maximum.reduceat(c, starts) - np.minimum.reduceat(c, starts) < SPAN16) if nnz else np.zeros(0, dtype=bool)


def narrow_share(row_ptr_end, col_ind, tile):
    fits = narrow_tiles(row_ptr_end, col_ind, tile)
    return float(fits.mean()) if len(fits) else 0.0


def offsets_used(row_ptr_end, col_ind, tile):
    """build_column_offsets keeps the offsets when 2 * narrow >= ntiles."""
    fits = narrow_tiles(row_ptr_end, col_ind, tile)
    return len(fits) > 0 and 2 * int(fits.sum()) >= len(fits)


def tile_overflow_positions(row_ptr, tile):
    """The entries a tile of the TJDS one-kernel product reads past its own end (build_stream_plan's ovf_ptr: from the tile's end
    to the end of the last row that starts in it), whose values the plan keeps a second time (build_tile_overflow)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nnz = int(row_ptr[-1])
    mask = np.zeros(nnz, dtype=bool)
    starts = row_ptr[:-1][np.diff(row_ptr) > 0]
    for b in range(-(-nnz // tile)):
        s, e = b * tile, min((b + 1) * tile, nnz)
        own = starts[(starts >= s) & (starts < e)]
        if len(own):
            mask[e:int(row_ptr[np.searchsorted(row_ptr, own[-1], side="right")])] = True
    return np.flatnonzero(mask)


# -------------------------------------------------------------------------------------------------------------- references
def _int(a):
    a = np.asarray(a)
    i = a.astype(np.int64)
    assert np.array_equal(i, a), "the operands of the exact references are integers"
    return i


def reference(row_ptr, col_ind, val, x):
    """y = A x in int64, as doubles; x of shape (cols,) or (cols, k)."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nnz = int(row_ptr[-1])
    xi = _int(x)
    v = _int(val)[:nnz]
    p = v * xi[np.asarray(col_ind)[:nnz]] if xi.ndim == 1 else v[:, None] * xi[np.asarray(col_ind)[:nnz]]
    run = np.concatenate([np.zeros((1,) + p.shape[1:], dtype=np.int64), np.cumsum(p, axis=0)])
    y = run[row_ptr[1:]] - run[row_ptr[:-1]]
    assert np.abs(y).max(initial=0) < 2 ** 53
    return y.astype(np.float64)


def reference_t(row_ptr, col_ind, val, x, cols):
    """y = A^T x in int64, as doubles; x of shape (rows,) or (rows, k) -- the block form."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nnz = int(row_ptr[-1])
    xi = _int(x)
    p = (_int(val)[:nnz] * xi[row_of_entries(row_ptr)].T).T
    y = np.zeros((cols,) + p.shape[1:], dtype=np.int64)
    np.add.at(y, np.asarray(col_ind)[:nnz], p)
    assert np.abs(y).max(initial=0) < 2 ** 53
    return y.astype(np.float64)


def coo(row_ptr, col_ind, val):
    """The COO list of the structure in storage order (the TJDS side is built from it)."""
    from transposed import coo_of_csr

    return coo_of_csr(row_ptr, col_ind, val)


# ------------------------------------------------------------------------------------------------ test 7: AUTO's two matrices
@functools.lru_cache(maxsize=None)
def auto_pair(n=AUTO_N, seed=7):
    """n x n with 3 entries per row -> namespace: rows, cols, nnz, row_ptr, band3 (columns r - 1, r, r + 1 modulo n: neighbouring
    gathers share lines, AUTO stays on STREAM), scattered3 (three distinct uniform columns, ascending: every gather pulls its own
    line and nearly every entry is far), val, x."""
    rng = np.random.default_rng(seed)
    r = np.arange(n, dtype=np.int64)
    band = np.sort(np.stack([(r - 1) % n, r, (r + 1) % n], axis=1), axis=1)
    scat = np.sort(rng.integers(0, n, (n, 3)), axis=1)
    while True:
        dup = np.flatnonzero((scat[:, 0] == scat[:, 1]) | (scat[:, 1] == scat[:, 2]))
        if not len(dup):
            break
        scat[dup] = np.sort(rng.integers(0, n, (len(dup), 3)), axis=1)
    m = SimpleNamespace(rows=n, cols=n, nnz=3 * n, row_ptr=(3 * np.arange(n + 1)).astype(np.int32),
                        band3=np.ascontiguousarray(band.reshape(-1), dtype=np.int32),
                        scattered3=np.ascontiguousarray(scat.reshape(-1), dtype=np.int32),
                        val=int_values(rng, 3 * n, 1, 8), x=int_values(rng, n, 1, 8))
    for a in vars(m).values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m
