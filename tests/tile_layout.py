"""The matrices, operands and yardsticks of test_gpu_tile_layout.py and the kernel's lane formula restated; plain functions, tested
on the host by test_tile_layout_host.py."""
import functools

import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm

TILES = (1024, 2048)          # the tile sizes the matrices are built for: VPT 4 and 8
CONTROL = 256                 # VPT == 1 on the matrices built for 1024
LONG_ROW = 32                 # kLongRow: rows up to this are summed left to right by one lane
OVER = 1024                   # kStreamOver: a last row that runs further than this past its tile is a giant
WAVE = 64
BLOCK = 256                   # threads per workgroup
KINDS = ("tail", "tail_wide_one", "tail_wide_all", "giant", "exact", "exact_less_one")


# --------------------------------------------------------------------------------------------------- the kernel's formula
def lane_entry(vpt, t, k):
    """Offset in the tile of entry k (0 ... vpt - 1) of thread t: owner_body's lane_entry (csrc/smvp_owner_kernel.h).  The product
    goes to prod[] at the same offset."""
    wave, lane = t // WAVE, t % WAVE
    if vpt == 1:
        return t
    return wave * WAVE * vpt + 128 * (k // 2) + 2 * lane + (k & 1)


# ------------------------------------------------------------------------------------------------------------ the matrices
def short_rows(rng, total):
    """Row lengths 0 ... 24, a quarter of them 0 ... 3, that add up to `total`."""
    out, left = [], total
    while left > 0:
        n = int(rng.integers(0, 25))
        if rng.random() < 0.25:
            n //= 8
        n = min(n, left)
        out.append(n)
        left -= n
    return out


def to_boundary(rng, lens, tile, short_of=0):
    """Short rows up to `short_of` entries in front of the next tile boundary."""
    at = sum(lens)
    want = -(-at // tile) * tile - short_of
    if want < at:
        want += tile
    return lens + short_rows(rng, want - at)


def row_lengths(kind, tile):
    rng = np.random.default_rng(tile + len(kind))
    if kind == "exact":
        return short_rows(rng, tile) + [0, 0]
    if kind == "exact_less_one":
        return [0] + short_rows(rng, tile - 1)
    if kind == "giant":
        # a row that runs 1500 entries past its tile; later one that starts 5 entries in front of a tile boundary and covers the
        # whole next tile (no row starts there); a partial last tile
        lens = [0, 0] + short_rows(rng, tile - 10) + [10 + 1500]
        lens = to_boundary(rng, lens, tile, short_of=5) + [5 + tile + 600]
        return lens + short_rows(rng, 700) + [0, 0, 0]
    # "tail*": 3 tiles and 517 entries.  Tile 0: short rows and one of 33, its last row starts 3 entries in front of the boundary
    # and runs 40 into tile 1.  Tile 1: a row of 574, short rows up to the boundary exactly, then 6 rows without entries (they
    # belong to tile 2).  Tile 2: short rows (some empty), its last row starts 7 in front of the boundary and runs 300 past it
    # (more overflow entries than the workgroup has lanes).  The partial tile 3: short rows.
    lens = [0, 0] + short_rows(rng, 200) + [33]
    lens = to_boundary(rng, lens, tile, short_of=3) + [3 + 40, 574]
    lens = to_boundary(rng, lens, tile) + [0] * 6
    lens = to_boundary(rng, lens + [5], tile, short_of=7) + [7 + 300]
    lens = lens + short_rows(rng, 3 * tile + 517 - sum(lens)) + [0, 0, 0]
    assert sum(lens) == 3 * tile + 517
    return lens


@functools.lru_cache(maxsize=None)
def matrix(kind, tile):
    """The structure, its operands and the two yardsticks, computed once and shared read-only.  Columns rise by 2 inside a row
    from an offset of the row's own; "band" keeps every column below 1200 (8000 where a row is longer than that), so every tile
    takes the 16-bit offsets; "tail_wide_one" puts the odd rows that start in tile 1 150000 columns to the right (that tile alone
    spans 65536 or more), "tail_wide_all" the odd rows of every tile (the plan keeps the 32-bit columns)."""
    lens = np.array(row_lengths(kind, tile), dtype=np.int64)
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    nnz = int(row_ptr[-1])
    band = 1200 if lens.max() < 600 else 8000
    cols = band if kind in ("tail", "giant", "exact", "exact_less_one") else 200000
    col_ind = np.zeros(nnz, dtype=np.int32)
    for r in range(rows):
        n = int(lens[r])
        off = (13 * r) % (band - 2 * n)
        if r & 1 and (kind == "tail_wide_all" or (kind == "tail_wide_one" and row_ptr[r] // tile == 1)):
            off += 150000
        col_ind[row_ptr[r]:row_ptr[r + 1]] = off + 2 * np.arange(n)
    rng = np.random.default_rng(7 * tile + len(kind))
    val, x = rng.random(nnz) * 2.0 - 1.0, rng.random(cols) + 0.5
    serial = np.zeros(rows)                   # the serial loop: products rounded, then added left to right
    for r in range(rows):
        acc = 0.0
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc += float(val[j]) * float(x[col_ind[j]])
        serial[r] = acc
    m = {"rows": rows, "cols": cols, "nnz": nnz, "lens": lens, "row_ptr": row_ptr, "col_ind": col_ind, "val": val, "x": x,
         "serial": serial, "oracle": ob.csr_spmv(row_ptr, col_ind, val, x),
         "scale": ob.csr_spmv(row_ptr, col_ind, np.abs(val), np.abs(x)),
         "coo": sm.make_coo(np.repeat(np.arange(rows), lens), col_ind, val)}
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def built_for(tile):
    return 1024 if tile == CONTROL else tile


def tile_spans(m, tile):
    """max - min column of every tile of `tile` entries."""
    return np.array([int(m["col_ind"][s:s + tile].max()) - int(m["col_ind"][s:s + tile].min()) for s in range(0, m["nnz"], tile)])


def expected_flavor(kind, tile):
    """Csr16 (5) where at least half of the tiles span less than 65536 columns and the tile has 1024 entries or more, else Csr (0)."""
    return 5 if tile >= 1024 and kind != "tail_wide_all" else 0
