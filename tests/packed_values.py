"""Structures and value sets for tests/test_gpu_packed_values.py (SMVP_CSR_KERNEL_STREAM_PACKED, the tile kernel's flavour 6), numpy only.

The family keeps the values of the packable tiles -- the full 2048-entry tiles whose columns span less than 65536 -- as 1-byte codes
into a table of the 64 most frequent bit patterns plus the other values ("escapes") wavefront by wavefront; wavefront w of a tile
takes the tile's entries [512 w, 512 w + 512).  The table comes from a sample of at most 2^20 values at a fixed stride: for the
matrices here, far smaller than that, the sample is the matrix and the table is the 64 most frequent patterns exactly (ties: the
smaller pattern).  hot_table() / escape_share() compute both on the host, so a test knows what the plan must have found.
"""
import numpy as np

TILE = 2048
WAVE = 512            # entries of a tile one wavefront takes
HOT = 64
LONG_ROW = 32         # kLongRow: longer rows are summed by a wavefront
OVER = 1024           # kStreamOver: a last row that runs further past its tile is finished from memory


def row_lengths(rng, nnz):
    """Rows of 1 ... 40 entries (85 % of 1 ... 8, 15 % of 9 ... 40) that hold `nnz` entries in all."""
    out, total = [], 0
    while total < nnz:
        n = int(rng.integers(1, 9)) if rng.random() < 0.85 else int(rng.integers(9, 41))
        n = min(n, nnz - total)
        out.append(n)
        total += n
    return np.array(out, dtype=np.int64)


def structure(lengths, cols, seed, band=400):
    """row_ptr, col_ind (ascending inside a row, within `band` of the row's place on the diagonal) for the given row lengths."""
    rng = np.random.default_rng(seed)
    rows = len(lengths)
    row_ptr = np.zeros(rows + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(lengths)
    col_ind = np.empty(int(row_ptr[-1]), dtype=np.int32)
    for r, n in enumerate(lengths):
        centre = int(r * (cols - 1) / max(1, rows - 1))
        lo, hi = max(0, centre - band), min(cols, centre + band)
        if hi - lo < n:      # (a row longer than the band is wide: it takes the first n columns from lo on, or the last n)
            lo = min(lo, cols - int(n))
            hi = lo + int(n)
        col_ind[row_ptr[r]:row_ptr[r + 1]] = np.sort(rng.choice(np.arange(lo, hi), size=int(n), replace=False))
    return row_ptr, col_ind


def base(tiles=6, tail=700, seed=11, cols=3000):
    """`tiles` full tiles and a partial one of `tail` entries (0: none): about 13 000 entries in 1 700 rows by default."""
    rng = np.random.default_rng(seed)
    lengths = row_lengths(rng, tiles * TILE + tail)
    rp, ci = structure(lengths, cols, seed + 1)
    return len(lengths), cols, rp, ci


def with_wide_tile(rows, cols, rp, ci, tile=3, far=150000):
    """The same rows over far + 1 columns, the last entry of a row in the middle of tile `tile` moved to column `far`: that tile's
    columns span more than 65535, its neighbours' do not."""
    ci = ci.copy()
    j = tile * TILE + TILE // 2
    r = int(np.searchsorted(rp, j, side="right")) - 1
    last = int(rp[r + 1]) - 1
    assert tile * TILE <= last < (tile + 1) * TILE
    ci[last] = far
    return rows, far + 1, rp, ci


def with_long_and_giant_rows(seed=23, cols=6000):
    """Six full tiles and a tail, with a row of 100 entries inside tile 1 and a row that starts 90 entries before the end of tile 2 and
    runs 1210 entries past it (more than kStreamOver): the overflow and giant-row paths read val itself."""
    rng = np.random.default_rng(seed)
    head = row_lengths(rng, TILE + 300)
    mid = row_lengths(rng, 3 * TILE - 90 - (TILE + 300) - 100)
    rest = row_lengths(rng, 7 * TILE - 400 - (3 * TILE + 1210))
    lengths = np.concatenate([head, [100], mid, [90 + 1210], rest])
    rp, ci = structure(lengths, cols, seed + 1, band=900)
    giant = len(head) + 1 + len(mid)
    assert rp[giant] == 3 * TILE - 90 and rp[giant + 1] - 3 * TILE > OVER and lengths[len(head)] > LONG_ROW
    return len(lengths), cols, rp, ci


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def hot_table(val):
    """The 64 most frequent bit patterns of val (ties: the smaller pattern), as the plan finds them when the sample is all of val."""
    pat, count = np.unique(bits(val), return_counts=True)
    order = np.lexsort((pat, -count))[:HOT]
    return np.sort(pat[order])


def packable_tiles(rp, ci):
    nnz = int(rp[-1])
    out = []
    for b in range(nnz // TILE):
        c = ci[b * TILE:(b + 1) * TILE].astype(np.int64)
        out.append(int(c.max() - c.min()) < 65536)
    return np.array(out + [False] * (int(nnz % TILE != 0)), dtype=bool)


def escapes_per_wavefront(rp, ci, val):
    """For every packable tile the four wavefronts' escape counts; None for the others."""
    hot = hot_table(val)
    esc = ~np.isin(bits(val), hot)
    return [np.add.reduceat(esc[b * TILE:(b + 1) * TILE], np.arange(0, TILE, WAVE)) if ok else None
            for b, ok in enumerate(packable_tiles(rp, ci))]


def escape_share(rp, ci, val):
    """Share of the entries one product still reads as 8-byte values: the escapes of the packable tiles and every entry of the others."""
    nnz = int(rp[-1])
    if nnz == 0:
        return 1.0
    total = 0
    for b, per in enumerate(escapes_per_wavefront(rp, ci, val)):
        total += int(per.sum()) if per is not None else min(TILE, nnz - b * TILE)
    return total / nnz


# ------------------------------------------------------------------------------------------------------------------ values
def distinct(n, start=1):
    """n different, finite, non-zero doubles: k / 1024 for k = start ... (exact in binary; sums of products with small integers too)."""
    return (np.arange(start, start + n, dtype=np.float64)) / 1024.0


def values(kind, rp, ci, seed=5):
    """One value per entry.  `kind`:
    hot64      every value one of 64 patterns: no escapes at all
    few        5 different values
    distinct   the full tiles hold different values throughout (512 escapes in every wavefront: the staging area exactly full); the
               64 table entries are taken by values that repeat in the partial tile alone (which reads val itself)
    half       about half of the entries from 40 frequent values, the others all different: odd and even counts per wavefront; in
               tile 2 wavefront 0 has no escape and wavefront 1 has 512
    third      three entries in ten hold a value of their own, the others one of 40 frequent values (AUTO's rule: well under its bound)
    special_hot      +0.0, -0.0, +-inf, a subnormal and two NaNs of different payload among the frequent values
    special_escaped  the same seven once or twice each among 64 far more frequent ordinary values: they escape
    """
    rng = np.random.default_rng(seed)
    nnz = int(rp[-1])
    full = nnz // TILE * TILE
    specials = np.array([0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x0000000000000123,
                         0x7ff8000000000001, 0xfff80000000abcde], dtype=np.uint64).view(np.float64)
    if kind == "hot64":
        return rng.choice(distinct(64), size=nnz)
    if kind == "few":
        return rng.choice(np.array([1.0, -2.5, 0.0, 3.0, 0.125]), size=nnz)
    if kind == "distinct":
        v = distinct(nnz, start=4096)
        if nnz > full:
            v[full:] = np.resize(np.repeat(distinct(64), 2), nnz - full)      # every table value at least twice where the tail allows
        return v
    if kind == "half":
        v = np.where(rng.random(nnz) < 0.5, rng.choice(distinct(40), size=nnz), distinct(nnz, start=4096))
        if nnz >= 3 * TILE:
            v[2 * TILE:2 * TILE + WAVE] = rng.choice(distinct(40), size=WAVE)
            v[2 * TILE + WAVE:2 * TILE + 2 * WAVE] = distinct(WAVE, start=4096 + 2 * TILE + WAVE)
        return v
    if kind == "third":
        return np.where(rng.random(nnz) < 0.3, distinct(nnz, start=4096), rng.choice(distinct(40), size=nnz))
    if kind == "special_hot":
        pool = np.concatenate([specials, distinct(20)])
        return np.where(rng.random(nnz) < 0.6, rng.choice(pool, size=nnz), distinct(nnz, start=4096))
    if kind == "special_escaped":
        v = rng.choice(distinct(64), size=nnz)
        where = rng.choice(full if full else nnz, size=2 * len(specials), replace=False)
        v[where] = np.concatenate([specials, specials])[:len(where)]
        if full >= 3 * TILE:       # ... and three of them side by side in one wavefront
            v[TILE + 5:TILE + 8] = specials[[1, 5, 6]]
        return v
    raise ValueError(kind)


KINDS = ("hot64", "few", "distinct", "half", "special_hot", "special_escaped")
