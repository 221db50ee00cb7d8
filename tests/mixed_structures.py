"""Matrices as Matrix Market files and the row blocks of a sharded run hold them: repeated (row, col) pairs, rows whose
columns are not ascending, rectangular shapes, row blocks with first_row != 0 -- at the smallest sizes that cross the blocks of
the blocked plans (K6's 8192 rows per workgroup, the binned plan's 16384-column blocks and 7168-entry buckets, the 65536-column
span of the 16-bit offsets).

Plain functions (no fixtures, no GPU): test_gpu_mixed_structures.py multiplies these on every path, test_mixed_structures_host.py
holds every structure to its conditions (assert_regime) and shows that numpy models of the wrong kernels these inputs are meant
to catch never give the exact reference.

structure(name) -> (rows, cols, first_row, coo); name = "<kind>:<seed>", seed 0 or 1 (NAMES).  `coo` is the entry list in
shuffled input order with the real values.  The kinds (KINDS):
  square      20 000 x 20 000, no repeated pair, CSR rows ascending: the control (COLSWEEP's serial-bits promise applies)
  repeats     20 000 x 50 000          wide   9 000 x 200 001: rows in stretches of 700, every fourth stretch scatters its far
  tall        30 000 x 17 000                 entries over all columns, the others keep them within 30 000 of the diagonal, so
                                              1024-entry tiles are a mix of spans below and above 65536
  block       rows [27 001, 52 001) of a 50 000-column matrix: first_row is no multiple of 8192, the last windows are clipped
              at `cols`, the diagonal leaves the matrix at local row 22 999
  block_low   rows [3 000, 12 000), 70 001 columns: the first window is clipped at column 0
  block_off   9 000 rows, 50 000 columns, first_row = 2 147 000 000: every window is empty, every entry far

Ingredients (the diagonal of local row r is column first_row + r; an ingredient leaves out what falls outside [0, cols)):
  band        0 ... 9 entries per row within 600 of the diagonal
  band edge   60 rows and the first and last row of every K6 row block with an entry at each of -4097, -4096, +4096, +4097 from
              the diagonal; 50 entries each in columns 0, cols - 1, 16383 and 16384
  far         1.2 entries per row anywhere (`wide`: see above)
  long rows   48 rows of 17 ... 300 entries within 4000 of the diagonal (16 of them in the first K6 block); rows of 33, 64, 65
              and 1024 far entries (a wavefront sums them); one row of 1500 far entries (above kBinRowCap: it stays near, outside
              the window); one row of 20 000 entries anywhere (above kOwnerMaxRow: AUTO resolves to STREAM_CARRY)
  repeats     3 % of the entries a second time with another value, elsewhere in the input order; one pair PAIR_EXTRA + rows
              times, so that its column holds more entries than the matrix has rows and tjds_from_coo reports num_diag > rows
  unsorted    csr_of() keeps the input order inside a row (a stable sort by row alone), so ties stay in input order and the
              columns of a row come as shuffled.  smvp_csr_from_coo sorts a row's columns: it is what `square` uses, and what
              transposing a handle twice must give back.

Operands (operands(name, "exact" | "real") -> (coo with those values, x of `cols`, x_rows of `rows`)):
  exact   val integers of magnitude 1 ... 1024, x integers of magnitude 1 ... 2^20, random signs, never zero: every product and
          every partial sum in any order is an integer below 2^53 (asserted), so every path -- TJDS ATOMIC and the column parts
          included -- must give the int64 reference (adopted.reference / reference_t) bit for bit
  real    val uniform in (-1, 1) times 10^k, k = -8 ... 7, x standard normal (the values of _fuzz_matrix): parity.check_y, and
          bits where the header promises them -- there the order of a column's ties shows
"""
import functools
import zlib

import numpy as np

import adopted
import parity
import smvp_toolkit_amd as sm
import special_values as sv

K6_ROWS, K6_BAND = sv.NW_ROW_BLOCK, sv.NW_BAND        # 8192, 4096
NW_SHORT_CAP, NW_LONG_CAP = 16, 1024                  # kNwShortCap, kNwLongCap
LONG_ROW = 32                                         # kLongRow
OWNER_MAX_ROW = 16 * 1024                             # kOwnerMaxRow
TILE, SPAN16 = 1024, adopted.SPAN16
EDGE_OFFSETS = (-4097, -4096, 4096, 4097)
PAIR_EXTRA = 50
FAR_ROWS = (33, 64, 65, 1024)                         # far entries of the rows a wavefront sums in pass B: 1024 = kBinRowCap
WIDE_STRETCH, WIDE_PERIOD, WIDE_NARROW_FAR = 700, 4, 30_000

#                 rows    cols     first_row      repeats
KINDS = {
    "square":    (20_000, 20_000,  0,             False),
    "repeats":   (20_000, 50_000,  0,             True),
    "wide":      (9_000,  200_001, 0,             True),
    "tall":      (30_000, 17_000,  0,             True),
    "block":     (25_000, 50_000,  27_001,        True),
    "block_low": (9_000,  70_001,  3_000,         True),
    "block_off": (9_000,  50_000,  2_147_000_000, True),
}
SEEDS = (0, 1)
NAMES = tuple("%s:%d" % (k, s) for k in KINDS for s in SEEDS)
WHOLE = tuple(n for n in NAMES if KINDS[n.split(":")[0]][2] == 0)          # first_row == 0: the TJDS side, the converters
BLOCKS = tuple(n for n in NAMES if n not in WHOLE)


def kind_of(name):
    return name.split(":")[0]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------------------------- the generator
def _far_columns(rng, d, cols, n):
    """n distinct columns further than 4096 from the diagonal column d (which may lie outside the matrix)."""
    lo_end, hi_start = int(np.clip(d - K6_BAND, 0, cols)), int(np.clip(d + K6_BAND + 1, 0, cols))
    cand = np.concatenate([np.arange(0, lo_end), np.arange(hi_start, cols)])
    return rng.choice(cand, size=n, replace=False)


@functools.lru_cache(maxsize=None)
def structure(name):
    """(rows, cols, first_row, coo): see the head of the file.  Deterministic: a second call of a fresh process gives the same
    bytes (test_mixed_structures_host.py builds it twice, past the cache)."""
    return _generate(name)


def _generate(name):
    kind, seed = name.split(":")
    rows, cols, row0, repeats = KINDS[kind]
    rng = np.random.default_rng([zlib.crc32(kind.encode()), int(seed)])
    r_all = np.arange(rows, dtype=np.int64)
    diag = row0 + r_all
    inside = (diag >= 0) & (diag < cols)
    anywhere = ((r_all // WIDE_STRETCH) % WIDE_PERIOD == 0) if kind == "wide" else np.ones(rows, dtype=bool)
    R, C = [], []

    def add(r, c):
        r, c = np.asarray(r, dtype=np.int64).reshape(-1), np.asarray(c, dtype=np.int64).reshape(-1)
        keep = (c >= 0) & (c < cols)
        R.append(r[keep])
        C.append(c[keep])

    # band
    r = np.repeat(r_all, rng.integers(0, 10, rows))
    add(r, diag[r] + rng.integers(-600, 601, len(r)))
    # band edge: around the diagonal (the first and last row of every K6 block among them), and the fixed columns
    ends = np.unique(np.concatenate([np.arange(0, rows, K6_ROWS), np.minimum(np.arange(0, rows, K6_ROWS) + K6_ROWS - 1, rows - 1)]))
    for off in EDGE_OFFSETS:
        cand = np.flatnonzero((diag + off >= 0) & (diag + off < cols))
        if len(cand):
            pick = np.union1d(rng.choice(cand, size=min(60, len(cand)), replace=False), np.intersect1d(ends, cand))
            add(pick, diag[pick] + off)
    for c in (0, cols - 1, sv.BIN_COL_BLOCK - 1, sv.BIN_COL_BLOCK):
        if 0 <= c < cols:
            add(rng.choice(np.flatnonzero(anywhere), size=50, replace=False), np.full(50, c))
    # far scatter
    r = rng.integers(0, rows, int(1.2 * rows))
    c = rng.integers(0, cols, len(r))
    if kind == "wide":
        off = rng.integers(K6_BAND + 1, WIDE_NARROW_FAR, len(r)) * rng.choice([-1, 1], len(r))
        off = np.where((diag[r] + off < 0) | (diag[r] + off >= cols), -off, off)
        c = np.where(anywhere[r], c, diag[r] + off)
    add(r, c)
    # long rows: distinct rows, none of them a K6 block's first or last row
    free = np.ones(rows, dtype=bool)
    free[ends] = False

    def take(mask, n):
        pick = rng.choice(np.flatnonzero(mask & free), size=n, replace=False)
        free[pick] = False
        return pick

    roomy = inside & (diag >= 4000) & (diag < cols - 4000)
    if roomy.any():
        near_rows = np.concatenate([take(roomy & (r_all < K6_ROWS), 16), take(roomy, 32)])
        lens = rng.integers(17, 301, len(near_rows))
        lens[:4] = (17, 32, 33, 300)
        for r, n in zip(near_rows, lens):
            add(np.full(n, r), diag[r] + rng.choice(np.arange(-4000, 4001), size=n, replace=False))
    far_rows = {int(take(anywhere, 1)[0]): n for n in FAR_ROWS}
    r = int(take(anywhere, 1)[0])
    add(np.full(1500, r), _far_columns(rng, int(diag[r]), cols, 1500))
    r = int(take(anywhere, 1)[0])
    add(np.full(20_000, r), rng.permutation(cols)[:20_000] if cols >= 20_000 and not repeats else rng.integers(0, cols, 20_000))

    r, c = np.concatenate(R), np.concatenate(C)
    if not repeats:                                                   # `square`: every pair once
        flat = np.unique(r * cols + c)
        r, c = flat // cols, flat % cols
    else:
        again = np.flatnonzero(rng.random(len(r)) < 0.03)
        pr = int(take(inside if inside.any() else np.ones(rows, dtype=bool), 1)[0])
        pc = int(diag[pr] + 5) if inside.any() and 0 <= diag[pr] + 5 < cols else int(rng.integers(0, cols))
        r = np.concatenate([r, r[again], np.full(rows + PAIR_EXTRA, pr)])
        c = np.concatenate([c, c[again], np.full(rows + PAIR_EXTRA, pc)])
    # the rows of exactly 33, 64, 65 and 1024 far entries: whatever the ingredients above left there beyond the band goes, and
    # n far entries come in -- two of them copies of another where pairs repeat
    keep = ~(np.isin(r, list(far_rows)) & (np.abs(c - (row0 + r)) > K6_BAND))
    r, c = [r[keep]], [c[keep]]
    for fr, n in far_rows.items():
        fc = _far_columns(rng, int(diag[fr]), cols, n - 2 if repeats else n)
        r.append(np.full(n, fr))
        c.append(np.concatenate([fc, fc[:2]]) if repeats else fc)
    r, c = np.concatenate(r), np.concatenate(c)
    val = rng.uniform(-1, 1, len(r))
    val[val == 0] = 0.5
    val *= 10.0 ** rng.integers(-8, 8, len(r))
    order = rng.permutation(len(r))
    coo = sm.make_coo(r[order], c[order], val[order])
    _frozen(coo)
    return rows, cols, row0, coo


def csr_of(name, coo=None):
    """(row_ptr, col_ind, val) of the structure (or of `coo`, the same entries with other values): smvp_csr_from_coo's arrays on
    `square`; elsewhere the entries sorted by row alone, stable, so that a row holds its entries in input order."""
    rows = KINDS[kind_of(name)][0]
    coo = structure(name)[3] if coo is None else coo
    if not KINDS[kind_of(name)][3]:
        return sm.csr_from_coo(coo, rows)
    order = np.argsort(coo["row"], kind="stable")
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(coo["row"], minlength=rows))]).astype(np.int32)
    return row_ptr, np.ascontiguousarray(coo["col"][order], dtype=np.int32), np.ascontiguousarray(coo["val"][order], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=None)
def operands(name, kind):
    """(coo, x, x_rows): the structure's entries with the values of the operand set `kind`, the operand of y = A x and the one of
    y = A^T x."""
    rows, cols, row0, coo = structure(name)
    rng = np.random.default_rng([zlib.crc32(name.encode()), 1 if kind == "exact" else 2])
    if kind == "exact":
        val = adopted.int_values(rng, len(coo), 1, 1024)
        x, xr = adopted.int_values(rng, cols, 1, 1 << 20), adopted.int_values(rng, rows, 1, 1 << 20)
        out = sm.make_coo(coo["row"], coo["col"], val)
        per_row = np.bincount(out["row"], weights=np.abs(val) * np.abs(x[out["col"]]), minlength=rows)
        per_col = np.bincount(out["col"], weights=np.abs(val) * np.abs(xr[out["row"]]), minlength=cols)
        assert max(per_row.max(), per_col.max()) < 2.0 ** 53, "the exact operands' sums must stay below 2^53"
    else:
        assert kind == "real", kind
        out = coo.copy()
        x, xr = rng.standard_normal(cols), rng.standard_normal(rows)
    _frozen(out, x, xr)
    return out, x, xr


def reference(name, kind="exact"):
    """y = A x of the exact operands in int64 (adopted.reference), as doubles."""
    coo, x, _ = operands(name, kind)
    assert kind == "exact"
    return adopted.reference(*csr_of(name, coo), x)


def reference_t(name):
    """y = A^T x_rows of the exact operands in int64 (adopted.reference_t)."""
    coo, _, xr = operands(name, "exact")
    return adopted.reference_t(*csr_of(name, coo), xr, KINDS[kind_of(name)][1])


# ------------------------------------------------------------------------------------------------------------------ regime
def windows(rows, cols, row0):
    """[(wbase, wend)] of the K6 row blocks before clipping to [0, cols)."""
    return [(row0 + r0 - K6_BAND, row0 + r0 + K6_ROWS + K6_BAND) for r0 in range(0, rows, K6_ROWS)]


def near_mask(rows, row0, row_ptr, col_ind):
    row_of = sv.row_of_entries(row_ptr)
    return np.abs(np.asarray(col_ind, dtype=np.int64) - (row0 + row_of)) <= K6_BAND, row_of


@functools.lru_cache(maxsize=None)
def regime(name):
    """The numbers assert_regime's conditions are about, from the host alone."""
    rows, cols, row0, coo = structure(name)
    rp, ci, _ = csr_of(name)
    lens = np.diff(rp)
    near, row_of = near_mask(rows, row0, rp, ci)
    far_per_row = np.bincount(row_of[~near], minlength=rows)
    capped = far_per_row > parity.BIN_ROW_CAP
    near_per_row = np.where(capped, 0, np.bincount(row_of[near], minlength=rows))     # (a capped row is listed apart, outside the window)
    block_starts = np.arange(0, rows, K6_ROWS)
    g = {"rows": rows, "cols": cols, "first_row": row0, "nnz": len(coo), "k6_blocks": len(block_starts), "max_row": int(lens.max()),
         "far_share": float((~near).mean())}
    g.update(parity.binned_regime(rp, ci, cols, 0, row0=row0))
    g["long_near_rows"] = np.add.reduceat((near_per_row > NW_SHORT_CAP).astype(np.int64), block_starts).tolist()
    g["near_rows_above_32"] = int((near_per_row > LONG_ROW).sum())
    g["far_rows"] = sorted(int(n) for n in far_per_row[(far_per_row > LONG_ROW) & ~capped])
    d = ci.astype(np.int64) - (row0 + row_of)
    g["edge"] = {off: int((d == off).sum()) for off in EDGE_OFFSETS}
    g["edge_possible"] = {off: int(((row0 + np.arange(rows) + off >= 0) & (row0 + np.arange(rows) + off < cols)).sum()) for off in EDGE_OFFSETS}
    g["columns"] = {c: int((ci == c).sum()) for c in (0, cols - 1, sv.BIN_COL_BLOCK - 1, sv.BIN_COL_BLOCK) if 0 <= c < cols}
    flat = coo["row"].astype(np.int64) * cols + coo["col"]
    _, counts = np.unique(flat, return_counts=True)
    g["repeat_share"] = float((counts > 1).mean())
    g["most_copies"] = int(counts.max())
    g["num_diag"] = int(sm.tjds_from_coo(coo, rows, cols).num_diag)
    descends = np.zeros(rows, dtype=bool)
    inner = np.flatnonzero((np.diff(ci.astype(np.int64)) < 0) & (np.diff(row_of) == 0))
    descends[row_of[inner]] = True
    g["unsorted_share"] = float(descends[lens >= 2].mean())
    spans = ~adopted.narrow_tiles(rp[-1], ci, TILE)
    g["tiles"], g["narrow_share"], g["wide_share"] = len(spans), adopted.narrow_share(rp[-1], ci, TILE), float(spans.mean())
    w = windows(rows, cols, row0)
    g["clipped_low"] = sum(1 for wb, we in w if wb < 0 < we)
    g["clipped_high"] = sum(1 for wb, we in w if wb < cols < we)
    g["empty_windows"] = sum(1 for wb, we in w if we <= 0 or wb >= cols)
    g["diagonal_leaves_at"] = int(cols - row0) if 0 <= cols - row0 < rows else None
    edge_cols = ci[np.isin(d, EDGE_OFFSETS)]
    g["window_edges"] = sv.window_edges_in(edge_cols, rows, cols, row0)
    return g


def assert_regime(name):
    """Every structure reaches what it is there for; returns regime(name)."""
    g = regime(name)
    kind = kind_of(name)
    off_block = kind == "block_off"
    assert g["rows"] > K6_ROWS and g["k6_blocks"] >= 2, (name, g)
    assert 9_000 <= g["rows"] <= 30_000 and 17_000 <= g["cols"] <= 200_001 and g["nnz"] <= 400_000, (name, g)
    assert g["ncb"] >= 2 and g["nrb"] >= 2 and g["cells"] >= 2 and g["runs"] >= 2 and g["long_rows"] >= 3, (name, g)
    assert g["far_rows"] == list(FAR_ROWS), (name, g)
    assert g["max_row"] > OWNER_MAX_ROW, (name, g)
    if not off_block:
        assert g["capped_rows"] >= 1, (name, g)
        assert max(g["long_near_rows"]) >= 10 and max(g["long_near_rows"]) <= NW_LONG_CAP and g["near_rows_above_32"] >= 10, (name, g)
    for off in EDGE_OFFSETS:
        assert g["edge"][off] >= min(50, g["edge_possible"][off]), (name, off, g)
    assert off_block or all(g["edge_possible"][off] >= 50 for off in EDGE_OFFSETS), (name, g)
    assert all(n >= 50 for n in g["columns"].values()) and len(g["columns"]) == 4, (name, g)
    if kind == "square":
        assert g["repeat_share"] == 0 and g["most_copies"] == 1 and g["unsorted_share"] == 0 and g["num_diag"] <= g["rows"], (name, g)
    else:
        assert g["repeat_share"] >= 0.01 and g["most_copies"] >= g["rows"] + PAIR_EXTRA and g["num_diag"] > g["rows"], (name, g)
        assert g["unsorted_share"] >= 0.3, (name, g)
    if kind == "wide":
        assert g["narrow_share"] >= 0.5 and g["wide_share"] >= 0.1, (name, g)
    found, wanted = g["window_edges"]
    assert found == wanted, (name, g)
    if kind == "tall":
        assert g["empty_windows"] >= 1, (name, g)
    if kind == "block":
        assert g["first_row"] % K6_ROWS and g["clipped_high"] >= 1 and g["clipped_low"] == 0 and g["diagonal_leaves_at"] == 22_999, (name, g)
        assert wanted == [True, True], (name, g)
    if kind == "block_low":
        assert g["first_row"] % K6_ROWS and g["clipped_low"] == 1 and g["clipped_high"] == 0 and wanted == [True, True], (name, g)
    if off_block:
        assert g["empty_windows"] == g["k6_blocks"] and g["far_share"] == 1.0 and wanted == [False, False], (name, g)
    return g
