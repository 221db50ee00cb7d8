"""What the timed entry points (smvp_csr_compute / smvp_tjds_compute) are held to on every device-timed form of the tile kernel:
the launch arithmetic, the structures named by the tile count they produce, the operands, the edge structures, the times.

Plain functions (no fixtures): test_gpu_timed_runs.py uses them on the GPU, test_timed_runs_host.py tests them on the host.

A device-timed run goes through one of two forms of the tile kernel that a handle's spmv never launches: the repeating kernel
csr_stream_owner_repeat<VPT, FLAVOR> (one launch for up to 1024 products, a barrier between two products whose width goes by the
grid: one level up to 24 workgroups, 8 shards up to 640, 16 beyond) and the stamped single launch csr_stream_owner<.., true>
replayed from a hipGraph in rings of 256.  Which one, and how wide a barrier, is decided by the number of tiles alone, so the
structures here are named by that number and sized for the tile in use.
"""
import zlib

import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm

# ---------------------------------------------------------------------------------------------------------- launch arithmetic
# Mirrors of csrc/smvp_tile_map.h (tile_group_of, tile_grid_of), smvp_kernels.h (kStreamTileGroup, kTjdsTileGroup) and the shard
# rule of launch_csr_stream_owner_repeat (smvp_owner.hip).
WANTED_GROUP = {"csr": 64, "tjds": 32}
TILES = (256, 1024, 2048)
REPEAT_RING, GRAPH_RING = 1024, 256        # products per repeating launch / per graph replay (smvp_run.hip)
# (vpt, flavor) of the instantiations of csr_stream_owner_repeat (SMVP_OWNER_REPEAT_FORMS, smvp_owner_kernel.h); flavours as in smvp_kernels.h
CSR, TJDS_K, TJDS_S, TJDS_H, CSR16 = 0, 2, 3, 4, 5
REPEAT_FORMS = frozenset([(1, CSR), (4, CSR), (8, CSR), (4, CSR16), (8, CSR16), (1, TJDS_S), (4, TJDS_S), (8, TJDS_S),
                          (1, TJDS_H), (4, TJDS_H), (8, TJDS_H)])


def tile_group_of(ntiles, wanted):
    fit = ntiles // 64
    return 1 if fit < 1 else min(fit, wanted)


def tile_grid_of(ntiles, group):
    return (ntiles + 8 * group - 1) // (8 * group) * 8 * group


def shards_of(grid):
    return 1 if grid <= 24 else 8 if grid <= 640 else 16


def default_tile(nnz, fmt):
    """Entries per tile the plan picks when nobody names one (choose_csr_kernel): 256 below 512 K entries, else 1024 -- and 2048
    for a TJDS stream of 12 M entries or more, which no structure here reaches."""
    if nnz < 512 * 1024:
        return 256
    return 2048 if fmt == "tjds" and nnz >= 12 * 1024 * 1024 else 1024


def regime(nnz, tile, fmt):
    """{ntiles, group, grid, shards, members}: the launch of a matrix of nnz entries in tiles of `tile`; members[s] = workgroups
    that count on shard s of the repeating kernel's barrier (one entry, the grid, for the one-level barrier)."""
    ntiles = max(1, -(-int(nnz) // tile))
    group = tile_group_of(ntiles, WANTED_GROUP[fmt])
    grid = tile_grid_of(ntiles, group)
    s = shards_of(grid)
    return {"ntiles": ntiles, "group": group, "grid": grid, "shards": s, "members": [(grid - sh + s - 1) // s for sh in range(s)]}


def ceil_div(a, b):
    return -(-a // b)


# -------------------------------------------------------------------------------------------------------------- structures
# name -> (tiles, grid, shards): what the structure must produce, for CSR and for TJDS alike (below 2048 tiles the two groups agree)
NAMED = {"t1": (1, 8, 1), "t24": (24, 24, 1), "t25": (25, 32, 8), "t640": (640, 640, 8), "t641": (641, 720, 16), "t705": (705, 792, 16)}
COLS = 50021                            # <= 60000: every tile's columns fit 16-bit offsets from the tile's smallest
LENGTH_MIX = (1, 0, 2, 3, 7, 33, 200)   # one cycle: 246 entries in 7 rows
LONG_ROW = 3000


def row_lengths(nnz):
    """Row lengths that sum to exactly nnz: two empty rows, cycles of LENGTH_MIX, after the first cycle one row of LONG_ROW (where
    nnz has room for it: it then crosses the edges of every tile size), a last row that takes what is left, three empty rows."""
    lens = [0, 0]
    left = nnz
    cycle = sum(LENGTH_MIX)
    if left >= cycle:
        lens += LENGTH_MIX
        left -= cycle
    if left >= LONG_ROW + cycle:
        lens.append(LONG_ROW)
        left -= LONG_ROW
    full = left // cycle
    lens += list(LENGTH_MIX) * full
    left -= full * cycle
    for l in LENGTH_MIX:                # the last, cut cycle
        take = min(l, left)
        lens.append(take)
        left -= take
    assert left == 0 and sum(lens) == nnz
    while len(lens) > 2 and lens[-1] == 0:
        lens.pop()                      # the last row with entries ends at nnz ...
    return np.array(lens + [0, 0, 0], dtype=np.int64)   # ... and empty rows follow it


def pattern(lens, cols, seed):
    """(row_ptr, col_ind) for these row lengths: every row's columns ascending and distinct inside [0, cols) -- an arithmetic run
    base + k * step with a step and a base of the row's own."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max(initial=0) <= cols
    row_ptr = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    step = rng.integers(1, np.minimum(97, np.maximum(1, (cols - 1) // np.maximum(lens - 1, 1))) + 1)
    base = rng.integers(0, cols - (np.maximum(lens, 1) - 1) * step)
    row_of = np.repeat(np.arange(len(lens)), lens)
    k = np.arange(int(row_ptr[-1])) - row_ptr[row_of]
    col_ind = base[row_of] + k * step[row_of]
    return row_ptr.astype(np.int32), col_ind.astype(np.int32)


def structure(name, tile):
    """(rows, cols, row_ptr, col_ind) of the structure NAMED[name] for tiles of `tile` entries: ceil(nnz / tile) is the named
    tile count, and nnz is no multiple of the tile (the last tile is cut) except for t1, which fills its one tile to the brim."""
    tiles = NAMED[name][0]
    nnz = tile if tiles == 1 else (tiles - 1) * tile + tile // 2 + 3
    lens = row_lengths(nnz)
    row_ptr, col_ind = pattern(lens, COLS, zlib.crc32(("%s/%d" % (name, tile)).encode()))
    return len(lens), COLS, row_ptr, col_ind


# ---------------------------------------------------------------------------------------------------------------- operands
def exact_operands(nnz, cols, seed=1):
    """val in -3 ... 3 and x in -4 ... 4 as doubles: every product and every partial sum of a row is an integer far below 2^53,
    so every order of summation gives the same bits."""
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, nnz).astype(np.float64), rng.integers(-4, 5, cols).astype(np.float64)


def real_operands(nnz, cols, seed=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, nnz), rng.random(cols)


def exact_reference(row_ptr, col_ind, val, x):
    """The product of exact operands as an int64 dot product per row, converted to double: +0.0 for an empty row and for a row
    whose products cancel."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    nnz = int(row_ptr[-1])
    v, xi = np.asarray(val)[:nnz].astype(np.int64), np.asarray(x).astype(np.int64)
    assert np.array_equal(v, np.asarray(val)[:nnz]) and np.array_equal(xi, x), "exact operands are integers"
    run = np.concatenate([[0], np.cumsum(v * xi[np.asarray(col_ind)[:nnz]])])
    return (run[row_ptr[1:]] - run[row_ptr[:-1]]).astype(np.float64)


def coo_of(row_ptr, col_ind, val):
    return sm.make_coo(np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr)), col_ind, val)


def row_scale(row_ptr, col_ind, val, x):
    return ob.csr_spmv(row_ptr, col_ind, np.abs(val), np.abs(x))


# --------------------------------------------------------------------------------------------------------- edge structures
# the small ones of test_gpu_parity.EDGE_CASES, and three of this module's own
EDGE_FROM_PARITY = ("empty_matrix", "single_entry", "leading_and_trailing_empty_rows", "all_rows_empty_but_one",
                    "row_ending_exactly_on_tile_edges", "rows_just_past_a_tile_edge", "wide_rectangular", "tall_rectangular")
EDGE_OWN = {
    "no_rows": ([], 5),                        # 0 x 5: no product launches anything
    "one_row_of_16384": ([16384], 20000),      # the longest row AUTO leaves to STREAM
    "one_row_of_16385": ([16385], 20000),      # AUTO takes STREAM_CARRY, which has no stamped form
}
EDGES = EDGE_FROM_PARITY + tuple(EDGE_OWN)
OWNER_MAX_ROW = 16 * 1024                      # kOwnerMaxRow (smvp_engine.hip)


def edge(name):
    """(rows, cols, row_ptr, col_ind, val, x) of an edge structure, values uniform in [-1, 1) and x in [0, 1)."""
    import test_gpu_parity as gp

    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lens, cols = EDGE_OWN[name] if name in EDGE_OWN else gp.EDGE_CASES[name](rng)
    row_ptr, col_ind, val = gp.csr_from_lengths(rng, list(lens), cols)
    return len(lens), cols, row_ptr, col_ind, val, rng.random(cols)


def device_timing_is_refused(name, path):
    """Whether explicit TIMING_DEVICE must be refused (SMVP_ERR_UNSUPPORTED) for this edge structure on this path ("csr_auto",
    "csr_stream" = STREAM at 1024, "tjds"), from csr_stamp_slots / tjds_stamp_slots: the tile kernel STREAM can stamp its launch,
    STREAM_CARRY -- AUTO's choice for a row of more than 16384 entries -- cannot, and a matrix without rows launches nothing, so
    there is nothing that could stamp."""
    lens = EDGE_OWN[name][0] if name in EDGE_OWN else None
    if name == "no_rows":
        return True
    return path == "csr_auto" and lens is not None and max(lens) > OWNER_MAX_ROW


# ------------------------------------------------------------------------------------------------------------------- times
def check_times(ms, st, info, iters, positive=True):
    """What the per-product times of a run must be, whatever the timing form (section (c) of the suite): one per product, finite,
    positive (positive=False: not negative -- a run whose products launch nothing), none longer than the loop's wall time, and the
    statistics are those of the times.  Tolerances: a sum of at most 2049 positive doubles carries at most 2049 * 2^-53 ~ 2.3e-13
    of relative rounding, so 1e-12; the standard deviation 1e-12 of the mean, absolutely.  Device-timed: every time is a whole
    number of ticks of the device's wall clock -- below about 1e7 ticks, so the two roundings (ticks / kHz, ms * kHz) move it
    by less than 1e-6 of a tick."""
    ms = np.asarray(ms)
    assert len(ms) == iters, (len(ms), iters)
    assert np.all(np.isfinite(ms)), ms[~np.isfinite(ms)][:4]
    assert np.all(ms > 0) if positive else np.all(ms >= 0), ms[ms <= 0][:4]
    assert ms.max() <= info.wall_ms, (ms.max(), info.wall_ms)
    for got, want in ((st.time_total, ms.sum()), (st.time_avg, ms.mean()), (st.time_min, ms.min()), (st.time_max, ms.max())):
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    assert abs(st.time_stdev - ms.std()) <= 1e-12 * ms.mean(), (st.time_stdev, ms.std())
    if info.timing == sm.TIMING_DEVICE:
        assert info.device_clock_khz > 0
        ticks = ms * info.device_clock_khz
        assert np.all(np.abs(ticks - np.rint(ticks)) <= 1e-6) and np.all(np.rint(ticks) >= 1), ticks[:8]
    if info.repeat_launches > 0:       # windows between the barriers of one launch cannot overlap
        assert ms.sum() <= info.wall_ms, (ms.sum(), info.wall_ms)
