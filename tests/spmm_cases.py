"""The constructed structures and operands of the block products' tests (smvp_csr_spmm, K7, and smvp_tjds_spmm, K10), a numpy
model of one row group's loop of csr_spmm_rows with the faults the structures are meant to catch, and the assertions both the
GPU tests and the host test call.  Plain functions over numpy alone (no fixtures, no library, no device):
test_gpu_spmm.py and test_gpu_tjds_spmm.py run them on the GPU, test_spmm_cases_host.py holds each structure to what it is
for and shows that every fault of the model is rejected.

Both kernels share their launch arithmetic: a group of G lanes (G = 1, 2, 4, 8, 16) per row, 256 / G rows per workgroup,
workgroups dealt to the XCDs in rounds of 8 * group, rows ordered by length inside blocks of BLOCK_ROWS, entries taken BATCH
at a time with the unused slots of a row's last batch clamped to the row's last entry and left out of the sum.
"""
import numpy as np

GROUPS = (1, 2, 4, 8, 16)          # lanes per row of a pass
BATCH = 8                          # entries per batch (kSpmmU, kTjdsSpmmU)
BLOCK_ROWS = 4096                  # rows per sorted block (kSpmmBlockRows)
WORKGROUP = 256                    # threads per workgroup
MAX_VECTORS = 16                   # vectors per pass (kSpmmMaxVectors)


def first_pass_group(k):
    """G of the first pass of a product with k vectors: the smallest power of two >= min(k, 16)."""
    g = 1
    while g < min(k, MAX_VECTORS):
        g <<= 1
    return g


def _csr_of_lists(lists):
    row_ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    col_ind = np.concatenate([np.asarray(l, dtype=np.int64) for l in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    return row_ptr, col_ind


# ------------------------------------------------------------------------------------------------------------ structures
RAGGED_STARTS = (0, 9)


def ragged(g, start):
    """(rows, cols, row_ptr, col_ind, val, X): 3 * (64 / g) + 1 rows -- three wavefronts' worth of groups of g lanes and one row
    more -- of 40 columns; row r has (r + start) % 18 entries in sorted distinct columns, so neighbouring groups of one wavefront
    make a different number of batch trips.  X has g vectors.  The two starts together give every length 0 ... 17 for every g
    (13 rows at g = 16)."""
    rows, cols = 3 * (64 // g) + 1, 40
    rng = np.random.default_rng(6400 + 32 * g + start)
    lists = [np.sort(rng.choice(cols, (r + start) % 18, replace=False)) for r in range(rows)]
    row_ptr, col_ind = _csr_of_lists(lists)
    return rows, cols, row_ptr, col_ind, rng.uniform(-1, 1, len(col_ind)), rng.standard_normal((cols, g))


def slot_case():
    """(rows, cols, row_ptr, col_ind, val, last_col): 180 rows of 4000 columns, row r with 1 + r % 17 sorted distinct columns,
    every value in [0.5, 1.5); last_col[r] is the column of row r's last entry -- the one the last batch re-reads in its unused
    slots."""
    rows, cols = 180, 4000
    rng = np.random.default_rng(6700)
    lists = [np.sort(rng.choice(cols, 1 + r % 17, replace=False)) for r in range(rows)]
    row_ptr, col_ind = _csr_of_lists(lists)
    return rows, cols, row_ptr, col_ind, rng.uniform(0.5, 1.5, len(col_ind)), col_ind[row_ptr[1:] - 1].astype(np.int64)


def slot_operand(k, last_col, cols=4000):
    """X (cols x k) uniform in [0.5, 1) with +Inf in vector k - 1 at the last column of every third row: such a row sums to
    +Inf, and a kernel that multiplied its unused slots by 0.0 would add 0 * Inf = NaN to it."""
    X = np.random.default_rng(6710 + k).uniform(0.5, 1.0, (cols, k))
    X[last_col[::3], k - 1] = np.inf
    return X


# the multiples of 256 / G (workgroup), of 8 * 256 / G (one round of workgroups over the XCDs) and of BLOCK_ROWS with their
# neighbours, and one count inside a third block
ROW_COUNTS = (1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
              2049, 4095, 4096, 4097, 8191, 8192, 8193, 12289)
ROW_COUNT_KS = (1, 2, 3, 4, 8, 16)          # every G; k = 3 is a pass with an idle lane per group
ROW_COUNT_COLS = 97


def row_count_case(rows):
    """(rows, cols, row_ptr, col_ind, val, X): row r has (7 r) % 11 entries in the columns (r + 13 j) % 97, j = 0, 1, ... --
    distinct (13 and 97 are coprime) and not sorted: the product sums in storage order.  The last row holds at least one entry,
    so a last row that is never written shows.  X has 16 vectors; a test with k vectors takes the first k."""
    cols = ROW_COUNT_COLS
    lens = (7 * np.arange(rows, dtype=np.int64)) % 11
    lens[-1] = max(int(lens[-1]), 1)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), lens)
    j = np.arange(int(row_ptr[-1]), dtype=np.int64) - row_ptr[:-1].astype(np.int64)[row_of]
    col_ind = ((row_of + 13 * j) % cols).astype(np.int32)
    rng = np.random.default_rng(6800 + rows)
    return rows, cols, row_ptr, col_ind, rng.uniform(-1, 1, len(col_ind)), rng.standard_normal((cols, MAX_VECTORS))


FUZZ_SEEDS = tuple(range(25))
FUZZ_MAX_ROWS = 13107                       # about 3.2 blocks of 4096 rows
FUZZ_MAX_ENTRIES = 400_000                  # one GPU case stays well under a second of device time
FUZZ_SMALL_KS = (1, 2, 3, 4, 7, 8)


def block_fuzz(seed):
    """(rows, cols, row_ptr, col_ind, val, k, ldx, ldy, X): random shape and skew in the five row-length styles of
    test_gpu_parity._fuzz_matrix (short, power law, mostly empty, a few huge rows, uniform), with up to about 3.2 sorted blocks
    of rows, k from 1 to 40 (every other seed from the small values, so that every G of a first pass occurs), ldx and ldy each
    k plus 0 ... 8, values and X spread over several decades."""
    rng = np.random.default_rng(7102 + seed)
    rows = int(rng.integers(1, FUZZ_MAX_ROWS + 1))
    cols = int(rng.integers(1, 6000))
    style = seed % 5
    if style == 0:
        lens = rng.integers(0, 6, rows)
    elif style == 1:
        lens = np.minimum((rng.pareto(1.2, rows) * 3).astype(np.int64), 2000)
    elif style == 2:
        lens = np.where(rng.random(rows) < 0.7, 0, rng.integers(1, 40, rows))
    elif style == 3:
        lens = rng.integers(0, 3, rows)
        lens[rng.integers(0, rows, 3)] = int(rng.integers(1500, 5000))
    else:
        lens = np.full(rows, int(rng.integers(1, 30)))
    lens = np.minimum(lens, cols).astype(np.int64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col_ind = np.concatenate([np.sort(rng.choice(cols, int(l), replace=False)) if l else np.zeros(0, np.int64) for l in lens] +
                             [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.uniform(-1, 1, len(col_ind)) * 10.0 ** rng.integers(-8, 8, len(col_ind))
    k = int(rng.choice(FUZZ_SMALL_KS)) if seed % 2 else int(rng.integers(1, 41))
    ldx, ldy = k + int(rng.integers(0, 9)), k + int(rng.integers(0, 9))
    X = rng.standard_normal((cols, k)) * 10.0 ** rng.integers(-3, 3, (cols, k))
    return rows, cols, row_ptr, col_ind, val, k, ldx, ldy, X


# ------------------------------------------------------------------------------------------------------- the batch model
FAULTS = ("zero_mask", "drop_tail", "next_entry", "lost_block")


def batch_model(row_ptr, col_ind, val, X, fault=None):
    """Y = A X the way one row group of csr_spmm_rows sums it, all rows at once: batches of BATCH entries, the unused slots of a
    row's last batch clamped to entry z - 1 and left out, each product rounded and then added in entry order.  Y starts as NaN,
    as the tests' Y does.  Faults:
      zero_mask   the unused slots are multiplied by 0.0 and added instead of being skipped
      drop_tail   a row's last, partial batch is left out
      next_entry  the unused slots read the entries z, z + 1, ... (the next row's; none past the last entry) and are added
      lost_block  the rows of the last, partial block of BLOCK_ROWS are never written"""
    assert fault is None or fault in FAULTS
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col_ind, val, X = np.asarray(col_ind, dtype=np.int64), np.asarray(val, dtype=np.float64), np.asarray(X, dtype=np.float64)
    rows, k, nnz = len(row_ptr) - 1, X.shape[1], int(row_ptr[-1])
    a, z = row_ptr[:-1], row_ptr[1:]
    acc = np.zeros((rows, k))
    with np.errstate(invalid="ignore", over="ignore"):
        for j0 in range(0, int((z - a).max()) if rows else 0, BATCH):
            live = np.flatnonzero(a + j0 < z)
            j = a[live] + j0
            if fault == "drop_tail":
                keep = j + BATCH <= z[live]
                live, j = live[keep], j[keep]
            for u in range(BATCH):
                inside = j + u < z[live]
                if fault == "next_entry":
                    inside = j + u < nnz
                    jj = np.minimum(j + u, nnz - 1)
                else:
                    jj = np.where(inside, j + u, z[live] - 1)
                w = val[jj]
                if fault == "zero_mask":
                    w, inside = np.where(inside, w, 0.0), np.ones(len(live), bool)
                p = w[:, None] * X[col_ind[jj]]                              # rounded ...
                acc[live[inside]] = acc[live[inside]] + p[inside]            # ... then added
    Y = np.full((rows, k), np.nan)
    written = rows if fault != "lost_block" else rows // BLOCK_ROWS * BLOCK_ROWS
    Y[:written] = acc[:written]
    return Y


# ------------------------------------------------------------------------------------------------------------ assertions
def assert_bits(Y, ref, what=""):
    """Equality of bits on every element of a block, any NaN equal to any NaN."""
    Y, ref = np.ascontiguousarray(Y, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert Y.shape == ref.shape, "%s: shape %s against %s" % (what, Y.shape, ref.shape)
    ok = (Y.view(np.int64) == ref.view(np.int64)) | (np.isnan(Y) & np.isnan(ref))
    if not ok.all():
        r, v = np.argwhere(~ok)[0]
        raise AssertionError("%s: %d of %d elements differ from the serial loop's bits; first row %d, vector %d: %r against %r" % (
            what, (~ok).sum(), ok.size, r, v, Y[r, v], ref[r, v]))


def assert_slot_rows(Y, what=""):
    """What slot_operand makes of slot_case: no NaN, +Inf in every third row of the last vector, the vectors before it finite."""
    Y = np.asarray(Y)
    k = Y.shape[1]
    assert not np.isnan(Y).any(), "%s: NaN in row %d: an unused slot took part in the sum" % (what, np.argwhere(np.isnan(Y))[0][0])
    assert (Y[::3, k - 1] == np.inf).all(), "%s: a poisoned row of vector %d is not +Inf" % (what, k - 1)
    assert np.isfinite(Y[:, :k - 1]).all(), "%s: a vector beside the poisoned one is not finite" % what
