"""What the GPU parity tests check a product with: the row-wise error bound, the guarded y, the binned plan's regimes.

Plain functions (no fixtures): test_gpu_parity.py uses them on the GPU, test_parity_checks.py tests them on the host.

The bound.  A correct fp64 sum of a row's n products, in any order, lies within gamma_n * sum_j |a_rj x_j| of the exact
sum (gamma_n = n u / (1 - n u), u = 2^-53), and so does the serial loop the oracle runs: the two differ by at most
2 gamma_n * sum|a x|.  check_y allows 2 (n + 2) u * sum|a x|, and never more than the 1e-9 * sum|a x| of BASELINE.json,
so that dropping, doubling or misplacing one product shows up unless it is within a few ulps of the row's sum of terms.
"""
import numpy as np

TOL = 1e-9          # the normwise bound of BASELINE.json / SURVEY 8(c): no check is looser than this
U = 2.0 ** -53      # unit roundoff of fp64

# ------------------------------------------------------------------------------------------------------------- check_y
def bound(terms):
    """Allowed |y - ref| per unit of sum|a x| for a row of `terms` products."""
    return np.minimum(TOL, 2.0 * (np.asarray(terms, dtype=np.float64) + 2.0) * U)


def check_y(y, ref, scale, terms, exact=False):
    """y (the kernel's) against ref (the oracle's serial loop).  scale = sum_j |a_rj x_j| per row, terms = products per row
    (scalars broadcast).  Every row finite where ref is (a NaN left in y -- a row never written -- fails), within
    bound(terms) * scale; rows with scale == 0 (empty) equal ref exactly; rows where ref is not finite equal it.  exact: no NaN
    and the reference's bits, the sign of a zero included."""
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape, "y has shape %s, the reference %s" % (y.shape, ref.shape)
    if exact:
        bad = ~((y == ref) | (np.isnan(y) & np.isnan(ref)))
        assert np.array_equal(y, ref), "%d rows differ from the serial loop's bits; first row %d: %r against %r" % (
            bad.sum(), np.flatnonzero(bad)[0] if bad.any() else -1, y[bad][:1], ref[bad][:1])
        from transposed import assert_bits           # (its one copy; for np.array_equal -0.0 equals 0.0, and the serial loop never gives -0.0)

        assert_bits(y, ref, "rows that must have the serial loop's bits")
        return
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), ref.shape)
    terms = np.broadcast_to(np.asarray(terms, dtype=np.float64), ref.shape)
    lim = bound(terms) * scale
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        err = np.abs(y - ref)
        ok = np.where(fin, np.isfinite(y) & (err <= lim), (y == ref) | (np.isnan(y) & np.isnan(ref)))
    if ok.all():
        return
    bad = np.flatnonzero(~ok)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(np.isfinite(err[bad]), err[bad] / lim[bad], np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    r = int(bad[0])
    raise AssertionError("%d rows beyond 2 (terms + 2) 2^-53 sum|a x| (or non-finite); first bad row %d (%g terms): y %r, "
                         "ref %r, scale %r; worst |y - ref| / bound %g" % (len(bad), r, terms[r], y[r], ref[r], scale[r],
                                                                         ratio.max()))


# ------------------------------------------------------------------------------------------------------------ guarded y
G = 64                                  # guard doubles on either side: 512 bytes, so the view keeps the buffer's alignment
GUARD = np.int64(0x5A17C0DE0BADF00D)    # the guards' bit pattern (a finite double)


def guarded_y(torch, rows, device="cuda"):
    """(buffer, y): y is the view buffer[G:G + rows], filled with NaN; G doubles of GUARD on either side of it."""
    buf = torch.empty(rows + 2 * G, dtype=torch.float64, device=device)
    buf.view(torch.int64).fill_(int(GUARD))
    y = buf[G:G + rows]
    y.fill_(float("nan"))
    return buf, y


def check_guards(buf, rows):
    """The guards around a y of `rows` doubles, bit for bit: nothing written in front of row 0 or past the last row."""
    h = buf.cpu().numpy() if hasattr(buf, "cpu") else np.asarray(buf)
    h = np.ascontiguousarray(h).view(np.int64)
    assert h.shape == (rows + 2 * G,)
    front, back = h[:G] != GUARD, h[G + rows:] != GUARD
    assert not front.any(), "y written in front of row 0: %d guard words changed, nearest at row %d" % (
        front.sum(), np.flatnonzero(front)[-1] - G)
    assert not back.any(), "y written past its last row: %d guard words changed, first at row %d" % (
        back.sum(), rows + np.flatnonzero(back)[0])


# ---------------------------------------------------------------------------------------------- the binned plan's regimes
# Mirrors of smvp_kernels.h and build_binned_plan (smvp_binned.hip): kBinColBits, kBinSlots, kBinRowCap (the cap is
# slots / 8 there), the bucket slots - slots / 8, kBinShiftCap, kBinNearBand; q = min(64, max(1, ceil(112 ncb / bucket)));
# a far entry's row block = (far entries in front of its row) / bucket, its super block = row block / q, its column block =
# column >> kBinColBits (bin_keys).  Pass A's stream is grouped by column block and counts a cell per distinct super block in
# it (csr_binned_far_products reads the shift of cell >= kBinShiftCap from memory); pass B's stream is grouped by row block
# and counts a sub-run per distinct column block in it (csr_binned_far_sums, likewise); bin_far_rows_packed keeps the 32-bit
# far-row lists (fr_row / fr_ptr) when a row block's far rows span 65536 rows or more.
BIN_COL_BITS = 14
BIN_SLOTS = 8192
BIN_ROW_CAP = BIN_SLOTS // 8
BIN_BUCKET = BIN_SLOTS - BIN_ROW_CAP
BIN_SHIFT_CAP = 1024
BIN_NEAR_BAND = 4096
BIN_PACKED_SPAN = 1 << 16


def binned_regime(row_ptr, col_ind, cols, band=0, row0=0):
    """What the binned plan of (row_ptr, col_ind) at `band` (0: the default) builds, from the host: {nf, ncb, q, nrb,
    cells: most super blocks in one column block (pass A's cells), runs: most column blocks in one row block (pass B's
    sub-runs), span: widest row span of one row block's far rows, long_rows: far rows of more than 32 far entries,
    capped_rows: rows kept near for having more than BIN_ROW_CAP far entries}."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    rows = len(row_ptr) - 1
    lens = np.diff(row_ptr)
    row_of = np.repeat(np.arange(rows, dtype=np.int64), lens)
    far = np.abs(np.asarray(col_ind[:row_ptr[-1]], dtype=np.int64) - (row0 + row_of)) > (band if band > 0 else BIN_NEAR_BAND)
    per_row = np.bincount(row_of[far], minlength=rows)
    capped = per_row > BIN_ROW_CAP
    far &= ~capped[row_of]
    per_row[capped] = 0
    frp = np.concatenate([[0], np.cumsum(per_row)])
    nf = int(frp[-1])
    ncb = -(-int(cols) // (1 << BIN_COL_BITS))
    q = min(64, max(1, -(-112 * ncb // BIN_BUCKET)))
    out = {"nf": nf, "ncb": ncb, "q": q, "nrb": -(-nf // BIN_BUCKET), "cells": 0, "runs": 0, "span": 0,
           "long_rows": int((per_row > 32).sum()), "capped_rows": int(capped.sum())}
    if nf == 0:
        return out
    f_row = row_of[far]
    cb = np.asarray(col_ind[:row_ptr[-1]], dtype=np.int64)[far] >> BIN_COL_BITS
    rb = frp[f_row] // BIN_BUCKET
    nsb = -(-out["nrb"] // q)
    out["cells"] = int(np.bincount(np.unique(cb * nsb + rb // q) // nsb).max())
    out["runs"] = int(np.bincount(np.unique(rb * ncb + cb) // ncb).max())
    fr = np.flatnonzero(per_row)                          # far rows, ascending; their blocks are non-decreasing
    blk = frp[fr] // BIN_BUCKET
    first = np.flatnonzero(np.diff(blk, prepend=-1))
    last = np.append(first[1:], len(fr)) - 1
    out["span"] = int((fr[last] - fr[first]).max())
    return out


def binned_fits(nf, cols):
    """Whether build_binned_plan takes a matrix with nf far entries (binned_regime's nf: after the row cap) and `cols` columns:
    its streams of far products are addressed with 32-bit positions, nf plus up to 256 of padding for every column block,
    every row block and two more, and it refuses with SMVP_ERR_UNSUPPORTED where that passes 2147483000 (smvp_binned.hip)."""
    ncb = -(-int(cols) // (1 << BIN_COL_BITS))
    return int(nf) + 256 * (ncb + int(nf) // BIN_BUCKET + 2) <= 2147483000


SPILL_KINDS = ("cells", "runs", "fr32")


def spill_matrix(kind):
    """(rows, cols, band, row_ptr, col_ind, val): a matrix whose binned plan takes one of the paths past the plan's caps --
      cells  2^20 x 2^20, 12 uniform entries per row, band 1: nearly every entry far, 64 column blocks, q = 1, about 1756
             cells (super blocks) per column block: pass A reads the shifts of cells >= BIN_SHIFT_CAP from memory;
      runs   2^18 x 20 000 000, 32 uniform entries per row, band 1: 1221 column blocks, nearly all of them in every row block:
             pass B reads the shifts of sub-runs >= BIN_SHIFT_CAP from memory;
      fr32   2^20 x 2^20, default band: 3-7 entries per row within 3 of the diagonal, one entry more than 4096 columns away in
             every 50th row, a few far rows of 33 ... 1024 far entries (summed by a wavefront) and one row of 1500 (kept near):
             a row block's far rows span about 358 000 rows, so the plan keeps the 32-bit far-row lists."""
    import smvp_toolkit_amd as sm

    if kind == "cells":
        n = 1 << 20
        return (n, n, 1) + sm.synth_csr(sm.SYNTH_UNIFORM, 31, n, n, 12)
    if kind == "runs":
        rows, cols = 1 << 18, 20_000_000
        return (rows, cols, 1) + sm.synth_csr(sm.SYNTH_UNIFORM, 32, rows, cols, 32)
    assert kind == "fr32", kind
    rng = np.random.default_rng(33)
    n = 1 << 20
    lens = rng.integers(3, 8, n)
    pick = np.argsort(rng.random((n, 7)), axis=1) < lens[:, None]          # lens[r] distinct offsets out of -3 ... 3
    r_near, k = np.nonzero(pick)
    c_near = r_near + k - 3
    keep = (c_near >= 0) & (c_near < n)                                      # (the first and last rows lose a few)
    r_far = np.arange(0, n, 50)
    c_far = (r_far + rng.integers(4097, n - 4096, len(r_far))) % n          # |column - row| > 4096 either way round
    rs, cs = [r_near[keep], r_far], [c_near[keep], c_far]
    for r, k in ((100_001, 33), (300_007, 200), (500_003, 1024), (700_009, 1500)):
        rs.append(np.full(k, r))
        cs.append((r + 4097 + rng.choice(n - 8193, size=k, replace=False)) % n)
    r_all, c_all = np.concatenate(rs), np.concatenate(cs)
    order = np.lexsort((c_all, r_all))
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(r_all, minlength=n))]).astype(np.int32)
    return n, n, 0, row_ptr, c_all[order].astype(np.int32), rng.uniform(-1, 1, len(order))


def csr_from_lengths(rng, lens, cols):
    """(row_ptr, col_ind, val): lens[r] distinct ascending columns out of `cols` in row r, values uniform in (-1, 1)."""
    rows = len(lens)
    row_ptr = np.zeros(rows + 1, dtype=np.int32)
    np.cumsum(lens, out=row_ptr[1:])
    col_ind = np.concatenate([np.sort(rng.choice(cols, size=l, replace=False)) for l in lens] + [np.zeros(0, int)])
    val = rng.uniform(-1, 1, int(row_ptr[-1]))
    return row_ptr, col_ind.astype(np.int32), val


def corner_structures():
    """[(name, rows, cols, bands, row_ptr, col_ind, val, x)]: the binned plan where its bookkeeping is stressed --
      wide  6000 x 3 000 000 = 184 column blocks (more than a workgroup stages shifts for); rows of 0 ... 1500 entries: far rows
            longer than a wavefront's 32 (summed by a whole wavefront) and longer than the cap of 1024 (kept near), rows with only
            far / only near entries, empty rows, duplicate and unsorted columns, a rectangular matrix;
      tall  200 000 x 40 000: every column within a few blocks, many far rows per row block, stretches of rows without entries.
    `bands` are the bands each is multiplied at.  One generator draws both, in this order."""
    rng = np.random.default_rng(2024)
    rows, cols = 6000, 3_000_000
    lens = np.where(rng.random(rows) < 0.05, rng.integers(500, 1500, rows), rng.integers(0, 40, rows))
    lens[:3] = (0, 1, 33)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col_ind = rng.integers(0, cols, int(row_ptr[-1])).astype(np.int32)
    idx = np.arange(0, len(col_ind) - 1, 97)
    col_ind[idx] = col_ind[idx + 1]                               # some repeats (mostly inside rows)
    val = rng.uniform(-1, 1, len(col_ind))
    x = rng.random(cols)
    out = [("wide", rows, cols, (0, 5, 2_000_000), row_ptr, col_ind, val, x)]
    rows, cols = 200_000, 40_000
    lens = rng.integers(0, 9, rows)
    lens[50_000:90_000] = 0
    row_ptr, col_ind, val = csr_from_lengths(rng, lens.tolist(), cols)
    x = rng.random(cols)
    out.append(("tall", rows, cols, (16,), row_ptr, col_ind, val, x))
    return out


def assert_spill_regime(kind, rows, cols, band, row_ptr, col_ind):
    """The matrix of spill_matrix(kind) reaches its regime with at least 10 % to spare; returns binned_regime's numbers."""
    g = binned_regime(row_ptr, col_ind, cols, band)
    if kind == "cells":
        assert g["cells"] >= 1.1 * BIN_SHIFT_CAP, g
    elif kind == "runs":
        assert g["runs"] >= 1.1 * BIN_SHIFT_CAP, g
    else:
        assert g["span"] >= 1.1 * BIN_PACKED_SPAN and g["long_rows"] >= 3 and g["capped_rows"] == 1, g
    return g
