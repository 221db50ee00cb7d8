"""What the forward products y = A x are held to on non-finite, signed-zero, subnormal and overflowing operands: the
structures, the operands of scenarios A ... G, the conditions that keep a scenario from passing vacuously, the row classes.

Plain functions (no fixtures): test_gpu_special_values.py uses them on the GPU, test_special_values_host.py tests them -- and
numpy models of the wrong kernels they are meant to catch -- on the host.  The reference of every check is the oracle's serial
loop (ob.csr_spmv); two facts let paths that sum in another order be checked exactly too:

  row class   with every finite product small (|a x| <= 1e3, no partial sum overflows) the class of a row is the same for
              every order of summation: NaN if a product is NaN (a stored 0.0 times +-Inf included) or the row has both a
              +Inf and a -Inf product, else +Inf / -Inf if it has such a product, else finite (row_classes);
  exact sums  products that are integer multiples of one power of two, sums below 2^53 of those units: every order gives
              the same bits -- in the subnormal range too (scenario E), and for same-sign sums that overflow (F: partial
              sums of positive terms are monotone, so a row reaches +Inf in every order or in none).

The scenarios (ordinary / subnormal / overflowing / rounded build them, assert_regime holds each to its condition, the
assert_* functions at the end are what a product is held to in each):
  A  NaN / +Inf / -Inf in columns of x that no stored entry uses: y has the bits of the product with 0.0 there
  B  the same in referenced columns: classes exact, finite rows within parity.check_y's bound
  C  stored 0.0 / -0.0 values, some under +-Inf of x (the row is NaN), some under ordinary x (nothing changes)
  D  x = 0.0 and x = -0.0 everywhere, rows whose every product is -0.0, empty rows: y is +0.0 by bits everywhere
  E  subnormal values k 2^-1060 times small integers: exact, bits of the serial loop on every path
  F  products of exactly +-2^1020, one sign per row: n <= 15 of them sum to n 2^1020, n >= 16 overflow in every order
  G  full 53-bit mantissas: fma(a, x, acc) and round(a x) + acc differ in most rows (the serial-bits paths only)
"""
import zlib
from fractions import Fraction

import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm
from transposed import assert_bits as check_bits      # equality of the int64 views, any NaN equal to any NaN (one copy: transposed.py)

FINITE, PINF, NINF, NAN = 0, 1, 2, 3
CLASS_NAMES = ("finite", "+Inf", "-Inf", "NaN")
POISON = (np.nan, np.inf, -np.inf)
NEG_ZERO = np.int64(-2 ** 63)                         # the bits of -0.0

NW_ROW_BLOCK, NW_BAND = 8192, 4096                    # csr_near_window (smvp_kernels.h: kNwRowBlock, kNwBand)
BIN_COL_BLOCK = 1 << 14                               # the binned plan's column block (parity.BIN_COL_BITS)
MIN_COLS_A = 64                                       # scenario A needs room for 16 columns nobody uses


# ------------------------------------------------------------------------------------------------------------ row classes
def row_of_entries(row_ptr):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    return np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int64), np.diff(row_ptr))


def row_classes(row_ptr, col_ind, val, x):
    """FINITE / PINF / NINF / NAN per row, from the products alone (the rule above; no loop over rows)."""
    rows = len(row_ptr) - 1
    nnz = int(row_ptr[-1])
    row_of = row_of_entries(row_ptr)
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(val, dtype=np.float64)[:nnz] * np.asarray(x, dtype=np.float64)[np.asarray(col_ind)[:nnz]]
    has = lambda m: np.bincount(row_of[m], minlength=rows) > 0
    nan, pinf, ninf = has(np.isnan(p)), has(p == np.inf), has(p == -np.inf)
    out = np.full(rows, FINITE)
    out[pinf] = PINF
    out[ninf] = NINF
    out[nan | (pinf & ninf)] = NAN
    return out


def classes_of(y):
    y = np.asarray(y, dtype=np.float64)
    return np.where(np.isnan(y), NAN, np.where(y == np.inf, PINF, np.where(y == -np.inf, NINF, FINITE)))


def check_classes(y, classes, what=""):
    got = classes_of(y)
    bad = np.flatnonzero(got != classes)
    assert bad.size == 0, "%s: %d rows of the wrong class; first row %d is %s (%r), must be %s" % (
        what, bad.size, bad[0], CLASS_NAMES[got[bad[0]]], np.asarray(y)[bad[0]], CLASS_NAMES[classes[bad[0]]])


def check_no_negative_zero(y, what=""):
    bits = np.ascontiguousarray(y, dtype=np.float64).view(np.int64)
    bad = np.flatnonzero(bits == NEG_ZERO)
    assert bad.size == 0, "%s: -0.0 in %d rows (first %d): the serial loop starts from +0.0 and never gives it" % (
        what, bad.size, bad[0] if bad.size else -1)


def fma_serial(row_ptr, col_ind, val, x, rows):
    """The serial loop of the given rows with acc = fma(val, x, acc) (one rounding per step, exact rational arithmetic):
    the model of a kernel built without -ffp-contract=off."""
    out = np.zeros(len(rows))
    for i, r in enumerate(rows):
        acc = 0.0
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc = float(Fraction(float(val[j])) * Fraction(float(x[col_ind[j]])) + Fraction(acc))
        out[i] = acc
    return out


# ------------------------------------------------------------------------------------------------------------- structures
EDGE_NAMES = ("empty_matrix", "single_entry", "leading_and_trailing_empty_rows", "all_rows_empty_but_one", "row_spanning_many_tiles",
              "row_ending_exactly_on_tile_edges", "rows_just_past_a_tile_edge", "one_huge_row_between_short_ones", "many_short_rows",
              "mixed_skew", "wide_rectangular", "tall_rectangular", "exactly_33_per_row")
FUZZ_SEEDS = (0, 1, 2, 3, 4)                          # _fuzz_matrix's five styles
SMALL = tuple("edge:" + n for n in EDGE_NAMES) + tuple("fuzz:%d" % s for s in FUZZ_SEEDS) + (
    "memplus", "pwt", "straddle", "uniform32")
BIG = ("random_model", "fr32")                        # millions of rows: on the GPU only (the host suite checks the SMALL ones)
STRUCTURES = SMALL + BIG

# the structures that must meet a scenario's condition (assert_regime); the others are too small for it and only run
REGIME = {
    "A": tuple(s for s in STRUCTURES if s not in ("edge:empty_matrix", "edge:single_entry", "edge:leading_and_trailing_empty_rows",
                                                  "edge:tall_rectangular")),            # (those four have fewer than 64 columns)
    "B": ("edge:many_short_rows", "fuzz:0", "fuzz:4", "memplus", "pwt", "uniform32", "random_model", "fr32"),
    "C": ("edge:many_short_rows", "edge:mixed_skew", "edge:exactly_33_per_row", "fuzz:0", "fuzz:2", "fuzz:4", "memplus", "pwt", "straddle",
          "uniform32", "random_model", "fr32"),
    "D": ("edge:many_short_rows", "edge:mixed_skew", "edge:tall_rectangular", "fuzz:0", "fuzz:1", "fuzz:2", "fuzz:3", "straddle"),
    "G": ("edge:mixed_skew", "edge:wide_rectangular", "fuzz:1", "fuzz:2", "memplus", "pwt", "straddle", "uniform32"),
}

STRADDLE_LENS = [1, 14, 15, 16, 17, 31, 32, 33, 0, 255, 256, 257, 1023, 1024, 1025, 2, 0, 3] * 20   # 15 | 16, 32 | 33, tile edges


def unused_columns(rows, cols, row0=0):
    """Scenario A's set U for a matrix of this shape: column 0, the last column, the binned column-block edge (16383 | 16384),
    the column just in front of and just behind a csr_near_window window (row0 + R0 - 4096 ... row0 + R0 + 8192 + 4096), and
    others drawn from a seed up to 24; empty for matrices of fewer than MIN_COLS_A columns, which take no part in scenario A."""
    if cols < MIN_COLS_A:
        return np.zeros(0, dtype=np.int64)
    forced = {0, cols - 1}
    if cols > BIN_COL_BLOCK:
        forced |= {BIN_COL_BLOCK - 1, BIN_COL_BLOCK}
    lo = hi = None
    for r0 in range(0, max(rows, 1), NW_ROW_BLOCK):
        wb, we = row0 + r0 - NW_BAND, row0 + r0 + NW_ROW_BLOCK + NW_BAND
        if lo is None and 0 < wb < cols:
            lo = wb - 1
        if hi is None and we < cols:
            hi = we
    forced |= {c for c in (lo, hi) if c is not None}
    rng = np.random.default_rng(cols)
    others = [int(c) for c in rng.permutation(cols)[:40] if int(c) not in forced][:24 - len(forced)]
    return np.array(sorted(forced | set(others)), dtype=np.int64)


def window_edges_in(u, rows, cols, row0=0):
    """(found, wanted): which ends (low, high) of csr_near_window windows have a column of u within 2 of them, and which ends
    exist at all inside x (a window that starts at column 0 or ends at the last one has no such end)."""
    found, wanted = [False, False], [False, False]
    for r0 in range(0, max(rows, 1), NW_ROW_BLOCK):
        for k, edge in enumerate((row0 + r0 - NW_BAND, row0 + r0 + NW_ROW_BLOCK + NW_BAND)):
            if 0 < edge < cols:
                wanted[k] = True
                found[k] |= bool(np.any(np.abs(np.asarray(u) - edge) <= 2))
    return found, wanted


def _drop_columns(row_ptr, col_ind, u):
    keep = ~np.isin(col_ind[:row_ptr[-1]], u)
    lens = np.bincount(row_of_entries(row_ptr)[keep], minlength=len(row_ptr) - 1)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), np.ascontiguousarray(col_ind[:row_ptr[-1]][keep], dtype=np.int32)


def structure(name):
    """(rows, cols, row_ptr, col_ind, U): a sparsity pattern of the catalogue in which the columns U = unused_columns(...) hold no
    entry.  Patterns made from row lengths (the edge cases, `straddle`) draw their columns from the other columns, so every row
    keeps its length; fixed patterns (fuzz, samples, models) lose the few entries they had there."""
    import parity
    import test_gpu_parity as gp

    lens = None
    if name.startswith("edge:"):
        rng = np.random.default_rng(zlib.crc32(name[5:].encode()))
        lens, cols = gp.EDGE_CASES[name[5:]](rng)
    elif name == "straddle":
        rng, lens, cols = np.random.default_rng(15), STRADDLE_LENS, 4096
    if lens is not None:
        rows = len(lens)
        u = unused_columns(rows, cols)
        free = np.setdiff1d(np.arange(cols), u)
        row_ptr, col_ind, _ = gp.csr_from_lengths(rng, list(lens), len(free))
        return rows, cols, row_ptr, free[col_ind].astype(np.int32), u
    if name.startswith("fuzz:"):
        rows, cols, row_ptr, col_ind, _, _ = gp._fuzz_matrix(int(name[5:]))
    elif name in ("memplus", "pwt"):
        _, rows, cols, coo = sm.mm_read_coo(ob.fixture_path(name + ".mtx"))
        row_ptr, col_ind, _ = sm.csr_from_coo(coo, rows)
    elif name == "uniform32":                         # 32 uniform columns per row: the column sweep's strips, ragged last iteration
        rows, cols = 20_000, 60_000
        row_ptr, col_ind, _ = sm.synth_csr(sm.SYNTH_UNIFORM, 2025, cols, cols, 32, 0, rows)
    elif name == "random_model":                      # the size of test_binned_plan_on_the_random_model: AUTO = BINNED with the window
        rows = cols = 1 << 22
        row_ptr, col_ind, _ = sm.synth_csr(sm.SYNTH_MEMPLUS_SHAPED, 12345, rows, rows)
    elif name == "fr32":
        rows, cols, band, row_ptr, col_ind, _ = parity.spill_matrix("fr32")
        assert band == 0
    else:
        raise KeyError(name)
    u = unused_columns(rows, cols)
    row_ptr, col_ind = _drop_columns(np.asarray(row_ptr), np.asarray(col_ind), u)
    return rows, cols, row_ptr, col_ind, u


# --------------------------------------------------------------------------------------------------------------- operands
def _pick_columns(rng, counts, taken, n, rows):
    """n referenced columns outside `taken`, preferring those that few rows use (at most 0.3 % of the rows each, so that a dozen
    poisoned columns leave 90 % of the rows finite where the matrix allows it)."""
    cand = np.flatnonzero(counts > 0)
    cand = cand[~np.isin(cand, taken)]
    light = cand[counts[cand] <= max(1, rows * 0.003)]
    pool = light if len(light) >= n else cand[np.argsort(counts[cand], kind="stable")[:max(n, 1)]]
    return np.sort(rng.choice(pool, size=min(n, len(pool)), replace=False)) if len(pool) else pool


def ordinary(rows, cols, row_ptr, col_ind, u, seed=1):
    """The values and operands of scenarios A ... D on one pattern -> dict:
      val       uniform in (-1, 1), 2 % of the entries stored zeros (0.0 and -0.0), half the entries of the columns `pc` too;
                every 7th row all negative, the row after it all positive (zeros included: their sign bit);
      x         uniform in (-1, 1), 0.0 in the columns u; x_a the same with NaN, +Inf, -Inf cycling through u;
      x_b       x with NaN, +Inf, -Inf cycling through the twelve referenced columns pb;
      x_c       x with +Inf, -Inf alternating through the twelve referenced columns pc."""
    rng = np.random.default_rng(seed)
    nnz = int(row_ptr[-1])
    row_of = row_of_entries(row_ptr)
    val = rng.uniform(-1, 1, nnz)
    val[val == 0] = 0.5
    counts = np.bincount(col_ind[:nnz], minlength=cols)
    pb = _pick_columns(rng, counts, u, 12, rows)
    pc = _pick_columns(rng, counts, np.concatenate([u, pb]), 12, rows)
    zero = rng.random(nnz) < 0.02
    zero |= np.isin(col_ind[:nnz], pc) & (rng.random(nnz) < 0.5)
    val[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)
    val = np.where(row_of % 7 == 0, -np.abs(val), np.where(row_of % 7 == 1, np.abs(val), val))   # (|-0.0| = 0.0, -|0.0| = -0.0)
    x = rng.uniform(-1, 1, cols)
    x[x == 0] = 0.25
    x[u] = 0.0
    x_a, x_b, x_c = x.copy(), x.copy(), x.copy()
    x_a[u] = np.resize(POISON, len(u))
    x_b[pb] = np.resize(POISON, len(pb))
    x_c[pc] = np.resize(POISON[1:], len(pc))
    return {"val": val, "x": x, "x_a": x_a, "x_b": x_b, "x_c": x_c, "pb": pb, "pc": pc}


def subnormal(rows, cols, row_ptr, col_ind, seed=2):
    """Scenario E: val = k 2^-1060 (k = +-1 ... +-8), x = -4 ... 4: products and sums are exact multiples of 2^-1060 far below
    2^-1022 (a row would need 2^33 entries to leave the subnormal range)."""
    rng = np.random.default_rng(seed)
    nnz = int(row_ptr[-1])
    k = rng.integers(1, 9, nnz) * rng.choice([-1, 1], nnz)
    return k * 2.0 ** -1060, rng.integers(-4, 5, cols).astype(np.float64)


def overflowing(rows, cols, row_ptr, col_ind):
    """Scenario F: val = +-2^510 (even rows +, odd rows -), x = 2^510."""
    sign = np.where(row_of_entries(row_ptr) % 2 == 0, 1.0, -1.0)
    return sign * 2.0 ** 510, np.full(cols, 2.0 ** 510)


def rounded(rows, cols, row_ptr, col_ind, seed=3):
    """Scenario G: |val| and x uniform in [1, 2) with full mantissas, val of either sign: every product is rounded and the
    partial sums stay of the products' size, so the product's rounding error shows in the sum."""
    rng = np.random.default_rng(seed)
    nnz = int(row_ptr[-1])
    return (1.0 + rng.random(nnz)) * rng.choice([-1.0, 1.0], nnz), 1.0 + rng.random(cols)


# ---------------------------------------------------------------------------------------------------------------- regimes
def regime(scenario, rows, cols, row_ptr, col_ind, val, x, u=()):
    """The numbers a scenario's condition is about, from the host alone (products, the oracle, the pattern)."""
    nnz = int(row_ptr[-1])
    ci, val = np.asarray(col_ind)[:nnz], np.asarray(val)[:nnz]
    row_of = row_of_entries(row_ptr)
    lens = np.diff(row_ptr)
    if scenario == "A":
        used = np.bincount(ci, minlength=cols) > 0
        return {"unused_poisoned": int((~used[u] & ~np.isfinite(x[u])).sum()) if len(u) else 0, "used_poisoned": int((~np.isfinite(x) & used).sum()),
                "ends": int(0 in u) + int(cols - 1 in u), "block_edge": int(BIN_COL_BLOCK - 1 in u) + int(BIN_COL_BLOCK in u),
                "window_edges": window_edges_in(u, rows, cols)}
    with np.errstate(invalid="ignore", over="ignore"):
        p = val * x[ci]
    if scenario in ("B", "C"):
        cls = row_classes(row_ptr, col_ind, val, x)
        out = {"finite_share": float((cls == FINITE).mean()) if rows else 1.0, "nan": int((cls == NAN).sum()),
               "pinf": int((cls == PINF).sum()), "ninf": int((cls == NINF).sum())}
        bad = ~np.isfinite(p)
        from_zero = bad & (val == 0)
        out["zero_only"] = int(((np.bincount(row_of[from_zero], minlength=rows) > 0) &
                                (np.bincount(row_of[bad & ~from_zero], minlength=rows) == 0)).sum())
        return out
    if scenario == "D":
        negz = p.view(np.int64) == NEG_ZERO
        return {"all_negative_zero": int(((np.bincount(row_of[negz], minlength=rows) == lens) & (lens > 0)).sum()),
                "empty": int((lens == 0).sum()), "all_zero": bool(np.all(p == 0))}
    if scenario == "G":
        pick = np.flatnonzero((lens >= 5) & (lens <= 32))[:300]      # (a row's first step adds to 0.0: fused or not, the same)
        ref = ob.csr_spmv(row_ptr, col_ind, val, x)
        return {"sampled": len(pick), "fma_differs": float((fma_serial(row_ptr, col_ind, val, x, pick) != ref[pick]).mean()) if len(pick) else 0.0}
    raise KeyError(scenario)


def assert_regime(name, scenario, rows, cols, row_ptr, col_ind, val, x, u=()):
    """The input reaches what the scenario is about -- on the structures REGIME lists for it; on the others (too few rows or
    columns for the condition) the numbers are returned with "held": False, never taken for a pass."""
    g = regime(scenario, rows, cols, row_ptr, col_ind, val, x, u)
    must = name in REGIME[scenario]
    if scenario == "A":
        g["held"] = (g["unused_poisoned"] >= 16 and g["used_poisoned"] == 0 and g["ends"] == 2 and
                     (cols <= BIN_COL_BLOCK or g["block_edge"] == 2) and g["window_edges"][0] == g["window_edges"][1])
        assert cols >= MIN_COLS_A or not must, "%s: %d columns: takes no part in scenario A" % (name, cols)
    elif scenario == "B":
        g["held"] = g["finite_share"] >= 0.9 and min(g["nan"], g["pinf"], g["ninf"]) >= 10
    elif scenario == "C":
        g["held"] = g["zero_only"] >= 10
    elif scenario == "G":
        g["held"] = g["sampled"] >= 50 and g["fma_differs"] >= 0.5
    else:
        g["held"] = g["all_negative_zero"] >= 10 and g["empty"] >= 10 and g["all_zero"]
    assert g["held"] or not must, "%s does not reach scenario %s: %r" % (name, scenario, g)
    return g


# ------------------------------------------------------------------------------------------- what a product is held to
def assert_unreferenced(y_poisoned, y_clean, what):
    """Scenario A on a path that is reproducible from run to run: no tolerance."""
    assert np.isfinite(y_clean).all(), "%s: a row of the clean product is not finite" % what
    check_bits(y_poisoned, y_clean, what + ", x poisoned where nobody reads it")


def assert_against_oracle(y, ref, scale, terms, classes, what, serial=None):
    """Scenarios A (TJDS ATOMIC), B, C and G: classes exact and finite rows within the bound (parity.check_y); the serial loop's
    bits on the rows `serial` (a mask) that the path sums left to right."""
    import parity

    check_classes(y, classes, what)
    parity.check_y(y, ref, scale, terms)
    if serial is not None and serial.any():
        check_bits(np.asarray(y)[serial], np.asarray(ref)[serial], what + ", rows with the serial loop's bits")
        check_no_negative_zero(np.asarray(y)[serial], what)


def assert_exact(y, ref, what):
    """Scenarios D, E and F: every order of summation gives the oracle's bits; the serial loop never gives -0.0."""
    check_no_negative_zero(ref, what + " (the oracle itself)")
    check_bits(y, ref, what)
