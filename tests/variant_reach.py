"""Which compiled variant of K15 (smvp_trsv.hip) and K17 (smvp_ilu0.hip) a matrix runs, restated: the lanes-per-row rules of the two
plans, the lanes a chain gives a row, K17's hand-off of a long row to a wavefront, and for a whole case the set of cells (kernel, T,
what) its rows reach.  Plain functions, no fixtures.  test_variant_reach_host.py pins them to hand-computed values and holds the
union of the suite's cases to REQUIRED_TRSV and REQUIRED_ILU0; the GPU tests pin the constants mirrored here to what the library
reports (lanes_per_row, chain_width), so a drift fails there instead of moving a case to another variant unseen.

A cell.  kernel: "wide" (trsv_level_rows<T> / ilu0_level_rows<T>, a level of more than chain_width rows), "chain" (a level inside
trsv_chain / ilu0_chain) or, K17 only, "handed" (a row of a chain's level that its level's T lanes leave to a whole wavefront).
T: the lanes of the row's group (1: a lane walks the row alone; a handed row carries its LEVEL's T, the wavefront that takes it has
64).  what, K15: the passes of T * 4 entries the group makes over the WHOLE stored row (the kernel classifies every stored entry,
the other triangle's too) -- "1 partial" (fewer than 4 T entries), "1 full" (exactly 4 T), "2", "3", "4", "5+"; for T = 1 "<=8"
or ">8" entries, the lone lane's two loops.  what, K17: "regs" (the row fits the registers of the lanes that take it: 8 a lane) or
"mem" (its w lives in F)."""
import math

import numpy as np

import trsv_method as trsv

BLOCK = 256          # lanes of a chain's one workgroup (kVectorBlock)
CHUNK = 4            # entries a lane takes in a pass, and the divisor of both lane rules (kTrsvChunk, kIluChunk)
UNROLL = 8           # a lone lane's short loop (kTrsvUnroll)
SLOTS = 8            # entries of its row a lane of K17 keeps in registers (kIluSlots)
LONG_TRIPS = 8       # K17: a chain hands a row over where its lanes would need more trips a pivot (kIluLongTrips)
LANES = (2, 4, 8, 16, 32, 64)
PASSES = ("1 partial", "1 full", "2", "3", "4", "5+")


# ---------------------------------------------------------------------------------------------------------------------- the rules
def pow2(x):
    """pow2_lanes: the smallest power of two from 2 to 64 that is not below x."""
    p = 2
    while p < 64 and p < x:
        p <<= 1
    return p


def lanes_rule(mean, longest):
    return pow2(math.sqrt(mean * longest) / CHUNK)


def triangle_lengths(M, uplo):
    """Stored entries of every row inside the triangle, the diagonal included (whatever the diag setting; repeats count)."""
    r, c, _ = M.entries()
    keep = (c <= r) if uplo == trsv.LOWER else (c >= r)
    return np.bincount(r[keep], minlength=M.n)


def wide_lanes_trsv(M, uplo):
    t = triangle_lengths(M, uplo)
    return lanes_rule(float(t.sum()) / M.n if M.n else 0.0, int(t.max()) if M.n else 0)


def wide_lanes_ilu0(M):
    lengths = np.diff(M.csr[0])
    return lanes_rule(float(M.nnz) / M.n if M.n else 0.0, int(lengths.max()) if M.n else 0)


def chain_lanes(width):
    """Lanes a row of a chain's level of `width` rows gets: the largest power of two, 64 at the most, that leaves every row a
    group of the 256 lanes; 1 from 129 rows on (under the wider chain options too: a lane then takes 2 or 4 rows)."""
    q = BLOCK // max(width, 1)
    return 64 if q >= 64 else 1 << (q.bit_length() - 1) if q >= 2 else 1


def ilu0_is_long(length, T):
    return T < 64 and length > LONG_TRIPS * SLOTS * T


def passes(length, T):
    """K15: what a group of T >= 2 lanes makes of a stored row of `length` entries."""
    n = -(-length // (CHUNK * T))
    return "1 partial" if length < CHUNK * T else "1 full" if length == CHUNK * T else str(n) if n <= 4 else "5+"


def trsv_cell(kernel, T, length):
    return (kernel, T, ("<=8" if length <= UNROLL else ">8") if T == 1 else passes(length, T))


def ilu0_cell(width, length, w, wide_T):
    if width > w:
        return ("wide", wide_T, "regs" if length <= SLOTS * wide_T else "mem")
    T = chain_lanes(width)
    if ilu0_is_long(length, T):
        return ("handed", T, "regs" if length <= SLOTS * 64 else "mem")
    return ("chain", T, "regs" if length <= SLOTS * T else "mem")


# ---------------------------------------------------------------------------------------------------------------------- the reach
def reach_trsv(M, uplo, w):
    """The cells the rows of M reach in one solve with the `uplo` triangle at a chain width of w."""
    f = M.facts(uplo, trsv.STORED)
    lengths, wide_T = np.diff(M.csr[0]), wide_lanes_trsv(M, uplo)
    out = set()
    for l, width in enumerate(f["widths"].tolist()):
        rows = f["order"][f["level_ptr"][l]:f["level_ptr"][l + 1]]
        kernel, T = ("wide", wide_T) if width > w else ("chain", chain_lanes(width))
        out |= {trsv_cell(kernel, T, n) for n in set(lengths[rows].tolist())}
    return out


def reach_ilu0(M, w):
    """The cells the rows of M reach in one factorisation at a chain width of w."""
    f = M.facts(trsv.LOWER, trsv.UNIT)
    lengths, wide_T = np.diff(M.csr[0]), wide_lanes_ilu0(M)
    out = set()
    for l, width in enumerate(f["widths"].tolist()):
        rows = f["order"][f["level_ptr"][l]:f["level_ptr"][l + 1]]
        out |= {ilu0_cell(width, n, w, wide_T) for n in set(lengths[rows].tolist())}
    return out


def handed_places(M, w):
    """K17's hand-off, level by level: for every chain level that holds long rows, (T, width, places of the long rows in the
    level).  The k-th of them (from 0) goes to wavefront k % 4; a place of 64 or more is found in a later ballot round."""
    f = M.facts(trsv.LOWER, trsv.UNIT)
    lengths = np.diff(M.csr[0])
    out = []
    for l, width in enumerate(f["widths"].tolist()):
        if width > w:
            continue
        T = chain_lanes(width)
        rows = f["order"][f["level_ptr"][l]:f["level_ptr"][l + 1]]
        places = [k for k, n in enumerate(lengths[rows].tolist()) if ilu0_is_long(n, T)]
        if places:
            out.append((T, width, places))
    return out


def updates_off_the_diagonal(M):
    """For every row of M (a Case ilu0_method accepts): the updates w[t] -= l * u that land on a position other than the row's
    diagonal, counted from the pattern as the factorisation's loop finds them."""
    row_ptr, col_ind, _ = M.csr
    rp, ci = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist()
    dp = {i: next(p for p in range(rp[i], rp[i + 1]) if ci[p] == i) for i in range(M.n)}
    count = np.zeros(M.n, dtype=np.int64)
    for i in range(M.n):
        if dp[i] == rp[i]:
            continue
        mine = set(ci[rp[i]:rp[i + 1]]) - {i}
        for p in range(rp[i], dp[i]):
            k = ci[p]
            count[i] += sum(1 for q in range(dp[k] + 1, rp[k + 1]) if ci[q] in mine)
    return count


# ------------------------------------------------------------------------------------------------------------------- the tables
# K15.  Every wide variant at every pass count.  A chain's thin levels run the same passes with T at run time: every T once, the
# lone lane's two loops, and -- where a DPP hand-up crosses the 16-lane rows of a wavefront -- T = 32 and 64 at every pass count.
REQUIRED_TRSV = frozenset([("wide", T, p) for T in LANES for p in PASSES] + [("chain", T, "1 partial") for T in LANES]
                          + [("chain", T, p) for T in (32, 64) for p in PASSES] + [("chain", 1, "<=8"), ("chain", 1, ">8")])

# K17.  Every wide variant on both paths; a chain's level at every T on both paths (T = 1: more than 8 entries, at most 64); a
# handed row from every level T below 64 on the memory path, and on the register path (at most 512 entries) where a long row can
# be that short: more than 64 T entries, so T <= 4.
REQUIRED_ILU0 = frozenset([("wide", T, p) for T in LANES for p in ("regs", "mem")]
                          + [("chain", T, p) for T in (1,) + LANES for p in ("regs", "mem")]
                          + [("handed", T, "mem") for T in (1, 2, 4, 8, 16, 32)] + [("handed", T, "regs") for T in (1, 2, 4)])
