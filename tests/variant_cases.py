"""Matrices built to run one chosen variant of K15 and K17 each (variant_reach.py has the rules they are built on): tiers(T, w) and
its ILU(0) twin for every wide kernel, chain_tail(T, w) for the long rows of a K15 chain's 32- and 64-lane groups, handed(T, w) for
K17's hand-off of a long row to a wavefront from a level of every width class.  Plain functions, no fixtures; the knobs (how many
diagonal-only rows, how long the filler rows are) are what makes the lane rule yield T, and test_variant_reach_host.py holds every
case to that and to its shape."""
import functools

import numpy as np

import ilu0_method as im
import trsv_method as trsv
import variant_reach as vr

N_B = 9              # rows of tiers' middle level
SHARED = 3           # rows of the first level each of them depends on, shared with the last level's rows of its group


def special_lengths(T):
    """Triangle lengths (diagonal included) a tiers case holds in its wide last level: both sides of 1, 2, 3, 4 and 5 passes of 4 T."""
    return [2, 3, 4 * T - 1, 4 * T, 4 * T + 1, 8 * T, 8 * T + 1, 12 * T, 12 * T + 1, 16 * T, 16 * T + 1, 20 * T + 1]


# how many diagonal-only rows and how long a filler row, so that K15's rule on the triangle / K17's on the whole rows of the
# symmetrised twin yields T at a chain width of 256 (the lane rule's input is mean * longest: see test_variant_reach_host.py)
KNOBS_TRSV = {2: (1400, 3), 4: (700, 3), 8: (500, 5), 16: (600, 8), 32: (900, 16), 64: (1500, 72)}
KNOBS_ILU0 = {2: (3000, 3), 4: (700, 3), 8: (400, 4), 16: (500, 6), 32: (800, 10), 64: (1400, 28)}


def tiers_entries(T, w, nA, filler, seed, shuffle):
    """(n, rows, cols) of a lower triangular structure of three levels.  A: nA rows, diagonal only.  B: N_B rows, each on SHARED rows
    of A of its own.  C: w + 7 rows (wider than a chain; odd, so the last wavefront's groups have no row), row j in group j % N_B:
    it holds its group's B row, from three entries on one of that B row's A rows, and beyond that distinct other rows of A.  The
    special lengths stand 21 places apart among the fillers."""
    rng = np.random.default_rng(seed)
    nC = w + 7
    lengths = [filler] * nC
    for k, m in enumerate(special_lengths(T)):
        lengths[5 + k * (nC // 12)] = m
    pool = np.arange(N_B * SHARED, nA)
    assert len(pool) >= max(lengths) - 3 and filler >= 3
    r, c = list(range(nA)), list(range(nA))
    for g in range(N_B):
        cols = [nA + g] + list(range(g * SHARED, (g + 1) * SHARED))
        r += [nA + g] * len(cols)
        c += cols
    for j, m in enumerate(lengths):
        i, g = nA + N_B + j, j % N_B
        cols = [i, nA + g] + ([g * SHARED + (j // N_B) % SHARED] if m >= 3 else [])
        cols = np.array(cols[:m] + rng.choice(pool, max(m - 3, 0), replace=False).tolist())
        assert len(cols) == m
        if shuffle:
            cols = cols[rng.permutation(m)]
        r += [i] * m
        c += cols.tolist()
    return nA + N_B + nC, r, c, lengths


@functools.lru_cache(maxsize=None)
def tiers(T, w):
    """K15's case for trsv_level_rows<T>: every row's entries in a random storage order, trsv_method.dominant values."""
    nA, filler = KNOBS_TRSV[T]
    n, r, c, _ = tiers_entries(T, w, nA, filler, 20500 + T, shuffle=True)
    return trsv.dominant("tiers(%d, %d)" % (T, w), n, r, c, 20501 + T)


@functools.lru_cache(maxsize=None)
def tiers_flipped(T, w):
    return trsv.flipped(tiers(T, w))


@functools.lru_cache(maxsize=None)
def tiers_ilu0(T, w):
    """K17's case for ilu0_level_rows<T>: the structure plus its transpose, columns ascending.  A C row's pivot on its shared A row
    updates the C row's entry in its B row's column -- a position another lane owns and a later pivot."""
    nA, filler = KNOBS_ILU0[T]
    n, r, c, _ = tiers_entries(T, w, nA, filler, 20600 + T, shuffle=False)
    return im.symmetrised(trsv.Case("tiers_ilu0(%d, %d)" % (T, w), n, r, c, np.ones(len(r))), 20601 + T)


def chain_tail_lengths(T):
    """8 T + 1: the third pass begins with one lane holding one entry; 4, 5 and 7 passes, partial and exact; 1 and 2 passes."""
    return [8 * T + 1, 12 * T + 1, 16 * T, 16 * T + 1, 20 * T, 24 * T + 3, 28 * T, 8 * T, 4 * T + 2, 3, 4 * T]


CHAIN_TAIL_WIDTHS = {32: (5, 8, 6, 7), 64: (1, 4, 2, 4)}


@functools.lru_cache(maxsize=None)
def chain_tail(T, w):
    """K15: a level of diagonal-only rows, then thin levels whose rows get T = 32 or 64 lanes in a chain and take up to 7 passes."""
    rng = np.random.default_rng(20700 + T)
    widths = [max(w + 1, 28 * T + 8)] + list(CHAIN_TAIL_WIDTHS[T])
    start = np.concatenate([[0], np.cumsum(widths)])
    r, c = list(range(widths[0])), list(range(widths[0]))
    lengths, at = chain_tail_lengths(T), 0
    for l in range(1, len(widths)):
        for k in range(widths[l]):
            i, m = int(start[l]) + k, lengths[at % len(lengths)]
            at += 1
            first = int(rng.integers(start[l - 1], start[l]))
            others = rng.choice(np.setdiff1d(np.arange(start[l]), [first]), m - 2, replace=False)
            cols = np.array([i, first] + others.tolist())[rng.permutation(m)]
            r += [i] * m
            c += cols.tolist()
    M = trsv.dominant("chain_tail(%d, %d)" % (T, w), int(start[-1]), r, c, 20701 + T)
    assert M.facts(trsv.LOWER, trsv.STORED)["widths"].tolist() == widths
    return M


# ------------------------------------------------------------------------------------------------------------------------ handed
HEAD = 4             # rows in front of a handed case: level 0, pivots of the thin rows, their upper parts reach every thin row


def handed_widths(T, w):
    """Widths of the four thin levels, each of T's class (T = 1: 129 rows or more; the first as wide as a chain may be, less 3)."""
    lo = {1: 129, 2: 65, 4: 33, 8: 17, 16: 9, 32: 5}[T]
    hi = w - 3 if T == 1 else vr.BLOCK // T
    return [hi, lo + 1, lo, hi if T > 1 else lo + 3]


def handed_lengths(T, w):
    """Whole-row lengths of the four thin levels' rows, by place.  Level 1: 64 T (the longest row that stays), 64 T + 1 (long),
    a long row of at most 512 entries where T <= 4 (registers after the hand-off), one of more than 512 (memory), one of more
    than 1536 (each lane makes a second trip of 8 * 64 per pivot), rows of 8 T + 1 (the level's own memory path), short rows; for T
    <= 2 the long rows stand at places of 64 and more.  Level 2: seven long rows among short ones, so the deal wraps round the four
    wavefronts.  Level 3: long rows only.  Level 4: one long row, the last of the level, dealt to wavefront 0."""
    widths = handed_widths(T, w)
    long_ = 64 * T + 1
    short = [3, 4, 6, 5]
    first = [64 * T, long_] + ([64 * T + 37] if T <= 4 else []) + [max(long_, 513) + 90, max(long_, 1537) + 70, 8 * T + 1, 8 * T + 1]
    one = [short[k % 4] for k in range(widths[0])]
    at = [66 + 9 * k for k in range(len(first))] if T <= 2 else [(k * widths[0]) // len(first) for k in range(len(first))]
    for p, m in zip(at, first):
        one[p] = m
    two = [short[k % 4] for k in range(widths[1])]
    for k in range(7):
        two[(k * (widths[1] - 1)) // 6] = long_ + k                                  # (the last of them is the level's last row)
    three = [long_ + (k % 5) for k in range(widths[2])]
    four = [short[k % 4] for k in range(widths[3])]
    four[-1] = long_ + 2
    return [one, two, three, four]


@functools.lru_cache(maxsize=None)
def handed(T, w):
    """K17: HEAD rows, four thin levels, then a tail of diagonal-only rows that the thin rows' upper parts name.  Row i of a thin
    level holds below the diagonal a row k of the level before (long ones among them: read from F behind the barrier) and the head
    row k % HEAD, whose upper part holds k: the first pivot updates the second's position.  Above the diagonal it holds tail columns,
    drawn from the first few of the tail so that rows share them.  The pattern is not symmetric; the columns ascend."""
    rng = np.random.default_rng(20800 + T)
    lengths = handed_lengths(T, w)
    n_thin = sum(len(x) for x in lengths)
    tail0 = HEAD + n_thin
    n_tail = max(max(x) for x in lengths) + 64
    n = tail0 + n_tail
    r, c = [], []
    for h in range(HEAD):
        cols = [h] + [j for j in range(HEAD, tail0) if j % HEAD == h] + list(range(tail0, tail0 + 16))
        r += [h] * len(cols)
        c += cols
    i, before = HEAD, list(range(HEAD))
    for level in lengths:
        mine = []
        for place, m in enumerate(level):
            k = before[(place * 7 + 3) % len(before)] if before[0] >= HEAD else None
            lower = [i % HEAD] if k is None else sorted({k % HEAD, k})
            ups = m - 1 - len(lower)
            among = min(n_tail, max(2 * ups, 16))
            cols = lower + [i] + sorted((tail0 + rng.choice(among, ups, replace=False)).tolist())
            assert len(cols) == m
            r += [i] * m
            c += cols
            mine.append(i)
            i += 1
        before = mine
    r += list(range(tail0, n))
    c += list(range(tail0, n))
    M = trsv.dominant("handed(%d, %d)" % (T, w), n, r, c, 20801 + T)
    assert M.facts(trsv.LOWER, trsv.UNIT)["widths"].tolist() == [HEAD + n_tail] + handed_widths(T, w), M.name
    return M


TIERS_T = vr.LANES
CHAIN_TAIL_T = (32, 64)
HANDED_T = (1, 2, 4, 8, 16, 32)


def trsv_cases(w):
    return tuple([tiers(T, w) for T in TIERS_T] + [tiers_flipped(T, w) for T in TIERS_T] + [chain_tail(T, w) for T in CHAIN_TAIL_T])


def ilu0_cases(w):
    return tuple([tiers_ilu0(T, w) for T in TIERS_T] + [handed(T, w) for T in HANDED_T])
