"""ILU(0) on a CSR handle (include/smvp_amd.h: smvp_csr_ilu0_create / smvp_ilu0_factor, kernel K17) restated in plain Python, and
the cases it is held to.  Plain functions, no fixtures: test_ilu0_host.py pins them to hand-computed values, to the library's own
host loop and to derived bounds on the CPU, test_gpu_ilu0.py compares the library's bits with them.

Why bits.  Row i's pivots come in ascending column, each w[t] takes at most one update per pivot -- the product rounded, then the
difference rounded -- and every multiplier is one division by the final u_kk.  Every element of F has one right answer, the serial
loop's.  The updates below run on Python floats, which are the machine's IEEE doubles; the division is np.float64's, so a zero
pivot gives +-Inf or NaN instead of raising."""
import functools

import numpy as np

import cg_method as cg
import pcg_method as pcg
import pcg_tri_method as tri
import power_iteration as pi
import trsv_method as trsv

LOWER, UPPER, STORED, UNIT = trsv.LOWER, trsv.UPPER, trsv.STORED, trsv.UNIT


# ------------------------------------------------------------------------------------------------------------ the factorisation
def diag_positions(M):
    """diag_pos of a Case whose rows hold their columns strictly ascending and a diagonal each (asserted)."""
    row_ptr, col_ind, _ = M.csr
    r, c, _ = M.entries()
    same_row = np.diff(r) == 0
    assert (np.diff(c)[same_row] > 0).all(), "%s: a row's columns are not strictly ascending" % M.name
    at = np.flatnonzero(c == r)
    assert len(at) == M.n and (r[at] == np.arange(M.n)).all(), "%s: a row stores no diagonal" % M.name
    return at.astype(np.int32)


def ilu0(M, finite=True):
    """F as a Case on M's own arrays' pattern: the loop of the header.  Where the case claims a finite factor that is asserted."""
    row_ptr, col_ind, val = M.csr
    rp, ci = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist()
    F = np.asarray(val, dtype=np.float64).tolist()
    dp = diag_positions(M).tolist()
    with np.errstate(all="ignore"):
        for i in range(M.n):
            where = {ci[p]: p for p in range(rp[i], rp[i + 1])}
            for p in range(rp[i], dp[i]):
                k = ci[p]
                l = float(np.float64(F[p]) / np.float64(F[dp[k]]))
                F[p] = l
                for q in range(dp[k] + 1, rp[k + 1]):
                    t = where.get(ci[q])
                    if t is not None:                                                # an update that does not exist is skipped
                        F[t] = F[t] - l * F[q]
    F = np.array(F, dtype=np.float64)
    if finite:
        assert np.isfinite(F).all(), "%s: the restatement's own factor is not finite at %r" % (M.name, np.flatnonzero(~np.isfinite(F))[:5])
    out = trsv.Case.of_csr("ilu0(%s)" % M.name, M.n, row_ptr, col_ind, F, finite_stored=finite)
    assert (out.csr[1] == col_ind).all()
    return out


def factor(M, finite=True):
    """ilu0(M), computed once per Case, shared, left unchanged."""
    if "ilu0" not in M._ref:
        F = ilu0(M, finite)
        F.csr[2].setflags(write=False)
        M._ref["ilu0"] = F
    return M._ref["ilu0"]


def plans(F):
    """(first, m, second) for pcg_tri_method.run: M = L U from the one Case F."""
    return (F, LOWER, UNIT), None, (F, UPPER, STORED)


# ---------------------------------------------------------------------------------------------------------------- the matrices
def coalesced(M):
    """The same matrix with repeated (i, j) added up in storage order and every row's columns ascending."""
    r, c, v = M.entries()
    order = np.lexsort((c, r))                                                       # stable: repeats keep their stored order
    r, c, v = r[order], c[order], v[order].tolist()
    rows, cols, vals = [], [], []
    for i in range(len(r)):
        if rows and rows[-1] == r[i] and cols[-1] == c[i]:
            vals[-1] = vals[-1] + v[i]
        else:
            rows.append(int(r[i]))
            cols.append(int(c[i]))
            vals.append(v[i])
    return trsv.Case(M.name + ", coalesced", M.n, rows, cols, vals, M.finite_stored)


def symmetrised(M, seed):
    """M's structure plus its transpose, coalesced, with trsv_method.dominant values: the LOWER levels are M's (for a lower
    triangular M), every pivot has an upper row to subtract, and dominant rows make the matrix an H-matrix, so the factorisation
    exists."""
    r, c, _ = M.entries()
    both = np.unique(np.stack([np.concatenate([r, c]), np.concatenate([c, r])], axis=1), axis=0)   # sorted by (row, column)
    return trsv.dominant(M.name + ", symmetrised", M.n, both[:, 0], both[:, 1], seed)


def order_dependent():
    """Rows 0 .. 2 hold a unit diagonal and u_03 = 1, u_13 = -1, u_23 = -1; row 3 holds 1e16, 1e16, 1 and the diagonal 1.  Its
    multipliers are 1e16, 1e16 and 1, so the diagonal takes the subtractions of 1e16, -1e16 and -1 in that pivot order:
    ((1 - 1e16) + 1e16) + 1 = 1, the 1 it started from lost in the first.  Taking the third first gives (2 - 1e16) + 1e16 = 2, the
    second last 0: four of the five other orders give another value (the first two alone may swap: they are each other's negative)."""
    r = [0, 0, 1, 1, 2, 2, 3, 3, 3, 3]
    c = [0, 3, 1, 3, 2, 3, 0, 1, 2, 3]
    v = [1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1e16, 1e16, 1.0, 1.0]
    return trsv.Case("order_dependent", 4, r, c, v)


def of_matrix(name, M):
    """A cg_method / pcg_method matrix as the coalesced Case of its CSR arrays."""
    return coalesced(trsv.of_matrix(name, M))


def as_matrix(Cs):
    """A Case as a power_iteration.Matrix: the product's side of a system whose preconditioner stands on the Case."""
    r, c, v = Cs.entries()
    return pi.Matrix(Cs.n, r, c, v)


@functools.lru_cache(maxsize=None)
def grid(k):
    return of_matrix("lap2d(%d)" % k, tri.lap2d(k))


@functools.lru_cache(maxsize=None)
def spd_1003():
    return of_matrix("spd(1003)", cg.spd(1003))


@functools.lru_cache(maxsize=None)
def constructed_cases(w):
    """The symmetrised twins of K15's constructed LOWER schedules for a chain width of w."""
    return tuple(symmetrised(M, 20400 + i) for i, M in enumerate(trsv.constructed_cases(w)[:14]))


@functools.lru_cache(maxsize=None)
def more_cases():
    return (of_matrix("spd_long", cg.spd_long()), spd_1003(), of_matrix("tridiagonal(300)", pcg.tridiagonal(300)),
            trsv.sample("ibm32"), trsv.sample("curtis54"), trsv.sample("memplus"), trsv.sample("pwt"), order_dependent())


N_CONSTRUCTED, N_MORE = 14, 8


def case(w, i):
    return constructed_cases(w)[i] if i < N_CONSTRUCTED else more_cases()[i - N_CONSTRUCTED]


# --------------------------------------------------------------------------------------------------------- what the factor is held to
def scaled_integers(values):
    """(ints, S): every float64 of `values` times 2^S, S the smallest power of two that makes them all integers -- exact."""
    ratios = [float(x).as_integer_ratio() for x in values]
    S = max([d.bit_length() - 1 for _, d in ratios] + [0])
    return [n << (S - (d.bit_length() - 1)) for n, d in ratios], S


def product_terms(M, F):
    """For every stored position: (sum, sum of magnitudes, terms, S) of (L U)_ij = sum_k l_ik u_kj over the k for which both
    factors are stored (l_ii = 1), as integers times 2^(2 S): exact, nothing of the check's own rounding enters."""
    row_ptr, col_ind, _ = M.csr
    rp, ci = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist()
    f, S = scaled_integers(F.csr[2].tolist())
    dp = diag_positions(M).tolist()
    total, terms = [x << S for x in f], [1] * len(f)                                 # the k = min(i, j) term: l_ii u_ij on and above the diagonal,
    for i in range(M.n):                                                             # l_ij u_jj below it
        for p in range(rp[i], dp[i]):
            total[p] = f[p] * f[dp[ci[p]]]
    mag = [abs(x) for x in total]
    for i in range(M.n):
        where = {ci[p]: p for p in range(rp[i], rp[i + 1])}
        for p in range(rp[i], dp[i]):
            k = ci[p]
            for q in range(dp[k] + 1, rp[k + 1]):
                t = where.get(ci[q])
                if t is not None:
                    prod = f[p] * f[q]
                    total[t] += prod
                    mag[t] += abs(prod)
                    terms[t] += 1
    return total, mag, terms, S
