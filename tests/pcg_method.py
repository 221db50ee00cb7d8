"""The diagonal of a handle and conjugate gradients with a diagonal preconditioner (include/smvp_amd.h: smvp_csr_diagonal /
smvp_tjds_diagonal, smvp_csr_pcg / smvp_tjds_pcg, kernel K14) restated in numpy, on cg_method.py's dot.  Plain functions, no
fixtures: test_pcg_host.py pins them to known answers on the CPU, test_gpu_pcg.py compares the library's bits with them.

Why bits.  A diagonal element is a sum in storage order from +0.0, the dot's order is the header's, and everything else -- the
division z_i = r_i / m_i included -- is one correctly rounded IEEE operation per element: each number has one right answer.  The
only input that is the library's own is the product, so run() takes it as a function, as cg_method.run does."""
import functools

import numpy as np

import cg_method as cg
import power_iteration as pi
import smvp_toolkit_amd as sm

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = cg.CONVERGED, cg.MAX_STEPS, cg.BREAKDOWN, cg.NONFINITE


# ------------------------------------------------------------------------------------------------------------- the diagonal
def _sum_in_order(rows, at, where, val):
    """d[at[j]] += val[where[j]] for j in ascending order, every element from +0.0."""
    d = np.zeros(rows)
    with np.errstate(all="ignore"):
        for i, j in zip(at.tolist(), where.tolist()):
            d[i] = d[i] + val[j]
    return d


def diagonal_csr(rows, cols, row_ptr, col_ind, val, first_row=0):
    """Element r: the entries of row r at column first_row + r, added in ascending position inside the row, from +0.0.  A column
    beyond cols - 1 is nobody's."""
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(np.asarray(row_ptr, dtype=np.int64)))
    col = np.asarray(col_ind, dtype=np.int64)[:len(row_of)]
    hit = np.flatnonzero((col == row_of + first_row) & (row_of + first_row < cols))
    return _sum_in_order(rows, row_of[hit], hit, np.asarray(val, dtype=np.float64))


def diagonal_tjds(t):
    """Element i: the entries of original column i in row i, added in ascending TJDS position inside the column, from +0.0 (the
    entry at position start_pos[d] + k belongs to permuted column k, original column perm[k])."""
    sp = np.asarray(t.start_pos, dtype=np.int64)
    width = np.diff(sp)
    k = np.arange(t.nnz, dtype=np.int64) - np.repeat(sp[:-1], width)
    col = np.asarray(t.perm, dtype=np.int64)[k] if t.nnz else np.zeros(0, dtype=np.int64)
    row = np.asarray(t.row_ind, dtype=np.int64)[:t.nnz]
    hit = np.flatnonzero(row == col)                                             # ascending position: ascending diagonal inside a column
    return _sum_in_order(t.rows, row[hit], hit, np.asarray(t.val, dtype=np.float64))


class Case:
    """A rows x cols matrix from its entries in storage order: CSR arrays that keep that order inside every row (a stable sort by
    row: the columns of a row are NOT ascending, as adopted arrays' need not be) and the host converter's TJDS arrays."""

    def __init__(self, name, rows, cols, r, c, v):
        self.name, self.rows, self.cols = name, int(rows), int(cols)
        self.coo = sm.make_coo(r, c, v)
        self.nnz = len(self.coo)
        order = np.argsort(self.coo["row"], kind="stable")
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(self.coo["row"], minlength=self.rows))]).astype(np.int32)
        self.csr = row_ptr, self.coo["col"][order].astype(np.int32), self.coo["val"][order].astype(np.float64)
        self.tjds = sm.tjds_from_coo(self.coo, self.rows, self.cols)


def diagonal(M):
    """The diagonal of a Case or of a power_iteration.Matrix, from the CSR and from the TJDS arrays: both add the repeats of (i, i)
    in storage order (the converters keep ties in input order), so they agree to the bit -- asserted here."""
    if isinstance(M, Case):
        rows, cols, csr, t = M.rows, M.cols, M.csr, M.tjds
    else:
        rows, cols, csr, t = M.n, M.n, M.csr, sm.tjds_from_coo(M.coo, M.n, M.n)
    a, b = diagonal_csr(rows, cols, *csr), diagonal_tjds(t)
    ok = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), "the CSR and the TJDS walk disagree at %r" % np.flatnonzero(~ok)[:5]
    return a


# ------------------------------------------------------------------------------------------------------------------- the run
def run(product, b, x0, m, max_steps, tol):
    """(steps, updates, reason, rr_each, rz_each, sigma_each, x): the run as the header defines it; there is no check_every in it,
    because nothing depends on it.  product: numpy in, numpy out."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    m = np.ascontiguousarray(m, dtype=np.float64)
    tol = np.float64(tol)
    with np.errstate(all="ignore"):
        bb = cg.dot(b, b)
        thr = (tol * tol) * bb
        if x0 is None:
            x, r = np.zeros(len(b)), b.copy()
        else:
            x = np.ascontiguousarray(x0, dtype=np.float64).copy()
            r = b - np.ascontiguousarray(product(x), dtype=np.float64)
        z = r / m
        p = z.copy()
        rr, rho = cg.dot(r, r), cg.dot(r, z)
        rrs, rzs, sigmas = [rr], [rho], []

        def out(steps, updates, reason):
            return steps, updates, reason, np.array(rrs), np.array(rzs), np.array(sigmas), x

        if not (np.isfinite(bb) and np.isfinite(rr) and np.isfinite(rho)):
            return out(0, 0, NONFINITE)
        if rr <= thr:
            return out(0, 0, CONVERGED)
        if not rho > 0.0:
            return out(0, 0, BREAKDOWN)
        k = 0
        while True:
            k += 1
            q = np.ascontiguousarray(product(p), dtype=np.float64)
            sigma = cg.dot(p, q)
            sigmas.append(sigma)
            if not np.isfinite(sigma):
                return out(k, k - 1, NONFINITE)
            if not sigma > 0.0:
                return out(k, k - 1, BREAKDOWN)
            alpha = rho / sigma
            x = x + alpha * p                                                        # alpha * p is an array of its own: rounded first
            r = r - alpha * q
            z = r / m
            rr, rho_new = cg.dot(r, r), cg.dot(r, z)
            rrs.append(rr)
            rzs.append(rho_new)
            if not (np.isfinite(rr) and np.isfinite(rho_new)):
                return out(k, k, NONFINITE)
            if rr <= thr:
                return out(k, k, CONVERGED)
            if not rho_new > 0.0:
                return out(k, k, BREAKDOWN)
            if k == max_steps:
                return out(k, k, MAX_STEPS)
            beta = rho_new / rho
            p = z + beta * p
            rho = rho_new


# ---------------------------------------------------------------------------------------------------------------- the matrices
def scaled(M, span, seed=20290):
    """S A S of a cg_method matrix with S = diag(10^U[-span, span]): still symmetric positive definite, its condition number
    raised by up to 10^(4 span); the entries keep their storage order."""
    s = 10.0 ** np.random.default_rng(seed).uniform(-span, span, M.n)
    rows, cols, vals = (np.array(M.coo[f]) for f in ("row", "col", "val"))
    return pi.Matrix(M.n, rows, cols, (s[rows] * vals) * s[cols])


def tridiagonal(n):
    """2 on the diagonal, -0.5 beside it: symmetric, strictly dominant, and cheap to build at any size."""
    i = np.arange(n)
    rows = np.concatenate([i, i[1:], i[:-1]])
    cols = np.concatenate([i, i[:-1], i[1:]])
    vals = np.concatenate([np.full(n, 2.0) + 0.25 * (i % 7), np.full(2 * (n - 1), -0.5)])
    return pi.Matrix(n, rows, cols, vals)


def _random_entries(rng, rows, cols, lens, diagonal_share):
    """Rows of `lens` distinct columns in a random order inside the row; a row keeps its diagonal column with the given chance."""
    r, c = [], []
    for i, l in enumerate(lens.tolist()):
        pool = np.delete(np.arange(cols), i) if i < cols else np.arange(cols)
        take = rng.choice(pool, min(int(l), len(pool)), replace=False)
        if i < cols and len(take) and rng.random() < diagonal_share:
            take[rng.integers(len(take))] = i
        r.append(np.full(len(take), i))
        c.append(take)
    r, c = np.concatenate(r), np.concatenate(c)
    return r, c, rng.uniform(-1.0, 1.0, len(r)) * 10.0 ** rng.integers(-2, 3, len(r))


def _sparse(name, rows, cols, top, seed, diagonal_share=0.6):
    rng = np.random.default_rng(seed)
    return Case(name, rows, cols, *_random_entries(rng, rows, cols, rng.integers(0, top + 1, rows), diagonal_share))


def _signed_zeros():
    """Row 3 stores a lone 0.0 diagonal, row 7 a lone -0.0 (it reads +0.0), row 11 -0.0 twice (still +0.0), row 15 -0.0 and 2.5."""
    C0 = _sparse("z", 40, 40, 4, 20291, diagonal_share=0.0)
    r, c, v = (np.array(C0.coo[f]) for f in ("row", "col", "val"))
    er = [3, 7, 11, 11, 15, 15]
    ev = [0.0, -0.0, -0.0, -0.0, -0.0, 2.5]
    return Case("signed zeros on the diagonal", 40, 40, np.concatenate([r, er]), np.concatenate([c, er]), np.concatenate([v, ev]))


def _repeats():
    """Rows 5, 64 and 199 store their diagonal three times -- 1e16, 1.0, -1e16 in that storage order, which gives (1e16 + 1) - 1e16
    = 0.0 where any order that meets the two large values first gives 1.0 -- among the other entries, the whole in a random order
    that keeps those three in theirs."""
    rng = np.random.default_rng(20292)
    C0 = _sparse("r", 200, 200, 6, 20293, diagonal_share=0.0)
    r, c, v = (np.array(C0.coo[f]) for f in ("row", "col", "val"))
    three = np.array([1e16, 1.0, -1e16])
    for i in (5, 64, 199):
        r, c, v = np.concatenate([r, [i] * 3]), np.concatenate([c, [i] * 3]), np.concatenate([v, [np.nan] * 3])
    order = rng.permutation(len(r))
    r, c, v = r[order], c[order], v[order]
    for i in (5, 64, 199):
        slots = np.flatnonzero((r == i) & (c == i))
        v[slots] = three                                                            # ascending storage position
    return Case("three repeats of mixed sign, shuffled", 200, 200, r, c, v)


LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 257)


def _positions(filler):
    """n = 260.  For every length L of LENGTHS three rows of L entries whose diagonal is the first, the middle and the last entry
    of the row; every other row has `filler` entries and no diagonal (filler moves the mean row length, hence the width of the
    group of lanes a row gets: 0 -> 8, 2 -> 16, 20 -> 32, 40 -> 64)."""
    rng = np.random.default_rng(20294 + filler)
    n = 260
    r, c = [], []
    special = {}
    for a, L in enumerate(LENGTHS):
        for b, at in enumerate((0, L // 2, L - 1)):
            special[3 + 9 * a + 3 * b] = (L, at)
    for i in range(n):
        others = np.delete(np.arange(n), i)
        if i in special:
            L, at = special[i]
            take = rng.choice(others, L - 1, replace=False)
            take = np.concatenate([take[:at], [i], take[at:]])
        else:
            take = rng.choice(others, filler, replace=False)
        r.append(np.full(len(take), i))
        c.append(take)
    r, c = np.concatenate(r), np.concatenate(c)
    return Case("the diagonal first, in the middle and last in rows of %s entries, filler %d" % (LENGTHS, filler), n, n, r, c,
                rng.uniform(0.5, 1.5, len(r)) * rng.choice([-1.0, 1.0], len(r)))


def _nonfinite():
    """NaN and +-Inf on the diagonal (rows 2, 9, 30; row 41 stores Inf and -Inf: NaN) and off it (rows 4, 17, 33, which keep a
    finite diagonal, and row 50, which has none): the off-diagonal ones must not leak into any element."""
    C0 = _sparse("n", 60, 60, 5, 20295, diagonal_share=0.0)
    r, c, v = (np.array(C0.coo[f]) for f in ("row", "col", "val"))
    keep = ~np.isin(r, (50,)) | (c != 50)
    r, c, v = r[keep], c[keep], v[keep]
    er = [2, 9, 30, 41, 41, 4, 4, 17, 17, 33, 33, 50]
    ec = [2, 9, 30, 41, 41, 4, 5, 17, 3, 33, 59, 0]
    ev = [np.nan, np.inf, -np.inf, np.inf, -np.inf, 1.5, np.nan, -2.5, np.inf, 3.5, -np.inf, np.nan]
    return Case("NaN and Inf on and off the diagonal", 60, 60, np.concatenate([r, er]), np.concatenate([c, ec]), np.concatenate([v, ev]))


def _of_matrix(name, M):
    return Case(name, M.n, M.n, *(np.array(M.coo[f]) for f in ("row", "col", "val")))


@functools.lru_cache(maxsize=None)
def diag_cases():
    """The small matrices the diagonal kernels can go wrong on, built once and left unchanged."""
    return (
        _sparse("empty rows and rows without a diagonal, 0 to 4 entries", 300, 300, 4, 20296),
        _sparse("empty rows and rows without a diagonal, 0 to 6 entries", 301, 301, 6, 20297),
        Case("no entries at all", 5, 5, [], [], []),
        Case("one entry", 1, 1, [0], [0], [-3.25]),
        _signed_zeros(),
        _repeats(),
        _positions(0), _positions(2), _positions(20), _positions(40),
        _of_matrix("spd_long: three full rows", cg.spd_long()),
        _of_matrix("spd_shuffled: a random storage order", cg.spd_shuffled()),
        _sparse("300 x 200", 300, 200, 6, 20298),
        _sparse("200 x 300", 200, 300, 6, 20299),
        _nonfinite(),
    )
