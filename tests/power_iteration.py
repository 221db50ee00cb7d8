"""What the power-iteration tests are made of (iterate / normalize, include/smvp_amd.h): the normalisation as a pure function,
the host chain (one product, normalise on the host, hand the result back as the next operand), seeded square matrices and the
start vectors that put the first product into a chosen regime.  Plain functions, no fixtures: test_power_iteration_host.py
pins them against the oracle on the CPU, test_gpu_power_iteration.py compares the library's bits with them.

Why bits.  k chained steps compound their rounding, and no tight bound on that exists, so nothing here bounds it.  The loop
adds nothing to the products: on a path whose product is reproducible from run to run, k iterated steps must be bit for bit the
chain of k single products of the same handle with normalise() in between.  A maximum is exact in any order and an IEEE
division is correctly rounded, so normalise() has one right answer, numpy's."""
import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm

STEPS = (1, 2, 3, 6)                    # the result lies in either buffer of the x / y swap
TINY = np.finfo(np.float64).tiny        # the smallest normal double
PEAK_SMALL = (1003, (0, 63, 64, 255, 256, 1002))
PEAK_LARGE = (2048 * 256 + 1, (2048 * 256 - 1, 2048 * 256))   # the last element of the absmax grid's first trip, the only one of its second


# ------------------------------------------------------------------------------------------------------- the pure functions
def normalise(y):
    """y / m with m = max |y_r| over the non-NaN r; y itself where m is 0 (or nothing is left to take a maximum of)."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    a = np.abs(y)
    a = a[~np.isnan(a)]
    m = a.max() if a.size else 0.0
    if not m > 0.0:
        return y.copy()
    with np.errstate(all="ignore"):     # inf / inf, finite / inf, subnormal quotients
        return y / m


def host_chain(product, x0, steps, normalize):
    """(raw, iterates): raw[k] = product(operand k), iterates[k] = normalise(raw[k]) or raw[k]; operand 0 is x0, operand k + 1 is
    iterates[k].  product: numpy in, numpy out."""
    x = np.ascontiguousarray(x0, dtype=np.float64)
    raw, iterates = [], []
    for _ in range(steps):
        y = np.ascontiguousarray(product(x), dtype=np.float64)
        raw.append(y)
        x = normalise(y) if normalize else y.copy()
        iterates.append(x)
    return raw, iterates


def operands(x0, iterates):
    """The operand of every step of a chain."""
    return [np.ascontiguousarray(x0, dtype=np.float64)] + list(iterates[:-1])


def in_range(v):
    """Neither overflowed nor subnormal: every element finite and zero or at least the smallest normal double."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    return bool(np.isfinite(v).all() and (v[v != 0.0] >= TINY).all())


# ------------------------------------------------------------------------------------------------------------- the matrices
class Matrix:
    """A square matrix: its entries in storage order (coo) and the host converter's CSR arrays of them."""

    def __init__(self, n, rows, cols, vals):
        self.n = int(n)
        self.coo = sm.make_coo(rows, cols, vals)
        self.row_ptr, self.col_ind, self.val = sm.csr_from_coo(self.coo, self.n)
        self.nnz = len(self.coo)

    @property
    def csr(self):
        return self.row_ptr, self.col_ind, self.val

    def spmv(self, x):
        return ob.csr_spmv(self.row_ptr, self.col_ind, self.val, x)

    def iterate(self, x0, steps, normalize=False):
        return ob.csr_iterate(self.row_ptr, self.col_ind, self.val, x0, steps, normalize=normalize)

    def scale(self, x):
        """sum_j |a_rj x_j| per row: check_y's yardstick."""
        with np.errstate(all="ignore"):
            return ob.csr_spmv(self.row_ptr, self.col_ind, np.abs(self.val), np.abs(x))

    @property
    def terms(self):
        return np.diff(self.row_ptr)


def ones(M):
    return np.ones(M.n)


def random_x(M, seed=7):
    """A start vector of both signs, away from zero."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, M.n) * rng.choice([-1.0, 1.0], M.n)


def _values(rng, k):
    """Not dyadic, over four decades, both signs."""
    return rng.uniform(-1.0, 1.0, k) * 10.0 ** rng.integers(-2, 2, k)


def _entries(rng, n, lens):
    """(rows, cols) of rows of `lens` distinct columns, ascending inside every row."""
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.sort(rng.choice(n, int(l), replace=False)) for l in lens] + [np.zeros(0, dtype=np.int64)])
    return rows, cols.astype(np.int64)


def _rescaled(n, rows, cols, vals):
    """The values divided by the sixth root of what six un-normalised steps from ones grow to: those steps stay near 1."""
    M = Matrix(n, rows, cols, vals)
    with np.errstate(all="ignore"):
        growth = np.abs(M.iterate(np.ones(n), 6)).max()
    assert np.isfinite(growth) and growth > 0.0
    return vals / growth ** (1.0 / 6.0)


def _short_parts():
    rng = np.random.default_rng(20250)
    n = 1003
    lens = rng.integers(0, 9, n)
    rows, cols = _entries(rng, n, lens)
    return n, rows, cols, _rescaled(n, rows, cols, _values(rng, len(rows)))


def short():
    """n = 1003, rows of 0 to 8 entries (some empty), columns ascending."""
    return Matrix(*_short_parts())


def long():
    """n = 700, rows of 0 to 40 entries and three full rows of 700: those cross the tiles of every size."""
    rng = np.random.default_rng(20251)
    n = 700
    lens = rng.integers(0, 41, n)
    lens[[5, 350, 699]] = n
    rows, cols = _entries(rng, n, lens)
    return Matrix(n, rows, cols, _rescaled(n, rows, cols, _values(rng, len(rows))))


def shuffled():
    """The entries of short() and 25 repeated (row, col) pairs with values of their own, in a random storage order: a row's TJDS
    order is no longer its CSR order, and the converters have ties to keep in input order."""
    n, rows, cols, vals = _short_parts()
    rng = np.random.default_rng(20252)
    again = rng.choice(len(rows), 25, replace=False)
    rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
    vals = np.concatenate([vals, _values(rng, 25) * np.abs(vals).mean()])
    order = rng.permutation(len(rows))
    return Matrix(n, rows[order], cols[order], vals[order])


def peak(n, p, sign):
    """1 to 3 entries per row with sum |val| <= 1.5 in every row, except row p, whose only entry is (p, p) = sign * 3.  From
    ones, element p of iterate k is (sign * 3)^k and every other element at most 1.5 * 3^(k - 1) in magnitude: the largest
    magnitude of every iterate is at index p alone, and with sign = -1 its sign alternates."""
    rng = np.random.default_rng(20253 + n % 1000 + p)
    lens = rng.integers(1, 4, n)
    step = rng.integers(1, n // 3, (n, 3))                      # distinct columns: base, base + d1, base + d1 + d2 (mod n)
    cols = (rng.integers(0, n, n)[:, None] + np.cumsum(step, axis=1) - step[:, :1]) % n
    keep = np.arange(3)[None, :] < lens[:, None]
    keep[p] = False
    rows = np.broadcast_to(np.arange(n)[:, None], (n, 3))[keep]
    cols = cols[keep]
    vals = rng.uniform(-0.5, 0.5, len(rows))
    rows, cols, vals = np.append(rows, p), np.append(cols, p), np.append(vals, sign * 3.0)
    order = np.lexsort((cols, rows))
    return Matrix(n, rows[order], cols[order], vals[order])


def square_zero():
    """n = 300, entries only in rows < 150 and columns >= 150: A^2 = 0.  Iterate 1 from ones is not zero, iterate 2 is +0.0 in
    every element (its maximum is 0: the vector is left alone, no 0 / 0), iterate 3 again."""
    rng = np.random.default_rng(20254)
    n, h = 300, 150
    lens = np.concatenate([rng.integers(1, 9, h), np.zeros(n - h, dtype=np.int64)])
    rows = np.repeat(np.arange(n), lens)
    cols = np.concatenate([np.sort(rng.choice(n - h, int(l), replace=False)) + h for l in lens[:h]])
    return Matrix(n, rows, cols, _values(rng, len(rows)))


def small_integers():
    """n = 1003, rows of 0 to 8 entries, values in {-2, -1, 1, 2}: from ones every partial sum of five steps is an integer far
    below 2^53, so any order of summation -- TJDS ATOMIC's -- is exact."""
    rng = np.random.default_rng(20255)
    n = 1003
    lens = rng.integers(0, 9, n)
    rows, cols = _entries(rng, n, lens)
    return Matrix(n, rows, cols, rng.choice([-2.0, -1.0, 1.0, 2.0], len(rows)))


def partial_sum_bound(M, x0, steps):
    """The largest |partial sum| any order of summation can meet in `steps` un-normalised steps: the iterates of |A| on |x0|."""
    v = np.abs(np.asarray(x0, dtype=np.float64))
    worst = 0.0
    for _ in range(steps):
        v = ob.csr_spmv(M.row_ptr, M.col_ind, np.abs(M.val), v)
        worst = max(worst, float(v.max()))
    return worst


def tiny_integers():
    """n = 5, small-integer values, no empty row: more ranks than rows."""
    rows = [0, 0, 1, 2, 2, 2, 3, 4, 4]
    cols = [0, 3, 1, 0, 2, 4, 3, 1, 4]
    return Matrix(5, rows, cols, [2.0, -1.0, 3.0, 1.0, 1.0, -2.0, 2.0, -1.0, 1.0])


# ----------------------------------------------------------------------------------------- start vectors of the special classes
def nan_case():
    """(short(), x): a NaN in the column most rows use -- some rows of the first product are NaN, not all."""
    M = short()
    x = random_x(M, 11)
    x[np.bincount(M.col_ind, minlength=M.n).argmax()] = np.nan
    return M, x


def overflow_case():
    """(matrix, x, q): values around 1e100 under an operand around 1e200 -- every product is finite (below 1e300, at most 8 to a
    row) except the one of row q, whose only entry is 1e110: exactly that row of the first product is +Inf.  The maximum is
    Inf: the finite rows become +-0.0 with their sign, row q becomes NaN."""
    rng = np.random.default_rng(20256)
    n, q = 300, 123
    lens = rng.integers(0, 9, n)
    lens[q] = 1
    rows, cols = _entries(rng, n, lens)
    vals = rng.uniform(0.1, 1.0, len(rows)) * rng.choice([-1.0, 1.0], len(rows)) * 1e100
    vals[rows == q] = 1e110
    x = rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n) * 1e200
    x[cols[rows == q]] = 0.5e200
    return Matrix(n, rows, cols, vals), x, q


def subnormal_case():
    """(small_integers(), x): small integers times 5e-324 -- the first product is exact and its largest magnitude subnormal."""
    M = small_integers()
    x = np.random.default_rng(20257).integers(-3, 4, M.n) * 5e-324
    return M, x
