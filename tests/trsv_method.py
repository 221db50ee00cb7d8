"""Sparse triangular solves on a CSR handle (include/smvp_amd.h: smvp_csr_trsv_create / smvp_trsv_solve, kernel K15) restated in
numpy and plain Python.  Plain functions, no fixtures: test_trsv_host.py pins them to hand-computed values and to a derived
backward-error bound on the CPU, test_gpu_trsv.py compares the library's bits with them.

Why bits.  Row i's two sums start at +0.0 and take the row's stored entries in ascending storage position, each product rounded
before it is added; then one subtraction and one division.  Every x_i has one right answer, the serial substitution loop's.  The
inner sums below run on Python floats, which are the machine's IEEE doubles (the same operations as np.float64 scalars, without the
per-operation cost); the subtraction and the division are np.float64's, so a zero diagonal gives +-Inf or NaN instead of raising."""
import functools
import os

import numpy as np

import cg_method as cg
import pcg_method as pcg

LOWER, UPPER = 0, 1
STORED, UNIT = 0, 1
ARRAYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arrays")
SAMPLES = ("ibm32", "curtis54", "memplus", "pwt", "pdp08-pg4")


# ------------------------------------------------------------------------------------------------------------------ the schedule
def levels(rows, row_ptr, col_ind, uplo):
    """level_of_row: 0 where the row has no stored off-diagonal entry inside the triangle, else 1 + the largest level of the rows
    those entries name.  Structural: values are not looked at."""
    rp, ci = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist()
    level = [0] * rows
    for i in (range(rows) if uplo == LOWER else range(rows - 1, -1, -1)):
        lv = 0
        for p in range(rp[i], rp[i + 1]):
            c = ci[p]
            if (c < i) if uplo == LOWER else (c > i):
                lv = max(lv, level[c] + 1)
        level[i] = lv
    return np.array(level, dtype=np.int32)


def schedule(level_of_row):
    """(level_ptr, order): the rows by (level, row index) ascending, and where each level begins in that list."""
    level_of_row = np.asarray(level_of_row, dtype=np.int64)
    order = np.argsort(level_of_row, kind="stable").astype(np.int32)
    counts = np.bincount(level_of_row) if len(level_of_row) else np.zeros(0, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order


def launches(widths, chain_width):
    """Kernels one solve enqueues: every level wider than chain_width is one, every maximal run of levels that are not is one."""
    n, in_chain = 0, False
    for w in widths:
        thin = w <= chain_width
        if not thin or not in_chain:
            n += 1
        in_chain = thin
    return n


def chains(widths, chain_width):
    return launches(widths, chain_width) - sum(1 for w in widths if w > chain_width)


# ------------------------------------------------------------------------------------------------------------------- the solve
def solve(M, uplo, diag, b, finite=True):
    """x of T x = b for the `uplo` triangle of M as stored: the loop of the header.  Where the case claims a finite answer
    (finite=True) that is asserted."""
    row_ptr, col_ind, val = M.csr
    rp, ci, va = np.asarray(row_ptr).tolist(), np.asarray(col_ind).tolist(), np.asarray(val, dtype=np.float64).tolist()
    bl = np.asarray(b, dtype=np.float64).tolist()
    x = [0.0] * M.n
    with np.errstate(all="ignore"):
        for i in (range(M.n) if uplo == LOWER else range(M.n - 1, -1, -1)):
            s, d = 0.0, 0.0
            for p in range(rp[i], rp[i + 1]):
                c = ci[p]
                if c == i:
                    if diag == STORED:
                        d = d + va[p]
                elif (c < i) if uplo == LOWER else (c > i):
                    s = s + va[p] * x[c]
            x[i] = float(np.float64(bl[i]) - np.float64(s)) if diag == UNIT else float((np.float64(bl[i]) - np.float64(s)) / np.float64(d))
    x = np.array(x, dtype=np.float64)
    if finite:
        assert np.isfinite(x).all(), "%s: the restatement's own result is not finite at %r" % (M.name, np.flatnonzero(~np.isfinite(x))[:5])
    return x


def rhs(n, seed=15):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)


# ---------------------------------------------------------------------------------------------------------------- the matrices
class Case:
    """A square matrix from its entries in storage order: CSR arrays that keep that order inside every row (a stable sort by row:
    the columns of a row are NOT ascending unless the entries came so).  finite_stored: the case claims that DIAG_STORED solves are
    finite (every row has a stored diagonal whose sum is not zero); DIAG_UNIT solves of every case here are."""

    def __init__(self, name, n, r, c, v, finite_stored=True, b=None):
        self.name, self.n, self.finite_stored, self.b = name, int(n), finite_stored, b
        r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int32)
        order = np.argsort(r, kind="stable")
        row_ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=self.n))]).astype(np.int32)
        self.csr = row_ptr, np.ascontiguousarray(c[order]), np.ascontiguousarray(np.asarray(v, dtype=np.float64)[order])
        self.nnz = len(r)
        self._ref = {}

    @classmethod
    def of_csr(cls, name, n, row_ptr, col_ind, val, finite_stored=True):
        row_ptr = np.asarray(row_ptr)
        return cls(name, n, np.repeat(np.arange(n), np.diff(row_ptr)), col_ind, val, finite_stored)

    def entries(self):
        """(row, col, val) of every entry in storage order."""
        row_ptr, col_ind, val = self.csr
        return np.repeat(np.arange(self.n), np.diff(row_ptr)), col_ind, val

    def facts(self, uplo, diag):
        """What smvp_trsv_info and smvp_trsv_schedule report, from the restatement (computed once per uplo)."""
        key = ("facts", uplo)
        if key not in self._ref:
            row_ptr, col_ind, _ = self.csr
            level = levels(self.n, row_ptr, col_ind, uplo)
            level_ptr, order = schedule(level)
            r, c, _ = self.entries()
            inside = (c < r) if uplo == LOWER else (c > r)
            self._ref[key] = dict(level_of_row=level, level_ptr=level_ptr, order=order, levels=len(level_ptr) - 1,
                                  widths=np.diff(level_ptr), max_level_width=int(np.diff(level_ptr).max()) if self.n else 0,
                                  missing_diagonals=self.n - len(np.unique(r[c == r])), off=int(inside.sum()), on=int((c == r).sum()))
        f = dict(self._ref[key])
        f["entries"] = f["off"] + (f["on"] if diag == STORED else 0)
        return f

    def reference(self, uplo, diag):
        """(b, x): the right-hand side of this case and the restatement's solution, computed once, shared, left unchanged."""
        key = (uplo, diag)
        if key not in self._ref:
            b = rhs(self.n) if self.b is None else np.array(self.b, dtype=np.float64)
            x = solve(self, uplo, diag, b, finite=diag == UNIT or self.finite_stored)
            b.setflags(write=False)
            x.setflags(write=False)
            self._ref[key] = (b, x)
        return self._ref[key]


def dominant(name, n, r, c, seed, finite_stored=True):
    """Values on a given structure (entries in storage order): the off-diagonal magnitudes of every row, both triangles together,
    sum to at most 1/2, every stored diagonal entry lies in [1, 2].  So row i gives |x_i| <= |b_i| + |x|_inf / 2 for either diag
    setting (a stored diagonal is at least 1), hence |x|_inf <= 2 |b|_inf: finite wherever every row has a diagonal."""
    rng = np.random.default_rng(seed)
    r, c = np.asarray(r, dtype=np.int64), np.asarray(c, dtype=np.int64)
    off = r != c
    per_row = np.bincount(r[off], minlength=n)
    v = rng.uniform(1.0, 2.0, len(r))
    v[off] = rng.uniform(-1.0, 1.0, int(off.sum())) * (0.499 / per_row[r[off]])    # (0.499: the sum stays under 1/2 after rounding)
    return Case(name, n, r, c, v, finite_stored)


def flipped(M):
    """The matrix with rows and columns renumbered n - 1 - i (storage order kept): the lower triangle becomes the upper one with
    the same levels, so every constructed schedule is also an UPPER case."""
    r, c, v = M.entries()
    return Case(M.name + ", flipped", M.n, M.n - 1 - r, M.n - 1 - c, v, M.finite_stored)


def sample(name):
    """A golden sample's structure with dominant values (pdp08-pg4 stores 5 of its 6 diagonal entries: DIAG_STORED is not finite)."""
    g = np.load(os.path.join(ARRAYS, name + ".npz"), allow_pickle=False)
    n, row_ptr, col_ind = int(g["rows"]), g["row_ptr"], g["col_ind"]
    assert n == int(g["cols"])
    r = np.repeat(np.arange(n), np.diff(row_ptr))
    has_all = len(np.unique(r[col_ind == r])) == n
    return dominant(name, n, r, col_ind, 20300 + len(name), finite_stored=has_all)


def identity(n):
    return dominant("identity(%d)" % n, n, np.arange(n), np.arange(n), 20310)


def bidiagonal(n):
    """(i, i - 1) and (i, i): n levels of one row each."""
    i = np.arange(n)
    return dominant("bidiagonal(%d)" % n, n, np.concatenate([i[1:], i]), np.concatenate([i[:-1], i]), 20311)


def dense_lower(n):
    """Every (i, j) with j <= i: n levels, rows longer than a wavefront."""
    r, c = np.tril_indices(n)
    return dominant("dense_lower(%d)" % n, n, r, c, 20312)


def leveled(name, widths, deps, seed, shuffle=True):
    """A lower-triangular structure with the given level widths: rows are numbered level by level; a row of level l > 0 has
    deps(l, k) off-diagonal entries (k: its place in the level), the first at a row of level l - 1 -- which fixes its level -- the
    others anywhere in the levels before (drawn with replacement: repeats happen), and one diagonal entry; the entries of a row
    stand in a random storage order."""
    rng = np.random.default_rng(seed)
    start = np.concatenate([[0], np.cumsum(widths)])
    r, c = [], []
    for l, w in enumerate(widths):
        for k in range(w):
            i = start[l] + k
            cols = [i]
            if l > 0:
                m = max(1, deps(l, k))
                cols += [rng.integers(start[l - 1], start[l])] + rng.integers(0, start[l], m - 1).tolist()
            cols = np.array(cols)
            if shuffle:
                cols = cols[rng.permutation(len(cols))]
            r += [i] * len(cols)
            c += cols.tolist()
    M = dominant(name, int(start[-1]), r, c, seed + 1)
    assert (np.diff(M.facts(LOWER, STORED)["level_ptr"]) == np.asarray(widths)).all(), name
    return M


def wide_thin_wide(w):
    """A level of 3w rows, five levels of at most w, a level of w + 1 rows that depend on the thin ones, then a thin tail: a wide
    launch hands over to a chain, the chain to a wide launch, that to a chain."""
    return leveled("wide_thin_wide(%d)" % w, [3 * w, w, 1, w - 1, 7, w, w + 1, 3, 1], lambda l, k: 1 + (k + l) % 4, 20313)


def adjacent(w):
    """Levels of exactly w and w + 1 rows next to each other: the threshold between the two kernels."""
    return leveled("adjacent(%d)" % w, [w, w + 1, w, w + 1, w], lambda l, k: 1 + k % 3, 20314)


def divergent(w):
    """A chain whose rows have 1 or 300 entries inside the triangle, neighbouring lanes the one and the other, and most lanes of the
    workgroup no row at all: no lane may run ahead of the barrier between two levels."""
    return leveled("divergent(%d)" % w, [6, 5, 6, 5, 6, 5], lambda l, k: 300 if (k + l) % 2 else 1, 20315)


def interleaved(n, levels_=4):
    """Row i has level i % 4 and depends on rows i - 1, i - 5 and i - 9 (level i % 4 - 1, where they exist): the elements of x a row
    reads lie between elements that rows of its own level and of later levels have yet to write, in the same cache lines.  With n
    / 4 <= chain_width everything is one chain; wider levels are launches of their own."""
    r, c = [], []
    for i in range(n):
        cols = [i] + ([j for j in (i - 1, i - 5, i - 9) if j >= 0] if i % levels_ else [])
        r += [i] * len(cols)
        c += cols
    M = dominant("interleaved(%d)" % n, n, r, c, 20316)
    assert (M.facts(LOWER, STORED)["level_of_row"] == np.arange(n) % levels_).all()
    return M


def order_dependent():
    """Row 3's sum depends on the order of its additions: with b all ones x_0 = x_1 = x_2 = 1, and (1e16 + 1) - 1e16 is 0 in the
    stored order (columns 1, 2, 0) where (-1e16 + 1e16) + 1 is 1 with the columns sorted."""
    r = [0, 1, 2, 3, 3, 3, 3]
    c = [0, 1, 2, 1, 2, 0, 3]
    v = [1.0, 1.0, 1.0, 1e16, 1.0, -1e16, 1.0]
    return Case("order_dependent", 4, r, c, v, b=np.ones(4))


def sorted_copy(M):
    """The same entries with every row's columns ascending (ties in their stored order)."""
    r, c, v = M.entries()
    order = np.lexsort((c, r))
    return Case(M.name + ", sorted", M.n, r[order], c[order], v[order], M.finite_stored, M.b)


def triangle_of(M, uplo, zeros=False):
    """The `uplo` triangle of M with its diagonal as a matrix of its own (storage order kept); zeros=True stores an explicit 0.0 at
    every position of the other triangle instead of dropping it."""
    r, c, v = M.entries()
    keep = (c <= r) if uplo == LOWER else (c >= r)
    if zeros:
        return Case(M.name + ", other triangle zeroed", M.n, r, c, np.where(keep, v, 0.0), M.finite_stored, M.b)
    return Case(M.name + ", triangle", M.n, r[keep], c[keep], v[keep], M.finite_stored, M.b)


def of_matrix(name, M, as_stored=False):
    """A cg_method / pcg_method matrix (power_iteration.Matrix) as a Case: on the SAME CSR arrays (the host converter's: columns
    ascending, repeats in input order), or with as_stored=True on the entries in the order the matrix was given (a stable sort by
    row only: spd_shuffled's rows then hold their columns unsorted)."""
    if as_stored:
        return Case(name, M.n, M.coo["row"], M.coo["col"], M.coo["val"])
    return Case.of_csr(name, M.n, *M.csr)


@functools.lru_cache(maxsize=None)
def existing_cases():
    """The matrices the suite already has, and the five golden samples' structures with dominant values."""
    return tuple([of_matrix("spd(1003)", cg.spd(1003)), of_matrix("spd_long", cg.spd_long()), of_matrix("spd_shuffled", cg.spd_shuffled(), as_stored=True),
                  of_matrix("tridiagonal(300)", pcg.tridiagonal(300))] + [sample(name) for name in SAMPLES])


@functools.lru_cache(maxsize=None)
def constructed_cases(w):
    """The constructed schedules for a chain width of w, each with its flipped twin (an UPPER case of the same shape)."""
    lower = [identity(n) for n in (1, 2, w - 1, w, w + 1, 3 * w + 5)]
    lower += [bidiagonal(w + 1), bidiagonal(1003), dense_lower(70), wide_thin_wide(w), adjacent(w), divergent(w),
              interleaved(2 * w), interleaved(4 * w + 12)]
    return tuple(lower + [flipped(M) for M in lower[5:]])
