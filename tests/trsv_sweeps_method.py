"""Jacobi sweeps on a triangular system as a plan (include/smvp_amd.h: smvp_csr_trsv_create_sweeps, kernel K21) restated in numpy.
Plain functions, no fixtures: test_trsv_sweeps_host.py pins them to hand-computed values, to trsv_method.solve and to a derived
bound on the CPU, test_gpu_trsv_sweeps.py compares the library's bits with them.

Why bits.  Every sweep reads only the previous iterate; row i's sum starts at +0.0 and takes the row's stored entries inside the
triangle in ascending storage position, each product rounded before it is added; then one subtraction and one division.  So every
element of every iterate has one right answer.  The loop below runs over the place an entry has among its row's entries inside the
triangle and is vectorised ACROSS rows: step j adds the j-th such entry of every row that has one, as one rounded numpy
multiplication and one rounded numpy addition per row -- each row's additions happen in its storage order, one at a time.  (numpy's
elementwise float64 operations are IEEE's; no step fuses a product with a sum.)  Skipped entries are left out, which is adding +0.0."""
import numpy as np

import trsv_method as tm
from trsv_method import LOWER, STORED, UNIT, UPPER   # noqa: F401

MAX_SWEEPS = 4096


def kinds(M, uplo, diag):
    """Of every entry in storage order: 0 skipped, 1 inside the triangle, 2 on the diagonal (skipped where the diagonal is unit)."""
    r, c, _ = M.entries()
    k = np.where((c < r) if uplo == LOWER else (c > r), 1, 0)
    if diag == STORED:
        k[c == r] = 2
    return k


def ranges(M, uplo, diag):
    """(begin, end): per row the smallest range of storage positions that holds all of the row's entries inside the triangle and
    (STORED) on the diagonal; [row_ptr[i], row_ptr[i]) for a row that has none."""
    row_ptr = np.asarray(M.csr[0], dtype=np.int64)
    r, _, _ = M.entries()
    pos = np.flatnonzero(kinds(M, uplo, diag))
    first, last = np.full(M.n, np.iinfo(np.int64).max), np.full(M.n, -1, dtype=np.int64)
    np.minimum.at(first, r[pos], pos)
    np.maximum.at(last, r[pos], pos)
    has = last >= 0
    return np.where(has, first, row_ptr[:-1]).astype(np.int32), np.where(has, last + 1, row_ptr[:-1]).astype(np.int32)


def entries(M, uplo, diag):
    """What smvp_trsv_info reports as `entries` for a sweeps plan: the stored entries inside the ranges."""
    begin, end = ranges(M, uplo, diag)
    return int((end.astype(np.int64) - begin).sum())


def _steps(rows, n):
    """The entries at `rows` (ascending, one row's entries in storage order) grouped by their place in their row: a list of index
    arrays into `rows`, step j holding the j-th entry of every row that has one."""
    if len(rows) == 0:
        return []
    counts = np.bincount(rows, minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)])
    place = np.arange(len(rows)) - start[rows]
    order = np.argsort(place, kind="stable")
    cut = np.concatenate([[0], np.cumsum(np.bincount(place))])
    return [order[cut[j]:cut[j + 1]] for j in range(len(cut) - 1)]


def _summed(n, rows, terms, steps):
    s = np.zeros(n)
    for at in steps:
        s[rows[at]] = s[rows[at]] + terms[at]
    return s


def solve(M, uplo, diag, b, sweeps, within=None):
    """x(sweeps) of the header's iteration on the `uplo` triangle of M as stored.  within = (begin, end): only the entries at the
    storage positions begin_i <= p < end_i of row i are looked at (what the kernel does with ranges())."""
    return iterates(M, uplo, diag, b, sweeps, within)[sweeps]


def iterates(M, uplo, diag, b, sweeps, within=None):
    """[x(0), ..., x(sweeps)]: every iterate on the way, each an array of its own."""
    assert 0 <= sweeps <= MAX_SWEEPS
    r, c, v = M.entries()
    k = kinds(M, uplo, diag)
    if within is not None:
        p = np.arange(len(r))
        k = np.where((p >= np.asarray(within[0])[r]) & (p < np.asarray(within[1])[r]), k, 0)
    b = np.asarray(b, dtype=np.float64)
    off, on = np.flatnonzero(k == 1), np.flatnonzero(k == 2)
    off_steps = _steps(r[off], M.n)
    with np.errstate(all="ignore"):
        d = _summed(M.n, r[on], v[on], _steps(r[on], M.n))
        xs = [(b - 0.0) if diag == UNIT else (b - 0.0) / d]
        for _ in range(sweeps):
            s = _summed(M.n, r[off], v[off] * xs[-1][c[off]], off_steps)
            xs.append((b - s) if diag == UNIT else (b - s) / d)
    return xs
