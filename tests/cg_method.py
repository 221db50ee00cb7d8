"""The dot product and the conjugate gradients of include/smvp_amd.h (smvp_vector_dot, smvp_csr_cg / smvp_tjds_cg) restated in
numpy: the dot in the order of additions the header defines, the run with its stop rules.  Plain functions, no fixtures:
test_cg_host.py pins them to known answers on the CPU, test_gpu_cg.py compares the library's bits with them.

Why bits.  The header fixes the order of every addition of the dot, and everything else is one correctly rounded IEEE operation
per element: each number has one right answer.  The only input that is the library's own is the product, so run() takes it as a
function -- on the GPU the same handle's single product.

The dot is vectorised over lanes and workgroups; it pads with +0.0 terms, which the header allows (an accumulator that starts at
+0.0 never becomes -0.0, so adding +0.0 changes nothing).  The matrices are power_iteration.Matrix objects."""
import numpy as np

import power_iteration as pi

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = 0, 1, 2, 3      # SMVP_CG_*
BLOCK, GRID_CAP = 256, 2048
TRIP = BLOCK * GRID_CAP                                      # elements of one trip of the full grid


# ------------------------------------------------------------------------------------------------------------------- the dot
def fold256(c):
    """fold256 of every row of c (shape (..., 256)): inside each run of 64, c_j += c_{j+h} for h = 32 ... 1, then
    ((w0 + w1) + w2) + w3."""
    c = np.array(c, dtype=np.float64).reshape(c.shape[:-1] + (4, 64))
    with np.errstate(all="ignore"):
        for h in (32, 16, 8, 4, 2, 1):
            c = c[..., :h] + c[..., h:2 * h]
        w = c[..., 0]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _lanes(t, width):
    """Lane s of `width` starts at +0.0 and adds t_s, t_{s + width}, ... in ascending order (t padded with +0.0)."""
    trips = -(-len(t) // width)
    padded = np.zeros(trips * width)
    padded[:len(t)] = t
    acc = np.zeros(width)
    with np.errstate(all="ignore"):
        for row in padded.reshape(trips, width):
            acc = acc + row
    return acc


def dot(a, b):
    """dot(a, b) as the header defines it, a numpy float64."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    n = len(a)
    assert len(b) == n
    if n == 0:
        return np.float64(0.0)
    G = min(-(-n // BLOCK), GRID_CAP)
    with np.errstate(all="ignore"):
        t = a * b                                                                    # the terms, rounded
    partials = fold256(_lanes(t, BLOCK * G).reshape(G, BLOCK))
    return np.float64(fold256(_lanes(partials, BLOCK)))


# ------------------------------------------------------------------------------------------------------------------- the run
def run(product, b, x0, max_steps, tol):
    """(steps, updates, reason, rr_each, sigma_each, x): the run as the header defines it; there is no check_every in it, because
    nothing depends on it.  product: numpy in, numpy out."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    tol = np.float64(tol)
    with np.errstate(all="ignore"):
        bb = dot(b, b)
        thr = (tol * tol) * bb
        if x0 is None:
            x, r = np.zeros(len(b)), b.copy()
        else:
            x = np.ascontiguousarray(x0, dtype=np.float64).copy()
            r = b - np.ascontiguousarray(product(x), dtype=np.float64)
        p = r.copy()
        rho = dot(r, r)
        rrs, sigmas = [rho], []
        if not (np.isfinite(bb) and np.isfinite(rho)):
            return 0, 0, NONFINITE, np.array(rrs), np.array(sigmas), x
        if rho <= thr:
            return 0, 0, CONVERGED, np.array(rrs), np.array(sigmas), x
        k = 0
        while True:
            k += 1
            q = np.ascontiguousarray(product(p), dtype=np.float64)
            sigma = dot(p, q)
            sigmas.append(sigma)
            if not np.isfinite(sigma):
                return k, k - 1, NONFINITE, np.array(rrs), np.array(sigmas), x
            if not sigma > 0.0:
                return k, k - 1, BREAKDOWN, np.array(rrs), np.array(sigmas), x
            alpha = rho / sigma
            x = x + alpha * p                                                        # alpha * p is an array of its own: rounded first
            r = r - alpha * q
            rho_new = dot(r, r)
            rrs.append(rho_new)
            reason = NONFINITE if not np.isfinite(rho_new) else CONVERGED if rho_new <= thr else MAX_STEPS if k == max_steps else None
            if reason is not None:
                return k, k, reason, np.array(rrs), np.array(sigmas), x
            beta = rho_new / rho
            p = r + beta * p
            rho = rho_new


# ---------------------------------------------------------------------------------------------------------------- the matrices
def _spd_parts(n, seed):
    """(rows, cols, vals) of B + B^T without a diagonal: B has 0 to 4 entries per row at random columns off the diagonal, values
    in [-0.1, 0.1]."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5, n)
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, len(rows))
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    vals = rng.uniform(-0.1, 0.1, len(rows))
    return rng, np.concatenate([rows, cols]), np.concatenate([cols, rows]), np.concatenate([vals, vals])


def _with_diagonal(rng, n, rows, cols, vals):
    """The entries and a diagonal D_ii = sum_j |a_ij| + U[0.5, 1.5]: strictly diagonally dominant with a positive diagonal, hence
    symmetric positive definite when the rest is symmetric."""
    d = np.bincount(rows, weights=np.abs(vals), minlength=n) + rng.uniform(0.5, 1.5, n)
    return np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)]), np.concatenate([vals, d])


def spd(n, seed=20270):
    """A = B + B^T + D, n x n."""
    rng, rows, cols, vals = _spd_parts(n, seed)
    return pi.Matrix(n, *_with_diagonal(rng, n, rows, cols, vals))


def spd_long():
    """n = 700: spd's construction plus three full rows and the matching columns of values in +-1e-3 -- they cross the tiles of
    every size -- with the diagonal raised by their row sums."""
    n = 700
    rng, rows, cols, vals = _spd_parts(n, 20271)
    for i in (5, 350, 699):
        j = np.delete(np.arange(n), i)
        v = rng.uniform(-1e-3, 1e-3, n - 1)
        rows = np.concatenate([rows, np.full(n - 1, i), j])
        cols = np.concatenate([cols, j, np.full(n - 1, i)])
        vals = np.concatenate([vals, v, v])
    return pi.Matrix(n, *_with_diagonal(rng, n, rows, cols, vals))


def spd_shuffled():
    """spd(1003)'s entries in a random storage order with 25 (i, j) / (j, i) pairs repeated (and the diagonal raised by them): a
    row's TJDS order is no longer its CSR order, and the matrix stays symmetric and dominant."""
    n = 1003
    rng, rows, cols, vals = _spd_parts(n, 20270)
    half = len(rows) // 2
    again = rng.choice(half, 25, replace=False)
    extra = rng.uniform(-0.1, 0.1, 25)
    ri, ci = rows[again], cols[again]
    rows, cols = np.concatenate([rows, ri, ci]), np.concatenate([cols, ci, ri])
    vals = np.concatenate([vals, extra, extra])
    rows, cols, vals = _with_diagonal(rng, n, rows, cols, vals)
    order = rng.permutation(len(rows))
    return pi.Matrix(n, rows[order], cols[order], vals[order])


def identity(n):
    return pi.Matrix(n, np.arange(n), np.arange(n), np.ones(n))


def minus_identity(n):
    return pi.Matrix(n, np.arange(n), np.arange(n), -np.ones(n))


def swap2():
    return pi.Matrix(2, [0, 1], [1, 0], [1.0, 1.0])


def nan_value(n=300):
    """spd(n) with one off-diagonal pair of values replaced by NaN: the first product of a full vector has NaN elements."""
    M = spd(n)
    rows, cols, vals = (np.array(M.coo[f]) for f in ("row", "col", "val"))
    off = np.flatnonzero(rows != cols)[0]
    pair = ((rows == rows[off]) & (cols == cols[off])) | ((rows == cols[off]) & (cols == rows[off]))
    vals[pair] = np.nan
    return pi.Matrix(n, rows, cols, vals)


def dense(M):
    """The matrix as a dense array (repeated entries add up)."""
    rows, cols, vals = (np.array(M.coo[f]) for f in ("row", "col", "val"))
    A = np.zeros((M.n, M.n))
    np.add.at(A, (rows, cols), vals)
    return A


def rhs(n, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n)
