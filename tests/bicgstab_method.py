"""BiCGSTAB as include/smvp_amd.h defines it (smvp_csr_bicgstab / smvp_tjds_bicgstab, kernel K13) restated in numpy: the run with
its four stop rules, around cg_method.py's order-defined dot.  Plain functions, no fixtures: test_bicgstab_host.py pins them to
known answers on the CPU, test_gpu_bicgstab.py compares the library's bits with them.

Why bits.  As for conjugate gradients: the header fixes the order of every addition of the dot, everything else is one correctly
rounded IEEE operation per element, and the only input that is the library's own is the product, which run() takes as a function --
on the GPU the same handle's single product.  There is no check_every in run(), because nothing depends on it.

The matrices are power_iteration.Matrix objects: general square matrices that conjugate gradients cannot solve."""
import numpy as np

import power_iteration as pi
from cg_method import dot, dense, rhs, identity, minus_identity, swap2, TRIP  # noqa: F401  (the small cases are shared)

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = 0, 1, 2, 3      # SMVP_BICGSTAB_*


# ------------------------------------------------------------------------------------------------------------------- the run
def run(product, b, x0, max_steps, tol, trace=None):
    """(steps, full, half, reason, rr_each, ss_each, x): the run as the header defines it.  product: numpy in, numpy out.  Every
    array expression below is an array of its own: each product is rounded before the sum that uses it.  trace: a list that
    receives r_0, r_1, ... r_full, the residuals whose squared norms rr_each holds."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    tol = np.float64(tol)

    def mul(y):
        return np.ascontiguousarray(product(y), dtype=np.float64)

    with np.errstate(all="ignore"):
        bb = dot(b, b)
        thr = (tol * tol) * bb
        if x0 is None:
            x, r = np.zeros(len(b)), b.copy()
        else:
            x = np.ascontiguousarray(x0, dtype=np.float64).copy()
            r = b - mul(x)
        rhat, p = r.copy(), r.copy()
        rho = dot(r, r)
        rrs, sss = [rho], []
        if trace is not None:
            trace.append(r.copy())

        def end(steps, full, half, reason):
            return steps, full, half, reason, np.array(rrs), np.array(sss), x

        if not (np.isfinite(bb) and np.isfinite(rho)):
            return end(0, 0, 0, NONFINITE)
        if rho <= thr:
            return end(0, 0, 0, CONVERGED)
        k = 0
        while True:
            k += 1
            v = mul(p)
            sigma = dot(rhat, v)
            if not np.isfinite(sigma):                                               # rule A
                return end(k, k - 1, 0, NONFINITE)
            if sigma == 0.0:
                return end(k, k - 1, 0, BREAKDOWN)
            alpha = rho / sigma
            s = r - alpha * v
            ss = dot(s, s)
            sss.append(ss)
            if not np.isfinite(ss):                                                  # rule H
                return end(k, k - 1, 0, NONFINITE)
            if ss <= thr:
                x = x + alpha * p
                return end(k, k - 1, 1, CONVERGED)
            t = mul(s)
            ts, tt = dot(t, s), dot(t, t)
            if not (np.isfinite(ts) and np.isfinite(tt)):                            # rule T
                return end(k, k - 1, 0, NONFINITE)
            if not tt > 0.0:
                x = x + alpha * p
                return end(k, k - 1, 1, BREAKDOWN)
            omega = ts / tt
            x = (x + alpha * p) + omega * s
            r = s - omega * t
            rr, rho_new = dot(r, r), dot(rhat, r)
            rrs.append(rr)
            if trace is not None:
                trace.append(r.copy())
            if not (np.isfinite(rr) and np.isfinite(rho_new)):                       # rule B, the first that holds
                return end(k, k, 0, NONFINITE)
            if rr <= thr:
                return end(k, k, 0, CONVERGED)
            if k == max_steps:
                return end(k, k, 0, MAX_STEPS)
            if omega == 0.0 or rho_new == 0.0:
                return end(k, k, 0, BREAKDOWN)
            beta = (rho_new / rho) * (alpha / omega)
            p = r + beta * (p - omega * v)
            rho = rho_new


# ---------------------------------------------------------------------------------------------------------------- the matrices
def _nonsym_parts(n, seed):
    """(rng, rows, cols, vals) without a diagonal: 0 to 8 entries per row at random columns off the diagonal, values in
    [-0.1, 0.1], NOT mirrored."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 9, n)
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, len(rows))
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    vals = rng.uniform(-0.1, 0.1, len(rows))
    return rng, rows, cols, vals


def _with_diagonal(rng, n, rows, cols, vals):
    """The entries and a diagonal D_ii = sum_j |a_ij| + U[0.5, 1.5]: strictly row-diagonally dominant, hence non-singular."""
    d = np.bincount(rows, weights=np.abs(vals), minlength=n) + rng.uniform(0.5, 1.5, n)
    return np.concatenate([rows, np.arange(n)]), np.concatenate([cols, np.arange(n)]), np.concatenate([vals, d])


def nonsym(n, seed=20290):
    """n x n, strictly row-diagonally dominant and not symmetric (for n large enough to hold an off-diagonal entry)."""
    rng, rows, cols, vals = _nonsym_parts(n, seed)
    return pi.Matrix(n, *_with_diagonal(rng, n, rows, cols, vals))


def nonsym_long():
    """n = 700: nonsym's construction plus three full rows (5, 350, 699) of values in +-1e-3 -- they cross the tiles of every size
    -- with the diagonal raised by their row sums."""
    n = 700
    rng, rows, cols, vals = _nonsym_parts(n, 20291)
    for i in (5, 350, 699):
        j = np.delete(np.arange(n), i)
        rows = np.concatenate([rows, np.full(n - 1, i)])
        cols = np.concatenate([cols, j])
        vals = np.concatenate([vals, rng.uniform(-1e-3, 1e-3, n - 1)])
    return pi.Matrix(n, *_with_diagonal(rng, n, rows, cols, vals))


def nonsym_shuffled():
    """nonsym(1003)'s entries in a random storage order with 25 (i, j) pairs repeated (and the diagonal raised by them): a row's
    TJDS order is no longer its CSR order, and the matrix stays dominant."""
    n = 1003
    rng, rows, cols, vals = _nonsym_parts(n, 20290)
    again = rng.choice(len(rows), 25, replace=False)
    rows, cols = np.concatenate([rows, rows[again]]), np.concatenate([cols, cols[again]])
    vals = np.concatenate([vals, rng.uniform(-0.1, 0.1, 25)])
    rows, cols, vals = _with_diagonal(rng, n, rows, cols, vals)
    order = rng.permutation(len(rows))
    return pi.Matrix(n, rows[order], cols[order], vals[order])


def banded(n):
    """Tridiagonal and not symmetric: 2 + (i mod 7) / 8 on the diagonal, -3/4 below, -1/4 above.  Cheap to build at any n, strictly
    row-dominant, and its diagonal is not constant: Jacobi changes the run."""
    i = np.arange(n)
    rows = np.concatenate([i, i[1:], i[:-1]])
    cols = np.concatenate([i, i[1:] - 1, i[:-1] + 1])
    vals = np.concatenate([2.0 + (i % 7) / 8.0, np.full(n - 1, -0.75), np.full(n - 1, -0.25)])
    return pi.Matrix(n, rows, cols, vals)


def dense3(a):
    """A small matrix from its rows, the entries that are not zero stored."""
    a = np.array(a, dtype=np.float64)
    i, j = np.nonzero(a)
    return pi.Matrix(len(a), i, j, a[i, j])


def rule_t():
    """(A, b): s = (0, -1, 1), t = A s = 0, tt = 0 -> (1, 0, 1, BREAKDOWN) with x = (-1, 0, 0)."""
    return dense3([[-1, -1, -1], [-1, -1, -1], [1, -1, -1]]), np.array([1.0, 0.0, 0.0])


def rule_b():
    """(A, b): ts = 0, omega = 0, rho_1 = 0, rr_1 = 1 -> (1, 1, 0, BREAKDOWN) with x = (-0.5, -0.5, 0)."""
    return dense3([[-1, -1, -1], [-1, -1, -1], [-1, -1, 0]]), np.array([1.0, 1.0, 0.0])


def nan_value(n=300):
    """nonsym(n) with one off-diagonal value replaced by NaN: the first product of a full vector has a NaN element."""
    M = nonsym(n)
    rows, cols, vals = (np.array(M.coo[f]) for f in ("row", "col", "val"))
    vals[np.flatnonzero(rows != cols)[0]] = np.nan
    return pi.Matrix(n, rows, cols, vals)
