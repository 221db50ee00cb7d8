"""Conjugate gradients preconditioned by two triangular solves (include/smvp_amd.h: smvp_csr_pcg_tri / smvp_tjds_pcg_tri, kernel
K16) restated in numpy, on cg_method.py's dot and trsv_method.py's serial substitution.  Plain functions, no fixtures:
test_pcg_tri_host.py pins them to hand-computed values and known answers on the CPU, test_gpu_pcg_tri.py compares the library's
bits with them.

Why bits.  z = M^-1 r is two of K15's solves -- each element the serial substitution loop's -- with one rounded multiplication
between them; the dot's order is the header's; everything else is one correctly rounded IEEE operation per element, and the rules
are K14's in K14's order.  The only input that is the library's own is the product, so run() takes it as a function, as
pcg_method.run does.  A plan is a (trsv_method.Case, uplo, diag) triple."""
import functools

import numpy as np

import cg_method as cg
import pcg_method as pcg
import power_iteration as pi
import trsv_method as trsv

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = cg.CONVERGED, cg.MAX_STEPS, cg.BREAKDOWN, cg.NONFINITE
LOWER, UPPER, STORED, UNIT = trsv.LOWER, trsv.UPPER, trsv.STORED, trsv.UNIT

_solved = {}                                                     # (plan, operand's bytes) -> (the Case, kept alive; the solution)


def _solve(plan, b):
    """trsv_method.solve, remembered by plan and operand: the runs of one system on several product paths ask for the same solves
    again (a path whose product differed in a bit would ask for others and still get the loop's answer)."""
    M, uplo, diag = plan
    key = (id(M), uplo, diag, b.tobytes())
    if key not in _solved:
        x = trsv.solve(M, uplo, diag, b, finite=False)
        x.setflags(write=False)
        _solved[key] = (M, x)
    return _solved[key][1]


def apply(first, m, second, r):
    """z = T2^-1 (m .* (T1^-1 r)); the multiplication is skipped for m = None."""
    r = np.ascontiguousarray(r, dtype=np.float64)
    with np.errstate(all="ignore"):
        w = _solve(first, r)
        v = w if m is None else np.ascontiguousarray(m, dtype=np.float64) * w
        return _solve(second, np.ascontiguousarray(v)).copy()


def run(product, b, x0, first, m, second, max_steps, tol):
    """(steps, updates, reason, rr_each, rz_each, sigma_each, x): pcg_method.run with z = apply(first, m, second, r) in place of
    r / m, word for word."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    tol = np.float64(tol)
    with np.errstate(all="ignore"):
        bb = cg.dot(b, b)
        thr = (tol * tol) * bb
        if x0 is None:
            x, r = np.zeros(len(b)), b.copy()
        else:
            x = np.ascontiguousarray(x0, dtype=np.float64).copy()
            r = b - np.ascontiguousarray(product(x), dtype=np.float64)
        z = apply(first, m, second, r)
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
            z = apply(first, m, second, r)
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


# ---------------------------------------------------------------------------------------------------------------- the plans
def sgs(C):
    """(first, m, second) of symmetric Gauss-Seidel on the Case C itself: M = (D + L) D^-1 (D + U), the triangles of C as stored."""
    return (C, LOWER, STORED), pcg.diagonal_csr(C.n, C.n, *C.csr), (C, UPPER, STORED)


def diagonal_only(d):
    """(first, None, second) on a matrix that stores only the diagonal d: LOWER / STORED divides by d, UPPER / UNIT subtracts
    +0.0 -- every number of run() is then pcg_method.run's with m = d."""
    n = len(d)
    C = trsv.Case("diagonal_only(%d)" % n, n, np.arange(n), np.arange(n), np.asarray(d, dtype=np.float64))
    return (C, LOWER, STORED), None, (C, UPPER, UNIT)


# ---------------------------------------------------------------------------------------------------------------- the matrices
@functools.lru_cache(maxsize=None)
def lap2d(k):
    """The 5-point Laplacian on a k x k grid: 4 on the diagonal, -1 to the neighbours, n = k * k.  Its diagonal is constant, so
    Jacobi buys nothing on it."""
    i = np.arange(k * k)
    gx, gy = i % k, i // k
    rows, cols, vals = [i], [i], [np.full(k * k, 4.0)]
    for keep, off in ((gx > 0, -1), (gx < k - 1, 1), (gy > 0, -k), (gy < k - 1, k)):
        rows.append(i[keep])
        cols.append(i[keep] + off)
        vals.append(np.full(int(keep.sum()), -1.0))
    return pi.Matrix(k * k, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


def ic0(M):
    """(F, F^T) as trsv_method.Cases: a plain IC(0) of a small symmetric positive definite matrix, A ~ F F^T on the pattern of A's
    lower triangle; both Cases hold their rows' columns ascending.  Its values are only inputs to both sides of a comparison, so
    how they are rounded does not matter."""
    A = cg.dense(M)
    F = np.tril(A)
    pattern = F != 0.0
    n = M.n
    for k in range(n):
        F[k, k] = np.sqrt(F[k, k])
        below = np.flatnonzero(pattern[k + 1:, k]) + k + 1
        F[below, k] /= F[k, k]
        for j in below:
            rows = below[below >= j]
            rows = rows[pattern[rows, j]]
            F[rows, j] -= F[rows, k] * F[j, k]
    assert np.isfinite(F).all() and (np.diag(F) > 0.0).all(), "IC(0) broke down"
    r, c = np.nonzero(pattern)                                                       # row-major: every row's columns ascending
    lower = trsv.Case("ic0 factor", n, r, c, F[r, c])
    order = np.lexsort((r, c))                                                       # F^T: by column of F, then by row
    upper = trsv.Case("ic0 factor, transposed", n, c[order], r[order], F[r, c][order])
    return lower, upper


# ------------------------------------------------------------------------------------------------------------ the stop rules
def zero_diagonal(M, row):
    """M's CSR arrays as a Case with the stored diagonal of `row` replaced by 0.0: a LOWER / STORED solve divides by zero there."""
    C = trsv.of_matrix("%d x %d with a zero stored at (%d, %d)" % (M.n, M.n, row, row), M)
    r, c, v = C.entries()
    v = v.copy()
    v[(r == row) & (c == row)] = 0.0
    return trsv.Case(C.name, M.n, r, c, v, finite_stored=False)


def stop_cases():
    """(name, the product's matrix, b, (first, m, second), tol, (steps, updates, reason)) for max_steps = 10."""
    A = cg.spd(300)
    C = trsv.of_matrix("spd(300)", A)
    first, m, second = sgs(C)
    ident = diagonal_only(np.ones(300))
    b = cg.rhs(300)
    yield "a zero stored diagonal in first's triangle", A, b, ((zero_diagonal(A, 17), LOWER, STORED), m, second), 1e-10, (0, 0, NONFINITE)
    yield "m = -diag", A, b, (first, -m, second), 1e-10, (0, 0, BREAKDOWN)
    yield "minus_identity, identity plans", cg.minus_identity(300), cg.rhs(300, 5), ident, 1e-10, (1, 0, BREAKDOWN)
    yield "max_steps", A, b, (first, m, second), 1e-300, (10, 10, MAX_STEPS)
    yield "zero b", A, np.zeros(300), (first, m, second), 1e-10, (0, 0, CONVERGED)
    yield "zero b, tol 0", A, np.zeros(300), (first, m, second), 0.0, (0, 0, CONVERGED)
    yield "a NaN matrix value", cg.nan_value(), b, (first, m, second), 1e-10, (1, 0, NONFINITE)
    inf = cg.rhs(300)
    inf[17] = np.inf
    yield "inf in b", A, inf, (first, m, second), 1e-10, (0, 0, NONFINITE)
    yield "bb overflows", A, np.full(300, 1e200), (first, m, second), 1e-10, (0, 0, NONFINITE)
