"""LSQR as include/smvp_amd.h defines it (smvp_csr_lsqr / smvp_tjds_lsqr, kernel K22) restated in numpy, word for word: the run on
unnormalised bidiagonalisation vectors with its rules, around cg_method.py's order-defined dot.  Plain functions, no fixtures:
test_lsqr_host.py pins them to hand-computed runs and to numpy.linalg.lstsq on the CPU, test_gpu_lsqr.py compares the library's bits
with them.

Why bits.  As for every solver before it: the header fixes the order of every addition of the dot, sqrt is the correctly rounded
root (numpy's is), everything else is one correctly rounded IEEE operation per element or scalar, and the only inputs that are the
library's own are the two products, which run() takes as functions -- on the GPU the same handles' single products.  There is no
check_every in run(), because nothing depends on it.

The matrices are Rect objects: M x N, which no other solver's construction is."""
import numpy as np

import oracle_binding as ob
import smvp_toolkit_amd as sm
import transposed as tr
from cg_method import dot, rhs, TRIP  # noqa: F401

CONVERGED, LEAST_SQUARES, MAX_STEPS, NONFINITE = 0, 1, 2, 3   # SMVP_LSQR_*


# ------------------------------------------------------------------------------------------------------------------- the run
def _norm_after(scaling, dd):
    """The root of a dot, or +0.0 where the vector was not formed (its scaling was zero or not finite)."""
    return np.sqrt(dd) if np.isfinite(scaling) and scaling != 0.0 else np.float64(0.0)


def run(product, product_t, b, x0, max_steps, tol, atol):
    """(steps, updates, reason, rnorm_each, arnorm_each, x, (rnorm, arnorm, anorm, bnorm)): the run as the header defines it.
    product: N elements in, M out; product_t: M in, N out; numpy both ways.  Every array expression below is an array of its own:
    each quotient and product is rounded before the difference or sum that uses it."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    tol, atol = np.float64(tol), np.float64(atol)

    def mul(y):
        return np.ascontiguousarray(product(y), dtype=np.float64)

    def mul_t(y):
        return np.ascontiguousarray(product_t(y), dtype=np.float64)

    with np.errstate(all="ignore"):
        bnorm = np.sqrt(dot(b, b))
        thr = tol * bnorm
        uh = b.copy() if x0 is None else b - mul(np.ascontiguousarray(x0, dtype=np.float64))
        beta = np.sqrt(dot(uh, uh))
        p = mul_t(uh)
        x = np.zeros(len(p)) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        can = bool(np.isfinite(beta) and beta != 0.0)
        vh = p / beta if can else np.zeros(len(p))
        alpha = _norm_after(beta, dot(vh, vh))
        phibar, rhobar = beta, alpha
        a2 = alpha * alpha
        anorm, rnorm, arnorm = np.sqrt(a2), beta, beta * alpha
        rns, arns = [rnorm], [arnorm]

        def end(steps, updates, reason):
            return steps, updates, reason, np.array(rns), np.array(arns), x, (rnorm, arnorm, anorm, bnorm)

        if not all(np.isfinite(v) for v in (bnorm, beta, alpha, anorm, arnorm)):
            return end(0, 0, NONFINITE)
        if beta <= thr:
            return end(0, 0, CONVERGED)
        if alpha == 0.0:
            return end(0, 0, LEAST_SQUARES)
        w = vh / alpha
        k = 0
        while True:
            k += 1
            q = mul(vh)
            uh = (q / alpha) - (alpha * (uh / beta))
            beta_next = np.sqrt(dot(uh, uh))
            p = mul_t(uh)
            if np.isfinite(beta_next) and beta_next != 0.0:
                vh = (p / beta_next) - (beta_next * (vh / alpha))
                alpha_next = np.sqrt(dot(vh, vh))
            else:
                alpha_next = np.float64(0.0)                                           # vh_{k+1} is not formed
            rho = np.sqrt((rhobar * rhobar) + (beta_next * beta_next))
            c, s = rhobar / rho, beta_next / rho
            theta = s * alpha_next
            rhobar_next = -(c * alpha_next)
            phi, phibar_next = c * phibar, s * phibar
            tx, tw = phi / rho, theta / rho
            a2_next = (a2 + (beta_next * beta_next)) + (alpha_next * alpha_next)
            anorm_next = np.sqrt(a2_next)
            ac = alpha_next * np.abs(c)
            arnorm_next = phibar_next * ac
            if not all(np.isfinite(v) for v in (beta_next, alpha_next, rho, tx, tw, anorm_next, phibar_next, arnorm_next)):
                return end(k, k - 1, NONFINITE)                                        # rule N: nothing of the step is applied
            x = x + (tx * w)
            alpha, beta, phibar, rhobar, a2 = alpha_next, beta_next, phibar_next, rhobar_next, a2_next
            rnorm, arnorm, anorm = phibar_next, arnorm_next, anorm_next
            rns.append(rnorm)
            arns.append(arnorm)
            if rnorm <= thr:                                                          # rule S, the first that holds
                return end(k, k, CONVERGED)
            if ac <= atol * anorm:
                return end(k, k, LEAST_SQUARES)
            if k == max_steps:
                return end(k, k, MAX_STEPS)
            w = (vh / alpha) - (tw * w)


# ---------------------------------------------------------------------------------------------------------------- the matrices
class Rect:
    """An m x n matrix: its entries in storage order (coo), the host converter's CSR arrays of them, and both host products."""

    def __init__(self, m, n, rows, cols, vals):
        self.m, self.n = int(m), int(n)
        self.coo = sm.make_coo(rows, cols, vals)
        self.row_ptr, self.col_ind, self.val = sm.csr_from_coo(self.coo, self.m)
        self.nnz = len(self.coo)

    @property
    def csr(self):
        return self.row_ptr, self.col_ind, self.val

    def spmv(self, x):
        """A x by the oracle's serial loop."""
        return ob.csr_spmv(self.row_ptr, self.col_ind, self.val, x) if self.m else np.zeros(0)

    def spmv_t(self, x):
        """A^T x by the transposed product's reference."""
        return tr.reference(self.coo, self.m, self.n, x)

    def dense(self):
        A = np.zeros((self.m, self.n))
        np.add.at(A, (np.array(self.coo["row"]), np.array(self.coo["col"])), np.array(self.coo["val"]))
        return A

    def transpose(self):
        return Rect(self.n, self.m, self.coo["col"], self.coo["row"], self.coo["val"])


def of(M):
    """A square power_iteration.Matrix as a Rect."""
    return Rect(M.n, M.n, M.coo["row"], M.coo["col"], M.coo["val"])


def _sparse_block(rng, m, n, per_row, size):
    """m rows of 0 .. per_row entries at random columns, values in [-size, size]."""
    lens = rng.integers(0, per_row + 1, m)
    rows = np.repeat(np.arange(m), lens)
    return rows, rng.integers(0, n, len(rows)), rng.uniform(-size, size, len(rows))


def tall(m, n, seed=20300, per_row=3, size=0.05):
    """m x n, m >= n: a diagonal block with entries in [1, 2] stacked on an (m - n) x n sparse random block of small entries:
    well conditioned (the singular values stay near the diagonal's)."""
    assert m >= n
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 2.0, n)
    rows, cols, vals = _sparse_block(rng, m - n, n, per_row, size)
    i = np.arange(n)
    return Rect(m, n, np.concatenate([i, rows + n]), np.concatenate([i, cols]), np.concatenate([d, vals]))


def wide(m, n, seed=20301, per_row=3, size=0.05):
    """m x n, m <= n: a diagonal block with entries in [1, 2] beside an m x (n - m) sparse random block of small entries."""
    assert m <= n
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 2.0, m)
    rows, cols, vals = _sparse_block(rng, m, n - m, per_row, size)
    i = np.arange(m)
    return Rect(m, n, np.concatenate([i, rows]), np.concatenate([i, cols + m]), np.concatenate([d, vals]))


def rank_deficient(m, n, seed=20302):
    """tall(m, n) with column n - 1 replaced by a copy of column 0: rank n - 1."""
    T = tall(m, n, seed)
    rows, cols, vals = (np.array(T.coo[f]) for f in ("row", "col", "val"))
    keep = cols != n - 1
    first = cols == 0
    return Rect(m, n, np.concatenate([rows[keep], rows[first]]), np.concatenate([cols[keep], np.full(first.sum(), n - 1)]),
                np.concatenate([vals[keep], vals[first]]))


def dense_rect(a):
    """A small matrix from its rows, the entries that are not zero stored."""
    a = np.array(a, dtype=np.float64)
    i, j = np.nonzero(a)
    return Rect(a.shape[0], a.shape[1], i, j, a[i, j])


NAMED = ("tall(257, 131), inconsistent", "tall(257, 131), consistent", "wide(131, 257)", "nonsym(257)")


def named(name):
    """(A, b) of the constructions the step counts are pinned on: an inconsistent b is rhs(m); the consistent one is A x* for
    x* = rhs(n, 5) by the host product; wide and nonsym have full row rank, so every b is consistent."""
    import bicgstab_method as bi
    if name.startswith("tall"):
        A = tall(257, 131)
        return A, rhs(257) if name.endswith("inconsistent") else A.spmv(rhs(131, 5))
    if name.startswith("wide"):
        return wide(131, 257), rhs(131)
    return of(bi.nonsym(257)), rhs(257)
