"""Conjugate gradients for k right-hand sides (include/smvp_amd.h: smvp_csr_cg_multi / smvp_tjds_cg_multi, kernel K20) restated: the
header defines column v of every output as the one-vector run on column v of the operands, so the restatement IS cg_method.run
(m is None) or pcg_method.run per column, around a block product that is the oracle's serial loop per column -- the CSR row in
storage order, or the row's entries in ascending TJDS position.  Plain functions, no fixtures: test_cg_multi_host.py pins them on
the CPU, test_gpu_cg_multi.py compares the library's bits with them.

Unlike cg_method.run's product argument, which is the handle's own single product, the product here is never the library's: the
block products' bits are the serial loop's by contract (tests/test_gpu_spmm.py, tests/test_gpu_tjds_spmm.py), whatever the handle's
plan or mode."""
import functools

import numpy as np

import cg_method as cg
import oracle_binding as ob
import pcg_method as pcg
import power_iteration as pi
import smvp_toolkit_amd as sm

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = cg.CONVERGED, cg.MAX_STEPS, cg.BREAKDOWN, cg.NONFINITE


# ---------------------------------------------------------------------------------------------------------------- the products
def csr_product(M):
    """x -> A x by the oracle's serial CSR loop over a power_iteration.Matrix: column v of smvp_csr_spmm."""
    def product(x):
        with np.errstate(all="ignore"):
            return ob.csr_spmv(M.row_ptr, M.col_ind, M.val, np.ascontiguousarray(x, dtype=np.float64))
    return product


def tjds_product(M):
    """x -> A x by the oracle's serial TJDS loop over the host converter's arrays: column v of smvp_tjds_spmm."""
    t = sm.tjds_from_coo(M.coo, M.n, M.n)

    def product(x):
        with np.errstate(all="ignore"):
            return ob.tjds_spmv(t, np.ascontiguousarray(x, dtype=np.float64))
    return product


def product_of(M, fmt):
    return csr_product(M) if fmt == "csr" else tjds_product(M)


# --------------------------------------------------------------------------------------------------------------------- the run
def run_column(product, b, x0, m, max_steps, tol):
    """(steps, updates, reason, rr_each, rz_each, sigma_each, x) of one column: pcg_method.run's tuple; without an m it is
    cg_method.run's with rz_each = rr_each (the result block's rz is rr then)."""
    if m is not None:
        return pcg.run(product, b, x0, m, max_steps, tol)
    steps, updates, reason, rr, sigma, x = cg.run(product, b, x0, max_steps, tol)
    return steps, updates, reason, rr, rr, sigma, x


def run(product, B, X0, m, max_steps, tol):
    """The k runs of a block: a list of run_column's tuples, column by column.  B and X0 (or None) are (n, k)."""
    B = np.asarray(B, dtype=np.float64)
    assert B.ndim == 2 and (X0 is None or np.asarray(X0).shape == B.shape)
    return [run_column(product, B[:, v], None if X0 is None else np.asarray(X0)[:, v], m, max_steps, tol) for v in range(B.shape[1])]


def outcomes(runs):
    return [tuple(r[:3]) for r in runs]


def solution(runs):
    """(n, k): column v is run v's x."""
    return np.stack([r[6] for r in runs], axis=1)


def flat_histories(runs, max_steps, fill):
    """(rr_each, rz_each, sigma_each) as the C ABI lays them out: flat arrays of k * (max_steps + 1), k * (max_steps + 1) and
    k * max_steps doubles; column v's rr and rz at [v * (max_steps + 1) + j] for j = 0 .. updates_v, its sigma at [v * max_steps + j]
    for j = 0 .. steps_v - 1, and `fill` everywhere else."""
    k = len(runs)
    rr, rz, sigma = np.full(k * (max_steps + 1), fill), np.full(k * (max_steps + 1), fill), np.full(k * max_steps, fill)
    for v, (steps, updates, _, rrs, rzs, sigmas, _) in enumerate(runs):
        assert len(rrs) == len(rzs) == updates + 1 and len(sigmas) == steps
        rr[v * (max_steps + 1):v * (max_steps + 1) + updates + 1] = rrs
        rz[v * (max_steps + 1):v * (max_steps + 1) + updates + 1] = rzs
        sigma[v * max_steps:v * max_steps + steps] = sigmas
    return rr, rz, sigma


# ------------------------------------------------------------------------------------------- every way out, mixed in one block
MIXED_STEPS, MIXED_TOL = 3, 1e-10
MIXED_PLAIN = [(3, 3, MAX_STEPS), (1, 1, CONVERGED), (1, 0, BREAKDOWN), (0, 0, CONVERGED), (2, 1, BREAKDOWN), (0, 0, NONFINITE)]
MIXED_JACOBI = [(1, 1, CONVERGED), (1, 1, CONVERGED), (1, 0, BREAKDOWN), (0, 0, CONVERGED), (1, 0, BREAKDOWN), (0, 0, NONFINITE)]


def signed_diagonal_values(n=300):
    """d_i = 1 + i / 50 on the first half, -1 on the second."""
    i = np.arange(n)
    return np.where(i < n // 2, 1.0 + i / 50.0, -1.0)


@functools.lru_cache(maxsize=None)
def signed_diagonal(n=300):
    """diag(signed_diagonal_values(n)): positive definite on the first half of the indices, negative definite on the second."""
    return pi.Matrix(n, np.arange(n), np.arange(n), signed_diagonal_values(n))


def mixed_block(n=300):
    """Six right-hand sides for signed_diagonal(n) that end, at max_steps = MIXED_STEPS and tol = MIXED_TOL, in all four reasons
    (MIXED_PLAIN; with m = |d| MIXED_JACOBI): a vector on the positive half only, an eigenvector, a vector on the negative half
    only, zeros, a vector on both halves, a vector with a NaN."""
    rng = np.random.default_rng(5)
    h = n // 2
    B = np.zeros((n, 6))
    B[:h, 0] = rng.uniform(-1.0, 1.0, h)
    B[3, 1] = 1.5
    B[h:, 2] = rng.uniform(-1.0, 1.0, n - h)
    B[:, 4] = rng.uniform(-1.0, 1.0, n)
    B[:, 5] = rng.uniform(-1.0, 1.0, n)
    B[7, 5] = np.nan
    return B
