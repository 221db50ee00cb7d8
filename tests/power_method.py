"""The scaled power method of include/smvp_amd.h (smvp_csr_power_method / smvp_tjds_power_method) restated in numpy: absmax, one
step, the run with its looked steps and stop rules.  Plain functions, no fixtures: test_power_method_host.py pins them to the
oracle's iteration and to known answers on the CPU, test_gpu_power_method.py compares the library's bits with them.

Why bits.  Every number of the definition is a maximum, an element picked by index or one correctly rounded IEEE operation: it has
one right answer, numpy's, whatever order the device reduces in.  The only input that is the library's own is the product, so
run() takes it as a function -- on the GPU the same handle's single product.

Matrices and start vectors are power_iteration.py's; sym() is the one matrix added here."""
import numpy as np

import power_iteration as pi

CONVERGED, MAX_STEPS, ZERO, NONFINITE = 0, 1, 2, 3      # SMVP_POWER_*
REDUCE_TRIP = 2048 * 256                                # elements of one grid trip of the reduce pass (kPowerGridCap * kPowerBlock)
SYM_STEPS = 40                                          # sym() converges at tol 1e-9 inside these (test_power_method_host.py)


def absmax(v):
    """(m, p): m the largest |v_r| over the r whose v_r is not NaN (0.0 without any), p the smallest such r with |v_r| == m (-1)."""
    a = np.abs(np.ascontiguousarray(v, dtype=np.float64))
    ok = ~np.isnan(a)
    if not ok.any():
        return np.float64(0.0), -1
    m = a[ok].max()
    return np.float64(m), int(np.flatnonzero(ok & (a == m))[0])


def step(product, x, p):
    """One step from the operand x whose absmax index is p: (y, lambda, res, m, p_next, x_next)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(product(x), dtype=np.float64)
    with np.errstate(all="ignore"):
        lam = y[p] / x[p] if p >= 0 else np.float64(np.nan)       # numpy scalars: 0 / 0 is NaN, not an exception
        d = np.abs(y - lam * x)                                   # the product is an array of its own: rounded before the difference
    d = d[~np.isnan(d)]
    res = d.max() if d.size else np.float64(0.0)
    m, p_next = absmax(y)
    with np.errstate(all="ignore"):
        x_next = y / m if m > 0.0 else y.copy()
    return y, np.float64(lam), np.float64(res), m, p_next, x_next


def run(product, x0, max_steps, tol=0.0, check_every=1):
    """(steps, reason, index, lambda_each, residual_each, scale, x): the run as the header defines it.  product: numpy in, numpy
    out."""
    x = np.ascontiguousarray(x0, dtype=np.float64).copy()
    tol = np.float64(tol)
    _, p = absmax(x)
    lams, ress = [], []
    k = 0
    while True:
        k += 1
        y, lam, res, m, p_next, x_next = step(product, x, p)
        lams.append(lam)
        ress.append(res)
        reason = None
        if k % check_every == 0 or k == max_steps:
            with np.errstate(all="ignore"):
                bound = (tol * np.abs(lam)) * (np.abs(x[p]) if p >= 0 else np.float64(np.nan))
            if not np.isfinite(lam):
                reason = NONFINITE
            elif not m > 0.0:
                reason = ZERO
            elif res <= bound:
                reason = CONVERGED
            elif k == max_steps:
                reason = MAX_STEPS
        if reason is not None:
            return k, reason, p, np.array(lams), np.array(ress), m, x_next
        x, p = x_next, p_next


# ---------------------------------------------------------------------------------------------------------------- the matrices
def sym(dense=False):
    """n = 1003, B + B^T plus a diagonal, seeded: B has 0 to 4 entries per row in [-0.1, 0.1], the diagonal lies in [-1, 1] except
    one entry of 6 -- the dominant eigenvalue is real and simple (Gershgorin: alone beyond 5, everything else inside [-2, 2]) and
    its vector is no unit vector, so that lambda itself converges gradually, at a ratio below 0.4 a step.  dense: the array too."""
    rng = np.random.default_rng(20260)
    n, q = 1003, 417
    lens = rng.integers(0, 5, n)
    rows = np.repeat(np.arange(n), lens)
    cols = rng.integers(0, n, len(rows))
    keep = rows != cols
    rows, cols = rows[keep], cols[keep]
    vals = rng.uniform(-0.1, 0.1, len(rows))
    diag = rng.uniform(-1.0, 1.0, n)
    diag[q] = 6.0
    r = np.concatenate([rows, cols, np.arange(n)])
    c = np.concatenate([cols, rows, np.arange(n)])
    v = np.concatenate([vals, vals, diag])
    M = pi.Matrix(n, r, c, v)
    if not dense:
        return M
    A = np.zeros((n, n))
    np.add.at(A, (r, c), v)
    return M, A


def diagonal(n, entries):
    """A diagonal matrix of ones with the given {index: value} entries in their places."""
    d = np.ones(n)
    for i, v in entries.items():
        d[i] = v
    return pi.Matrix(n, np.arange(n), np.arange(n), d)


def edge(n):
    """n rows of 1 to min(3, n) entries with sum |val| <= 1.5, except the last row, whose only entry is (n - 1, n - 1) = -3: the
    largest magnitude of every iterate from ones is at the last element alone (the tail of a wavefront, of a workgroup)."""
    rng = np.random.default_rng(20261 + n)
    lens = rng.integers(1, min(3, n) + 1, n)
    lens[n - 1] = 0
    rows, cols = pi._entries(rng, n, lens)
    vals = rng.uniform(-0.5, 0.5, len(rows))
    return pi.Matrix(n, np.append(rows, n - 1), np.append(cols, n - 1), np.append(vals, -3.0))


TIE_AT = (5, 69, 261, 1000)                            # two lanes apart, two waves apart, two workgroups apart


def tie_case(sign_first=-1.0):
    """(matrix, x0): a diagonal matrix of n = 1003 with entries of magnitude 2 and mixed sign at TIE_AT (0.5 elsewhere), and a start
    vector of magnitude 1 with mixed sign there (0.25 elsewhere): every iterate has its largest magnitude, equal to the bit, at all
    four indices, and the smallest of them must be named."""
    signs = (sign_first, 1.0, -1.0, 1.0)
    d = {i: 0.5 for i in range(1003)}
    d.update({i: 2.0 * s for i, s in zip(TIE_AT, signs)})
    x = np.full(1003, 0.25)
    x[list(TIE_AT)] = (1.0, -1.0, -1.0, 1.0)
    return diagonal(1003, d), x
