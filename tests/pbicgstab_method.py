"""Right-preconditioned BiCGSTAB (include/smvp_amd.h: smvp_csr_pbicgstab / smvp_tjds_pbicgstab, kernel K18) restated in numpy, on
cg_method.py's dot and trsv_method.py's serial substitution.  Plain functions, no fixtures: test_pbicgstab_host.py pins them to
bicgstab_method.run, to exact cases and to the true residual on the CPU, test_gpu_pbicgstab.py compares the library's bits with them.

Why bits.  yhat = M^-1 y is up to two of K15's solves -- each element the serial substitution loop's -- and at most one rounded
multiplication between them; the dot's order is the header's; everything else is one correctly rounded IEEE operation per element,
and the rules are K13's in K13's order.  The only input that is the library's own is the product, so run() takes it as a function,
as bicgstab_method.run does.  A plan is a (trsv_method.Case, uplo, diag) triple or None; m is an array or None."""
import functools

import numpy as np

import bicgstab_method as bi
import ilu0_method as ilu
import pcg_method as pcg
import pcg_tri_method as tri
import power_iteration as pi
import trsv_method as trsv

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = bi.CONVERGED, bi.MAX_STEPS, bi.BREAKDOWN, bi.NONFINITE
LOWER, UPPER, STORED, UNIT = trsv.LOWER, trsv.UPPER, trsv.STORED, trsv.UNIT
dot = bi.dot


def apply(first, m, second, y):
    """yhat = T2^-1 (m .* (T1^-1 y)), every part optional: a solve is skipped for a plan that is None, the multiplication for
    m = None.  Always an array of its own."""
    w = np.ascontiguousarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        if first is not None:
            w = tri._solve(first, w)
        if m is not None:
            w = np.ascontiguousarray(m, dtype=np.float64) * w
        if second is not None:
            w = tri._solve(second, np.ascontiguousarray(w))
        return np.array(w, dtype=np.float64)


def run(product, b, x0, first, m, second, max_steps, tol):
    """(steps, full, half, reason, rr_each, ss_each, x): bicgstab_method.run with phat = apply(p) and shat = apply(s), word for
    word.  Every array expression below is an array of its own: each product is rounded before the sum that uses it."""
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

        def end(steps, full, half, reason):
            return steps, full, half, reason, np.array(rrs), np.array(sss), x

        if not (np.isfinite(bb) and np.isfinite(rho)):
            return end(0, 0, 0, NONFINITE)
        if rho <= thr:
            return end(0, 0, 0, CONVERGED)
        k = 0
        while True:
            k += 1
            phat = apply(first, m, second, p)
            v = mul(phat)
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
                x = x + alpha * phat
                return end(k, k - 1, 1, CONVERGED)
            shat = apply(first, m, second, s)
            t = mul(shat)
            ts, tt = dot(t, s), dot(t, t)
            if not (np.isfinite(ts) and np.isfinite(tt)):                            # rule T
                return end(k, k - 1, 0, NONFINITE)
            if not tt > 0.0:
                x = x + alpha * phat
                return end(k, k - 1, 1, BREAKDOWN)
            omega = ts / tt
            x = (x + alpha * phat) + omega * shat
            r = s - omega * t
            rr, rho_new = dot(r, r), dot(rhat, r)
            rrs.append(rr)
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


# ---------------------------------------------------------------------------------------------------------- the preconditioners
def plain():
    return None, None, None


def identity_plans(n):
    """(first, None, second) on a matrix that stores only a unit diagonal: LOWER / STORED gives (y - (+0.0)) / 1.0, UPPER / UNIT
    subtracts +0.0 -- every number of run() is then bicgstab_method.run's."""
    return tri.diagonal_only(np.ones(n))


def jacobi(Cs):
    """(None, 1 ./ diagonal, None): the diagonal by smvp_csr_diagonal's rule, one rounded reciprocal per element."""
    return None, 1.0 / pcg.diagonal_csr(Cs.n, Cs.n, *Cs.csr), None


def sgs(Cs):
    """Symmetric Gauss-Seidel on the Case itself: M = (D + L) D^-1 (D + U)."""
    return tri.sgs(Cs)


def ilu0(Cs):
    """M = L U from the ILU(0) of the Case (ilu0_method.factor: computed once per Case)."""
    return ilu.plans(ilu.factor(Cs))


# ---------------------------------------------------------------------------------------------------------------- the matrices
@functools.lru_cache(maxsize=None)
def convdiff(k, c):
    """The 5-point convection-diffusion grid on k x k points: 4 on the diagonal, -1 - c to the west and south neighbours, -1 + c to
    the east and north ones; n = k * k, not symmetric for c != 0.  The host converter sorts every row, and every row stores its
    diagonal, so ilu0_method accepts its CSR arrays."""
    i = np.arange(k * k)
    gx, gy = i % k, i // k
    rows, cols, vals = [i], [i], [np.full(k * k, 4.0)]
    for keep, off, v in ((gx > 0, -1, -1.0 - c), (gx < k - 1, 1, -1.0 + c), (gy > 0, -k, -1.0 - c), (gy < k - 1, k, -1.0 + c)):
        rows.append(i[keep])
        cols.append(i[keep] + off)
        vals.append(np.full(int(keep.sum()), v))
    return pi.Matrix(k * k, np.concatenate(rows), np.concatenate(cols), np.concatenate(vals))


@functools.lru_cache(maxsize=None)
def case_of(name):
    """(the product's matrix, the Case the plans stand on) of a named system, built once and left unchanged.  '..., coalesced': the
    product's matrix is the coalesced Case's own (repeats added up, rows sorted), so ILU(0) accepts it; nonsym_shuffled's Case
    holds the entries AS STORED (unsorted columns, repeats)."""
    if name == "convdiff(32, 0.5)":
        M = convdiff(32, 0.5)
        return M, trsv.of_matrix(name, M)
    if name.endswith(", coalesced"):
        base = name[:-len(", coalesced")]
        fn, arg = base[:-1].split("(")
        Cs = ilu.of_matrix(base, getattr(bi, fn)(int(arg)))
        return ilu.as_matrix(Cs), Cs
    M = getattr(bi, name)()
    return M, trsv.of_matrix(name, M, as_stored=name == "nonsym_shuffled")


# ------------------------------------------------------------------------------------------------------------ the stop rules
def lower_integer():
    """(A, b, x): a 4 x 4 lower triangular integer matrix, b = A x for an integer x.  With first = LOWER / STORED on A itself M = A:
    phat = A^-1 r_0 = x exactly, v = r_0, sigma = rho_0, alpha = 1, s = 0 -- rule H at step 1 with the half update, x exact."""
    A = bi.dense3([[2, 0, 0, 0], [1, 1, 0, 0], [0, -2, 4, 0], [3, 0, 1, -1]])
    x = np.array([3.0, -1.0, 2.0, 5.0])
    return A, bi.dense(A) @ x, x


def nan_m(n, at=17):
    m = np.ones(n)
    m[at] = np.nan
    return m


def stop_cases():
    """(name, the product's matrix, b, (first, m, second), tol, (steps, full, half, reason), x or None) for max_steps = 10; x is
    what d_x must hold where the case fixes it."""
    A = bi.nonsym(300)
    Cs = trsv.of_matrix("nonsym(300)", A)
    b = bi.rhs(300)
    b5 = bi.rhs(300, 5)
    ident = identity_plans(300)
    first, m, second = sgs(Cs)
    L, b4, x4 = lower_integer()
    yield "M = A, lower triangular integers", L, b4, ((trsv.of_matrix("lower_integer", L), LOWER, STORED), None, None), 1e-10, \
        (1, 0, 1, CONVERGED), x4
    yield "identity, identity plans", bi.identity(300), b5, ident, 0.0, (1, 0, 1, CONVERGED), b5
    yield "swap2 (rule A), m of ones", bi.swap2(), np.array([1.0, 0.0]), (None, np.ones(2), None), 1e-10, (1, 0, 0, BREAKDOWN), np.zeros(2)
    yield "rule T, identity plans", bi.rule_t()[0], bi.rule_t()[1], identity_plans(3), 1e-10, (1, 0, 1, BREAKDOWN), np.array([-1.0, 0.0, 0.0])
    yield "rule B, identity plans", bi.rule_b()[0], bi.rule_b()[1], identity_plans(3), 1e-10, (1, 1, 0, BREAKDOWN), np.array([-0.5, -0.5, 0.0])
    yield "rule B, m of ones", bi.rule_b()[0], bi.rule_b()[1], (None, np.ones(3), None), 1e-10, (1, 1, 0, BREAKDOWN), np.array([-0.5, -0.5, 0.0])
    yield "a zero stored diagonal in first's triangle", A, b, ((tri.zero_diagonal(A, 17), LOWER, STORED), m, second), 1e-10, \
        (1, 0, 0, NONFINITE), np.zeros(300)
    yield "a zero stored diagonal in second's triangle", A, b, (first, m, (tri.zero_diagonal(A, 17), UPPER, STORED)), 1e-10, \
        (1, 0, 0, NONFINITE), np.zeros(300)
    yield "a NaN in m, no plans", A, b, (None, nan_m(300), None), 1e-10, (1, 0, 0, NONFINITE), np.zeros(300)
    yield "a NaN in m, between two plans", A, b, (first, nan_m(300), second), 1e-10, (1, 0, 0, NONFINITE), np.zeros(300)
    yield "a NaN matrix value", bi.nan_value(), b, jacobi(Cs), 1e-10, (1, 0, 0, NONFINITE), np.zeros(300)
    inf = bi.rhs(300)
    inf[17] = np.inf
    yield "inf in b", A, inf, (first, m, second), 1e-10, (0, 0, 0, NONFINITE), np.zeros(300)
    yield "bb overflows", A, np.full(300, 1e200), jacobi(Cs), 1e-10, (0, 0, 0, NONFINITE), np.zeros(300)
    yield "zero b", A, np.zeros(300), (first, m, second), 1e-10, (0, 0, 0, CONVERGED), np.zeros(300)
    yield "zero b, tol 0", A, np.zeros(300), jacobi(Cs), 0.0, (0, 0, 0, CONVERGED), np.zeros(300)
    yield "max_steps", A, b, jacobi(Cs), 1e-300, (10, 10, 0, MAX_STEPS), None
