"""Right-preconditioned restarted GMRES (include/smvp_amd.h: smvp_csr_gmres / smvp_tjds_gmres, kernel K19) restated in numpy, on
cg_method.py's dot and pbicgstab_method.py's application of M.  Plain functions, no fixtures: test_gmres_host.py pins them to
hand-computed runs and to the true residual on the CPU, test_gpu_gmres.py compares the library's bits with them.

Why bits.  The dot's order is the header's; z = M^-1 y is K18's; the two roots are the correctly rounded IEEE root (numpy.sqrt);
everything else is one correctly rounded IEEE operation, on an element or on a scalar, and the Gram-Schmidt passes, the rotations
and the back-substitution run in the order the header writes them down.  The only input that is the library's own is the product,
so run() takes it as a function.  There is no check_every in run(), because nothing depends on it."""
import numpy as np

import pbicgstab_method as pb
from cg_method import dot

CONVERGED, MAX_STEPS, BREAKDOWN, NONFINITE = 0, 1, 2, 3      # SMVP_GMRES_*


def run_rr(product, b, x0, first, m, second, restart, max_steps, tol, trace=None):
    """run()'s tuple and, behind it, the result block's rr: rr_steps, or tr_c where a start rule ended the run or rule S1 fired in a
    cycle's first step (the squared norm that belongs to x as it stands)."""
    b = np.ascontiguousarray(b, dtype=np.float64)
    tol = np.float64(tol)
    plain = first is None and m is None and second is None
    assert 1 <= restart <= 64 and max_steps >= 1

    def mul(y):
        return np.ascontiguousarray(product(y), dtype=np.float64)

    def minv(y):
        return y if plain else pb.apply(first, m, second, y)

    with np.errstate(all="ignore"):
        bb = dot(b, b)
        thr = (tol * tol) * bb
        x = np.zeros(len(b)) if x0 is None else np.ascontiguousarray(x0, dtype=np.float64).copy()
        rrs, trs = [], []
        k, c = 0, 0
        while True:
            r = b.copy() if c == 0 and x0 is None else b - mul(x)
            tr = dot(r, r)
            trs.append(tr)
            if c == 0:
                rrs.append(tr)
            c += 1
            rr = tr

            def end(columns, reason):
                return k, c, columns, reason, np.array(rrs), np.array(trs), x, rr

            if not (np.isfinite(bb) and np.isfinite(tr)):                            # the start rule
                return end(0, NONFINITE)
            if tr <= thr:
                return end(0, CONVERGED)
            beta = np.sqrt(tr)
            V = [r / beta]
            gbar = beta
            g, cs, sn = [], [], []
            R = np.zeros((restart, restart))

            def update(cols):
                if cols == 0:
                    return x
                y = np.zeros(cols)
                for i in range(cols - 1, -1, -1):
                    acc = g[i]
                    for l in range(i + 1, cols):
                        acc = acc - (R[i, l] * y[l])
                    y[i] = acc / R[i, i]
                u = y[0] * V[0]
                for i in range(1, cols):
                    u = u + (y[i] * V[i])
                return x + minv(u)

            def basis():
                if trace is not None:
                    trace.append(np.array(V))

            for j in range(1, restart + 1):
                k += 1
                w = mul(minv(V[j - 1]))
                h = [dot(V[i], w) for i in range(j)]
                for i in range(j):
                    w = w - (h[i] * V[i])
                q = [dot(V[i], w) for i in range(j)]
                for i in range(j):
                    w = w - (q[i] * V[i])
                h = [h[i] + q[i] for i in range(j)]
                h.append(np.sqrt(dot(w, w)))
                raw = list(h)
                for i in range(j - 1):
                    t = (cs[i] * h[i]) + (sn[i] * h[i + 1])
                    h[i + 1] = (cs[i] * h[i + 1]) - (sn[i] * h[i])
                    h[i] = t
                d = np.sqrt((h[j - 1] * h[j - 1]) + (h[j] * h[j]))
                if not (np.isfinite(raw).all() and np.isfinite(d)) or d == 0.0:      # rule S1
                    x = update(j - 1)
                    basis()
                    return end(j - 1, BREAKDOWN if np.isfinite(raw).all() and np.isfinite(d) else NONFINITE)
                cs.append(h[j - 1] / d)
                sn.append(h[j] / d)
                R[:j - 1, j - 1] = h[:j - 1]
                R[j - 1, j - 1] = d
                gnext = -(sn[-1] * gbar)
                g.append(cs[-1] * gbar)
                gbar = gnext
                rr = gnext * gnext
                rrs.append(rr)
                if rr <= thr or k == max_steps:                                      # rule S2, the first that holds
                    x = update(j)
                    basis()
                    return end(j, CONVERGED if rr <= thr else MAX_STEPS)
                V.append(w / h[j])
            x = update(restart)
            basis()


def run(product, b, x0, first, m, second, restart, max_steps, tol, trace=None):
    """(steps, cycles, columns, reason, rr_each, restart_each, x): the run as the header defines it.  product: numpy in, numpy out.
    Every array expression is an array of its own: each product is rounded before the difference or the sum that uses it.  trace: a
    list that receives, at the end of every cycle, the basis vectors the cycle formed as the rows of one array."""
    return run_rr(product, b, x0, first, m, second, restart, max_steps, tol, trace)[:7]


def host_product(M):
    """The host CSR loop of a power_iteration.Matrix."""
    return M.spmv
