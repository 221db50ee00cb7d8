#!/usr/bin/env python3
"""K22 measured: a step of LSQR (smvp_csr_lsqr with ht = transposed(), smvp_tjds_lsqr with K8) against its expectation and against
the loop a caller composes today.

  python tools/exp_lsqr.py [--case large|small|both] [--routes csr,tjds] [--runs R]

Per case and route, in one process: the forward and the transposed product alone (median of R event timings), the expectation of a
step -- the two products as just measured + the passes over a vector at the copy bandwidth of profiles/r01_copy_bandwidth.txt --, a
step of the library (two calls at tol = atol = 0 with max_steps = S1 and S2 and one look at the end; their difference over
S2 - S1: the work space, step 0 and the history copies cancel), and a step of the composed loop: LSQR with normalised vectors
from the handle's spmv, the transposed product, torch.linalg.vector_norm (one host read per scalar, which the divisions need) and
torch.add / mul.  Prints met or missed per cell: met means within MARGIN of the expectation.

The cases: `large` is a tall construction of 16 777 216 x 4 194 304 (a diagonal block over two small entries a row: 29.4 M entries),
`small` is lsqr_method.tall(1003, 517), where launches decide."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "smvp-toolkit_amd", "python"), os.path.join(ROOT, "tests")]

COPY_BYTES_PER_S = 5.2e12                                    # profiles/r01_copy_bandwidth.txt
PASSES_M, PASSES_N = 3, 8                                    # pass U's uh half; pass V and pass U's x / w half
MARGIN = 1.15                                                # what the vector passes of profiles/krylov_refactor_measured.txt keep to
S1, S2 = 10, 30


def tall_csr(m, n, seed=20300):
    """A tall matrix as CSR arrays, built without the COO detour: row i < n holds (i, i) in [1, 2]; row i >= n holds two entries in
    +-0.05 at random columns, ascending."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.ones(n, np.int64), np.full(m - n, 2, np.int64)])
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    low = np.sort(rng.integers(0, n, (m - n, 2), dtype=np.int32), axis=1)
    col = np.concatenate([np.arange(n, dtype=np.int32), low.ravel()])
    val = np.concatenate([rng.uniform(1.0, 2.0, n), rng.uniform(-0.05, 0.05, 2 * (m - n))])
    return row_ptr, col, val


def timed(torch, fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), (max(out) - min(out)) / float(np.median(out))


def composed_step(torch, forward, trans, st):
    """One step of textbook LSQR on normalised u, v with host scalars: what a caller writes today."""
    u, v, w, x = st["u"], st["v"], st["w"], st["x"]
    q = forward(v)
    u = torch.add(q, u, alpha=-st["alpha"])
    beta = float(torch.linalg.vector_norm(u))
    u = u / beta
    p = trans(u)
    v = torch.add(p, v, alpha=-beta)
    alpha = float(torch.linalg.vector_norm(v))
    v = v / alpha
    rho = (st["rhobar"] ** 2 + beta ** 2) ** 0.5
    c, s = st["rhobar"] / rho, beta / rho
    theta, phi = s * alpha, c * st["phibar"]
    x = torch.add(x, w, alpha=phi / rho)
    w = torch.add(v, w, alpha=-theta / rho)
    st.update(u=u, v=v, w=w, x=x, alpha=alpha, rhobar=-c * alpha, phibar=s * st["phibar"])


def composed(torch, forward, trans, b, steps):
    beta = float(torch.linalg.vector_norm(b))
    u = b / beta
    v = trans(u)
    alpha = float(torch.linalg.vector_norm(v))
    v = v / alpha
    st = dict(u=u, v=v, w=v.clone(), x=torch.zeros_like(v), alpha=alpha, rhobar=alpha, phibar=beta)
    for _ in range(steps):
        composed_step(torch, forward, trans, st)
    return st["x"]


def measure(torch, sm, name, m, n, route, H, HT, runs):
    b = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, m)).cuda()
    xin = torch.from_numpy(np.random.default_rng(2).uniform(-1.0, 1.0, n)).cuda()
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    ym, yn = torch.empty(m, dtype=torch.float64, device="cuda"), torch.empty(n, dtype=torch.float64, device="cuda")
    if route == "csr":
        def forward(v, out=None):
            out = torch.empty(m, dtype=torch.float64, device="cuda") if out is None else out
            H.spmv(v, out)
            return out

        def trans(u, out=None):
            out = torch.empty(n, dtype=torch.float64, device="cuda") if out is None else out
            HT.spmv(u, out)
            return out

        def solve(steps):
            return H.lsqr(b, x, at=HT, max_steps=steps, tol=0.0, atol=0.0, check_every=steps)
    else:
        def forward(v, out=None):
            out = torch.empty(m, dtype=torch.float64, device="cuda") if out is None else out
            H.set_x(v)
            H.spmv(out)
            return out

        def trans(u, out=None):
            out = torch.empty(n, dtype=torch.float64, device="cuda") if out is None else out
            H.spmv_transposed(u, out)
            return out

        def solve(steps):
            return H.lsqr(b, x, max_steps=steps, tol=0.0, atol=0.0, check_every=steps)

    for fn in (lambda: forward(xin, ym), lambda: trans(b, yn), lambda: solve(S1)):     # warm-up: plans, code objects
        fn()
    fwd, fs = timed(torch, lambda: forward(xin, ym), runs)
    tra, ts = timed(torch, lambda: trans(b, yn), runs)
    vec_ms = (PASSES_M * 8.0 * m + PASSES_N * 8.0 * n) / COPY_BYTES_PER_S * 1e3
    expect = fwd + tra + vec_ms
    t1, _ = timed(torch, lambda: solve(S1), runs)
    t2, sp = timed(torch, lambda: solve(S2), runs)
    r = solve(S2)[0]
    assert (r.steps, r.updates, r.reason) == (S2, S2, sm.LSQR_MAX_STEPS), (r.steps, r.updates, r.reason)
    step = (t2 - t1) / (S2 - S1)
    c1, _ = timed(torch, lambda: composed(torch, forward, trans, b, S1), runs)
    c2, cs = timed(torch, lambda: composed(torch, forward, trans, b, S2), runs)
    cstep = (c2 - c1) / (S2 - S1)
    xc = composed(torch, forward, trans, b, S2)
    apart = float(torch.linalg.vector_norm(xc - x) / torch.linalg.vector_norm(x))
    print("%s, %s: forward %.4f ms (spread %.1f %%), transposed %.4f ms (spread %.1f %%), %d + %d vector passes %.4f ms"
          % (name, route, fwd, 100 * fs, tra, 100 * ts, PASSES_M, PASSES_N, vec_ms))
    print("%s, %s: expectation %.4f ms a step; library %.4f ms a step (calls of %d and %d steps: %.3f and %.3f ms, spread %.1f %%): "
          "%.2f x the expectation: %s" % (name, route, expect, step, S1, S2, t1, t2, 100 * sp, step / expect,
                                          "met" if step <= MARGIN * expect else "missed"))
    print("%s, %s: composed loop %.4f ms a step (%.3f and %.3f ms, spread %.1f %%): the library's step is %.2f x faster; "
          "|x_composed - x| / |x| = %.2e after %d steps" % (name, route, cstep, c1, c2, 100 * cs, cstep / step, apart, S2))
    return fwd, tra, step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="both", choices=["large", "small", "both"])
    ap.add_argument("--routes", default="csr,tjds")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--m", type=int, default=16 * 1024 * 1024)
    ap.add_argument("--n", type=int, default=4 * 1024 * 1024)
    args = ap.parse_args()
    import torch

    import lsqr_method as lm
    import smvp_toolkit_amd as sm

    print("# device %s" % torch.cuda.get_device_name(0))
    cases = []
    if args.case in ("small", "both"):
        A = lm.tall(1003, 517)
        cases.append(("tall(1003, 517)", 1003, 517, A.csr))
    if args.case in ("large", "both"):
        cases.append(("tall(%d, %d)" % (args.m, args.n), args.m, args.n, tall_csr(args.m, args.n)))
    for name, m, n, csr in cases:
        steps = {}
        for route in args.routes.split(","):
            if route == "csr":
                H = sm.CsrMatrix(m, n, *csr)
                HT = H.transposed()
                print("# %s: nnz %d; h on %s, ht on %s" % (name, H.nnz, H.describe()[0][:60], HT.describe()[0][:60]))
            else:
                coo = sm.make_coo(np.repeat(np.arange(m), np.diff(csr[0])), csr[1], csr[2])
                H, HT = sm.TjdsMatrix(sm.tjds_from_coo(coo, m, n)), None
                del coo
                print("# %s: TJDS forward %s, transposed %s" % (name, H.describe()[0][:60], H.transposed_describe()[0][:60]))
            steps[route] = measure(torch, sm, name, m, n, route, H, HT, args.runs)
            for X in (HT, H):
                if X is not None:
                    X.close()
        if len(steps) == 2:
            (cf, ct, cs), (tf, tt, ts) = steps["csr"], steps["tjds"]
            print("%s: K8 against the transposed handle %.2f x; a TJDS step against a CSR step %.2f x (%.4f against %.4f ms)"
                  % (name, tt / ct, ts / cs, ts, cs))


if __name__ == "__main__":
    main()
