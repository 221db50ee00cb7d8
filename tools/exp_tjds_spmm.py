#!/usr/bin/env python3
"""Y = A X for a block of k vectors from a TJDS handle (smvp_tjds_spmm, K10), against what it stands beside.

    python tools/exp_tjds_spmm.py [--cases headline,pwt459,config4] [--ks 1,2,4,8,16,32] [--window 0.3] [--repeats 3]
                                  [--only k10] [--out profiles/tjds_spmm_k_sweep.txt]

Matrices: memplus x944 and pwt x459 (kron(I, A) as tools/exp_tiled.py builds it) and BASELINE config 4 (synth_csr uniform,
10 M x 10 M, 32 per row), as in tools/exp_spmm_transposed.py.  Per matrix and k, in one process, the variants alternated window
by window, `repeats` windows of at least `window` seconds each, device events:

    K10        smvp_tjds_spmm with k vectors, contiguous operands (ldx = ldy = k); its plan is built before the first window
    k x spmv   k times (smvp_tjds_set_x + smvp_tjds_spmv, default mode) on the SAME handle, vector v of a (k, cols) block into
               vector v of a (k, rows) block -- the contiguous copy of every column of X a caller without K10 has to make first is
               NOT in the window (it would only add to this variant)
    csr spmm   smvp_csr_spmm with the same k on a CSR handle of the same matrix (the second-copy route)

Prints ms per product of every window, the median and the spread (max - min) / median of the windows, K10's share of 8 TB/s by
algorithmic bytes, its gathered rows of X per second (one per entry), the ratios k x spmv / K10 and csr spmm / K10, and the
SpMM plan's bytes and build time.  Before the windows K10 is held against csr spmm (another order of summation inside a row:
1e-9 of the largest element, not bits) and two K10 calls against each other (bits).  The lines go to stdout and to --out.
--only k10 runs K10 alone (for a profiler pass that should see one kernel).  Development aid only; bench.py is the measured
contract.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,pwt459,config4")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of products per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="", help="k10: run that variant alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tjds_spmm_k_sweep.txt"), help="'' = stdout only")
    a = ap.parse_args()
    import torch
    import smvp_toolkit_amd as sm
    from exp_transposed import CASES, device_coo, timed

    out = open(a.out, "w") if a.out else None

    def say(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    ks = [int(k) for k in a.ks.split(",")]
    say("# tools/exp_tjds_spmm.py --cases %s --ks %s --window %g --repeats %d%s" % (a.cases, a.ks, a.window, a.repeats,
                                                                                 " --only " + a.only if a.only else ""))
    say("# device %s; window >= %.2f s, %d windows per variant, variants alternated" % (sm.device_info(0)[0], a.window, a.repeats))
    for case in a.cases.split(","):
        name, rows, cols, rp, ci, v = CASES[case]()
        nnz = int(rp[-1])
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        d_rp, d_ci, d_v = dev(rp), dev(ci), dev(v)
        A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_v)
        d_coo = device_coo(torch, rows, d_rp, d_ci, d_v, nnz)
        T = sm.TjdsMatrix(sm.tjds_from_coo_device(d_coo, rows, cols, nnz))
        del d_coo
        if a.only == "k10":
            A.close()
            A = None
            del d_rp, d_ci, d_v
        say("# %s: rows=%d cols=%d nnz=%d diagonals=%d; k x spmv runs %s" % (name, rows, cols, nnz, T._t.num_diag, T.describe()[0]))
        say("%-14s %3s %-9s %-30s %9s %7s %8s %9s %8s" % ("matrix", "k", "variant", "ms per product, every window", "median", "spread%",
                                                         "% 8TB/s", "G rows/s", "/ K10"))
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2025)
        for k in ks:
            X = torch.rand(cols, k, dtype=torch.float64, device="cuda", generator=gen)
            Y = torch.empty(rows, k, dtype=torch.float64, device="cuda")
            xs = X.t().contiguous()                      # (k, cols): vector v contiguous, for the set_x calls
            ys = torch.empty(k, rows, dtype=torch.float64, device="cuda")

            def spmv_calls():
                for i in range(k):
                    T.set_x(xs[i])
                    T.spmv(ys[i])

            variants = {"K10": lambda: T.spmm(X, Y)}
            if a.only != "k10":
                Yc = torch.empty(rows, k, dtype=torch.float64, device="cuda")
                variants["k x spmv"] = spmv_calls
                variants["csr spmm"] = lambda: A.spmm(X, Yc)
            reps = {}
            for what, fn in variants.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                reps[what] = max(1, int(a.window / max(timed(torch, fn, 2) * 1e-3, 1e-6)) + 1)
            first = Y.clone()
            T.spmm(X, Y)
            torch.cuda.synchronize()
            assert torch.equal(Y.view(torch.int64), first.view(torch.int64)), "two K10 calls differ"
            del first
            if a.only != "k10":                          # the routes agree before they are timed
                for other, what in ((Yc, "csr spmm"), (ys.t(), "k x spmv")):
                    err = float((Y - other).abs().max()) / max(float(other.abs().max()), 1e-300)
                    assert err <= 1e-9, "K10 and %s differ by %g of the largest element" % (what, err)
            ms = {what: [] for what in variants}
            for _ in range(a.repeats):
                for what, fn in variants.items():
                    ms[what].append(timed(torch, fn, reps[what]))
            med = {what: float(np.median(t)) for what, t in ms.items()}
            alg = T.spmm_describe(k)[1]
            for what in variants:
                t = ms[what]
                say("%-14s %3d %-9s %-30s %9.4f %7.2f %8s %9s %8s" % (
                    name, k, what, " ".join("%.4f" % w for w in t), med[what], (max(t) - min(t)) / med[what] * 100,
                    "%.1f" % (alg / (med[what] * 1e-3) / 8e12 * 100) if what == "K10" else "-",
                    "%.1f" % (nnz / (med[what] * 1e-3) * 1e-9) if what == "K10" else "-",
                    "%.2f" % (med[what] / med["K10"])))
            del X, Y, xs, ys
            if a.only != "k10":
                del Yc
            torch.cuda.empty_cache()
        plan = T.spmm_describe(1)[2]
        say("# %s: SpMM plan %.0f bytes (matrix %.0f), built in %.1f ms; kernels at k = 8: %s" % (
            name, plan["plan_bytes"], T.plan_info()["matrix_bytes"], plan["build_ms"], T.spmm_describe(8)[0]))
        T.close()
        if A is not None:
            A.close()
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
