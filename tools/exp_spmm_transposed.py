#!/usr/bin/env python3
"""Y = A^T X for a block of k vectors from the TJDS arrays (smvp_tjds_spmm_transposed, K9), against what it stands beside.

    python tools/exp_spmm_transposed.py [--cases headline,pwt459,config4] [--ks 1,2,4,8,16,32] [--window 0.3] [--repeats 3]
                                        [--only k9]

Matrices: memplus x944 and pwt x459 (kron(I, A) as tools/exp_tiled.py builds it) and BASELINE config 4 (synth_csr uniform,
10 M x 10 M, 32 per row), as in tools/exp_transposed.py.  Per matrix and k, in one process, the variants alternated window by
window, `repeats` windows of at least `window` seconds each, device events:

    K9        smvp_tjds_spmm_transposed with k vectors, contiguous operands (ldx = ldy = k)
    k x K8    k calls of smvp_tjds_spmv_transposed on the SAME handle, vector v of a (k, rows) block into vector v of a
              (k, cols) block (contiguous vectors: what a caller without K9 does)
    At spmm   smvp_csr_spmm with the same k on the handle smvp_csr_create_transposed made (the second-copy route)

Prints ms per product of every window, the median and the spread (max - min) / median of the windows, K9's share of 8 TB/s by
algorithmic bytes, its gathered rows of X per second (one per entry) and the ratios k x K8 / K9 and At spmm / K9.  --only k9
runs K9 alone (for a profiler pass that should see one kernel).  Development aid only; bench.py is the measured contract.
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
    ap.add_argument("--only", default="", help="k9: run that variant alone")
    a = ap.parse_args()
    import torch
    import smvp_toolkit_amd as sm
    from exp_transposed import CASES, device_coo, timed

    ks = [int(k) for k in a.ks.split(",")]
    print("# device %s; window >= %.2f s, %d windows per variant, variants alternated" % (sm.device_info(0)[0], a.window, a.repeats),
          flush=True)
    for case in a.cases.split(","):
        name, rows, cols, rp, ci, v = CASES[case]()
        nnz = int(rp[-1])
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        d_rp, d_ci, d_v = dev(rp), dev(ci), dev(v)
        A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_v)
        d_coo = device_coo(torch, rows, d_rp, d_ci, d_v, nnz)
        T = sm.TjdsMatrix(sm.tjds_from_coo_device(d_coo, rows, cols, nnz))
        del d_coo
        At = None if a.only == "k9" else A.transposed()
        A.close()
        del d_rp, d_ci, d_v
        print("# %s: rows=%d cols=%d nnz=%d diagonals=%d" % (name, rows, cols, nnz, T._t.num_diag), flush=True)
        print("%-14s %3s %-9s %-30s %9s %7s %8s %9s %8s" % ("matrix", "k", "variant", "ms per product, every window", "median", "spread%",
                                                         "% 8TB/s", "G rows/s", "/ K9"), flush=True)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2025)
        for k in ks:
            X = torch.rand(rows, k, dtype=torch.float64, device="cuda", generator=gen)
            Y = torch.empty(cols, k, dtype=torch.float64, device="cuda")
            xs = X.t().contiguous()                      # (k, rows): vector v contiguous, for the K8 calls
            ys = torch.empty(k, cols, dtype=torch.float64, device="cuda")

            def k8_calls():
                for i in range(k):
                    T.spmv_transposed(xs[i], ys[i])

            variants = {"K9": lambda: T.spmm_transposed(X, Y)}
            if a.only != "k9":
                variants["k x K8"] = k8_calls
                variants["At spmm"] = lambda: At.spmm(X, Y)
            reps = {}
            for what, fn in variants.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                reps[what] = max(1, int(a.window / max(timed(torch, fn, 2) * 1e-3, 1e-6)) + 1)
            if a.only != "k9":                           # the three routes agree before they are timed
                Yt = ys.t()
                assert torch.equal(Y.view(torch.int64), Yt.contiguous().view(torch.int64)), "K9 and k x K8 differ"
            ms = {what: [] for what in variants}
            for _ in range(a.repeats):
                for what, fn in variants.items():
                    ms[what].append(timed(torch, fn, reps[what]))
            med = {what: float(np.median(t)) for what, t in ms.items()}
            alg = T.spmm_transposed_describe(k)[1]
            for what in variants:
                t = ms[what]
                print("%-14s %3d %-9s %-30s %9.4f %7.2f %8s %9s %8s" % (
                    name, k, what, " ".join("%.4f" % w for w in t), med[what], (max(t) - min(t)) / med[what] * 100,
                    "%.1f" % (alg / (med[what] * 1e-3) / 8e12 * 100) if what == "K9" else "-",
                    "%.1f" % (nnz / (med[what] * 1e-3) * 1e-9) if what == "K9" else "-",
                    "%.2f" % (med[what] / med["K9"])), flush=True)
            del X, Y, xs, ys
            torch.cuda.empty_cache()
        T.close()
        if At is not None:
            At.close()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
