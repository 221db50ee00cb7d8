#!/usr/bin/env python3
"""K7 (smvp_csr_spmm) against k smvp_csr_spmv calls: one product with k vectors, and the same k columns one at a time.

    python tools/exp_spmm.py [--cases headline,config4] [--ks 1,2,4,8,16,32] [--window 0.5]

Matrices: memplus x944 (kron(I, memplus) as tools/exp_tiled.py builds it) and BASELINE config 4 (synth_csr uniform,
10 M x 10 M, 32 per row, as tools/exp_csr.py builds it).  For every k: a few warm calls, then rounds that alternate spmm
(k vectors at once) and k spmv calls (AUTO plan) on the same k columns, each timed with device events; at least `window`
seconds of each.  Prints the median ms per round of each, GFLOP/s (2 nnz k / t), the fraction of 8 TB/s by algorithmic bytes
(12 nnz + 4 (rows + 1) + 8 k (cols + rows)) and the speed-up.  Checks every column of Y against spmv's y within
parity.check_y's bound and that two spmm calls give the same bits.  Development aid only; bench.py is the measured contract.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def headline():
    import oracle_binding as ob
    import smvp_toolkit_amd as sm
    from exp_tiled import tile_csr

    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path("memplus.mtx"))
    rp, ci, v = sm.csr_from_coo(coo, m)
    copies = (1 << 24) // m
    RP, CI, V = tile_csr(rp, ci, v, m, n, copies)
    return "memplus x%d" % copies, m * copies, n * copies, RP, CI, V


def config4():
    import smvp_toolkit_amd as sm

    N = 10_000_000
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 12345, N, N, 32)
    return "config 4", N, N, rp, ci, v


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,config4")
    ap.add_argument("--ks", default="1,2,4,8,16,32")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed calls of each form per k (at least)")
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    import torch
    import smvp_toolkit_amd as sm
    from parity import check_y

    ks = [int(k) for k in a.ks.split(",")]
    print("# device %s; spmm = one smvp_csr_spmm with k vectors, spmv = k smvp_csr_spmv calls (AUTO plan) on the same columns"
          % (sm.device_info(0)[0],), flush=True)
    for case in a.cases.split(","):
        t0 = time.time()
        name, rows, cols, rp, ci, v = {"headline": headline, "config4": config4}[case]()
        nnz = int(rp[-1])
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        A = sm.CsrMatrix(rows, cols, dev(rp), dev(ci), dev(v))
        Aabs = None if a.no_check else sm.CsrMatrix(rows, cols, dev(rp), dev(ci), dev(np.abs(v)))
        terms = np.diff(rp)
        print("# %s: rows=%d cols=%d nnz=%d, SpMV plan %s, built in %.1f s" % (name, rows, cols, nnz, A.describe()[0], time.time() - t0),
              flush=True)
        print("%-12s %3s %-52s %10s %9s %7s %12s %8s" % ("matrix", "k", "spmm kernels", "spmm ms", "GFLOP/s", "% 8TB/s",
                                                       "k x spmv ms", "speed-up"), flush=True)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2024)
        for k in ks:
            X = torch.rand(cols, k, dtype=torch.float64, device="cuda", generator=gen)
            Y = torch.empty(rows, k, dtype=torch.float64, device="cuda")
            xs = [X[:, c].contiguous() for c in range(k)]
            ys = [torch.empty(rows, dtype=torch.float64, device="cuda") for _ in range(k)]

            def run_spmm():
                A.spmm(X, Y)

            def run_spmv():
                for c in range(k):
                    A.spmv(xs[c], ys[c])

            for _ in range(3):
                run_spmm()
                run_spmv()
            torch.cuda.synchronize()
            n_mm = max(1, int(0.05 / max(timed(torch, run_spmm, 1) * 1e-3, 1e-6)))
            n_mv = max(1, int(0.05 / max(timed(torch, run_spmv, 1) * 1e-3, 1e-6)))
            t_mm, t_mv = [], []
            while sum(t_mm) * 1e-3 < a.window or sum(t_mv) * 1e-3 < a.window:  # (sums of per-round ms x calls below)
                t_mm.append(timed(torch, run_spmm, n_mm) * n_mm)
                t_mv.append(timed(torch, run_spmv, n_mv) * n_mv)
            ms_mm = float(np.median([t / n_mm for t in t_mm]))
            ms_mv = float(np.median([t / n_mv for t in t_mv]))
            kname, alg, _ = A.spmm_describe(k)
            print("%-12s %3d %-52s %10.4f %9.1f %7.1f %12.4f %8.2f" % (name, k, kname[:52], ms_mm, 2.0 * nnz * k / ms_mm * 1e-6,
                                                                       alg / (ms_mm * 1e-3) / 8e12 * 100, ms_mv, ms_mv / ms_mm),
                  flush=True)
            if not a.no_check:
                run_spmm()
                run_spmv()
                torch.cuda.synchronize()
                Yh = Y.cpu().numpy()
                Y.fill_(float("nan"))
                run_spmm()
                torch.cuda.synchronize()
                assert np.array_equal(Yh.view(np.int64), Y.cpu().numpy().view(np.int64)), "two spmm calls differ"
                y_abs = torch.empty(rows, dtype=torch.float64, device="cuda")
                for c in range(k):
                    Aabs.spmv(xs[c].abs(), y_abs)
                    torch.cuda.synchronize()
                    check_y(Yh[:, c], ys[c].cpu().numpy(), y_abs.cpu().numpy(), terms)
            del X, Y, xs, ys
            torch.cuda.empty_cache()
        if not a.no_check:
            print("# %s: every column within check_y's bound of spmv's y; two spmm calls bit-equal" % name, flush=True)
        A.close()
        if Aabs is not None:
            Aabs.close()


if __name__ == "__main__":
    main()
