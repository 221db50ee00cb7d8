#!/usr/bin/env python3
"""K14: smvp_csr_pcg against smvp_csr_cg and the product alone, wall time per step; the two diagonal kernels against their bytes.

    python tools/exp_pcg.py [--cases headline,small] [--diagonal headline,config4] [--repeats 3] [--out FILE]

Solver.  Matrices: tests/cg_method.py's spd(n) at the headline workload's row count (memplus x944: 16 763 552 rows; 100 steps) and
at n = 1003 (150 steps), the shapes of profiles/cg_measured.txt.  m is the handle's own diagonal (smvp_csr_diagonal).  Per matrix,
after one warm run of each form, `repeats` rounds that alternate, in one process,
  (i)   the handle's product alone, `steps` calls of spmv between one pair of events / steps;
  (cg)  cg(tol = 0, max_steps = steps) and
  (pcg) pcg(tol = 0, max_steps = steps), each at check_every = 1, 10 and steps: the host's clock around the whole call (it returns
        after a synchronise; workspace allocation, step 0 and the history copies included) / steps.
The expectation, derived and written down before the first run: a PCG step is K12's step plus two reads of m, 2 * 8 n bytes at the
5.2 TB/s of profiles/r01_copy_bandwidth.txt -- about 0.05 ms at 16.8 M rows, roughly 5 % over CG's step; at n = 1003 the launches
decide and PCG's step is CG's within launch noise.  The tool prints (pcg) - (cg) beside that figure and says met or missed.

Diagonal.  memplus x944 (kron(I, A), as tools/exp_tiled.py builds it) and BASELINE config 4 (10 M x 10 M, 32 uniform entries per
row), windows of at least --window seconds by events.  Bytes: CSR 4 per entry (col_ind) + 4 (rows + 1) (row_ptr) + 8 per row
written; TJDS 4 per entry (row_ind) + 4 (num_diag + 1) + 4 cols (perm) + 8 per row written; val is read at the matches only and is
not counted.  Expected within 1.5 x of those bytes at 5.2 TB/s.  Both results are checked against torch (the sum of the entries
with row == column, which do not repeat in these matrices) bit for bit.  Development aid only; bench.py is the measured contract.
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

COPY_TBS = 5.2                   # profiles/r01_copy_bandwidth.txt: copy 256 MB 5476, 1024 MB 4811, 2048 MB 5160 GB/s
EXTRA_PASSES = 2                 # vector passes of a K14 step beyond K12's ten: m read by pcg_residual and by pcg_direction
CASES = {"headline": (16763552, 100), "small": (1003, 150)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,small")
    ap.add_argument("--diagonal", default="headline,config4")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of diagonal calls per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import cg_method as cg
    import exp_transposed as xt
    import smvp_toolkit_amd as sm

    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say("# device %s; ms per step; (i) = spmv alone by events, (cg) = smvp_csr_cg, (pcg) = smvp_csr_pcg with m = smvp_csr_diagonal, "
        "both tol 0, host clock around the call / steps" % (sm.device_info(0)[0],))
    say("# expectation (derived, not measured): (pcg) - (cg) = %d vector passes at %.1f TB/s; at n = 1003 within launch noise" % (
        EXTRA_PASSES, COPY_TBS))
    for case in [c for c in a.cases.split(",") if c]:
        n, steps = CASES[case]
        t0 = time.time()
        M = cg.spd(n)
        A = sm.CsrMatrix(n, n, *M.csr)
        b = torch.from_numpy(cg.rhs(n)).cuda()
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        m = A.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
        name = "spd(%d)" % n
        everys = sorted({1, 10, steps})
        say("# %s: nnz=%d, %d steps, plan %s (%d launches per product), built in %.1f s" % (
            name, M.nnz, steps, A.describe()[0][:70], A.launches(), time.time() - t0))

        def product_alone():
            p, q = b.clone(), torch.empty_like(b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                A.spmv(p, q)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        def library(pre, every):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = (A.pcg(b, x, m, max_steps=steps, tol=0.0, check_every=every) if pre else
                 A.cg(b, x, max_steps=steps, tol=0.0, check_every=every))[0]
            ms = (time.perf_counter() - t) * 1e3 / steps
            assert r.steps == steps and r.reason == sm.CG_MAX_STEPS, (pre, r.steps, r.reason)
            return ms, r

        product_alone()                                            # warm: every code object loaded, every plan built once
        for pre in (False, True):
            bits = None
            for e in everys:
                library(pre, e)
                got = x.cpu().numpy().view(np.int64)
                assert bits is None or np.array_equal(bits, got), "d_x depends on check_every"
                bits = got
        ti, tc, tp = [], {e: [] for e in everys}, {e: [] for e in everys}
        for rnd in range(a.repeats):
            ti.append(product_alone())
            for e in everys:
                tc[e].append(library(False, e)[0])
                tp[e].append(library(True, e)[0])
            say("%-14s round %d  (i) %.4f  " % (name, rnd, ti[-1]) +
                "  ".join("every %d: (cg) %.4f (pcg) %.4f" % (e, tc[e][-1], tp[e][-1]) for e in everys))
        mi = float(np.median(ti))
        model = EXTRA_PASSES * 8.0 * n / (COPY_TBS * 1e12) * 1e3
        say("%-14s median (i) %.4f ms/step, spread %.1f %%" % (name, mi, 100 * (max(ti) - min(ti)) / mi))
        for e in everys:
            c, p = float(np.median(tc[e])), float(np.median(tp[e]))
            noise = max(max(tc[e]) - min(tc[e]), max(tp[e]) - min(tp[e]))
            say("%-14s median check_every %4d: (cg) %.4f ms/step, spread %.1f %%; (pcg) %.4f ms/step, spread %.1f %%; (pcg) / (cg) = "
                "%.3f, (pcg) / (i) = %.3f, (pcg) - (cg) = %.4f ms against %d passes at %.1f TB/s = %.3g ms (the rounds differ by up to "
                "%.4f ms)" % (name, e, c, 100 * (max(tc[e]) - min(tc[e])) / c, p, 100 * (max(tp[e]) - min(tp[e])) / p, p / c, p / mi,
                              p - c, EXTRA_PASSES, COPY_TBS, model, noise))
        r = library(True, everys[-1])[1]
        say("%-14s rr_%d = %.6g, rz_%d = %.6g, bb = %.6g; d_x bit-equal at every check_every, for cg and for pcg" % (
            name, r.updates, r.rr, r.updates, r.rz, r.bb))
        A.close()
        del M, b, x, m
        torch.cuda.empty_cache()

    for case in [c for c in a.diagonal.split(",") if c]:
        name, rows, cols, rp, ci, v = xt.CASES[case]()
        nnz = int(rp[-1])
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        d_rp, d_ci, d_v = dev(rp), dev(ci), dev(v)
        A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_v)
        d_coo = xt.device_coo(torch, rows, d_rp, d_ci, d_v, nnz)
        T = sm.TjdsMatrix(sm.tjds_from_coo_device(d_coo, rows, cols, nnz))
        del d_coo
        row_of = torch.repeat_interleave(torch.arange(rows, dtype=torch.int64, device="cuda"), (d_rp[1:] - d_rp[:-1]).to(torch.int64))
        on = row_of == d_ci[:nnz].to(torch.int64)
        want = torch.zeros(rows, dtype=torch.float64, device="cuda")
        want.index_add_(0, row_of[on], d_v[:nnz][on])
        assert int(torch.bincount(row_of[on], minlength=rows).max()) <= 1, "a repeated diagonal entry: index_add_ has no order"
        del row_of
        out = torch.empty(rows, dtype=torch.float64, device="cuda")
        forms = {"csr": (A, 4.0 * nnz + 4.0 * (rows + 1) + 8.0 * rows),
                 "tjds": (T, 4.0 * nnz + 4.0 * (T._t.num_diag + 1) + 4.0 * cols + 8.0 * rows)}
        say("# %s: rows=%d cols=%d nnz=%d (%.1f per row), diagonals=%d, %d diagonal entries stored" % (
            name, rows, cols, nnz, nnz / max(rows, 1), T._t.num_diag, int(on.sum())))
        ms = {k: [] for k in forms}
        for k, (H, _) in forms.items():
            out.fill_(float("nan"))
            H.diagonal(out)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int64), want.view(torch.int64)), "%s: the %s diagonal differs from torch's" % (name, k)
        for rnd in range(a.repeats):
            for k, (H, _) in forms.items():
                one = xt.timed(torch, lambda: H.diagonal(out), 3)
                ms[k].append(xt.timed(torch, lambda: H.diagonal(out), max(3, int(a.window * 1e3 / max(one, 1e-3)))))
        for k, (H, nbytes) in forms.items():
            med = float(np.median(ms[k]))
            floor = nbytes / (COPY_TBS * 1e12) * 1e3
            say("%-16s %-4s diagonal: %s ms, median %.4f, spread %.1f %%; %.1f MB = %.4f ms at %.1f TB/s: %.2f x its bytes (%s 1.5 x), "
                "%.0f GB/s" % (name, k, " ".join("%.4f" % t for t in ms[k]), med, 100 * (max(ms[k]) - min(ms[k])) / med, nbytes / 1e6,
                               floor, COPY_TBS, med / floor, "within" if med <= 1.5 * floor else "MISSES", nbytes / med / 1e6))
        A.close()
        T.close()
        del d_rp, d_ci, d_v, want, out, on
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
