#!/usr/bin/env python3
"""K16: smvp_csr_pcg_tri (symmetric Gauss-Seidel on the matrix itself) against smvp_csr_pcg (Jacobi) and smvp_csr_cg: wall time per
step, and steps and wall time to tol = 1e-8.

    python tools/exp_pcg_tri.py [--cases headline,small] [--repeats 3] [--out FILE]

Matrices: tests/cg_method.py's spd(n) at the headline workload's row count (16 763 552 rows; 50 steps) and at n = 1003 (50 steps),
the shapes of profiles/pcg_measured.txt.  first = LOWER / DIAG_STORED and second = UPPER / DIAG_STORED on the handle itself, m = the
handle's own diagonal (smvp_csr_diagonal).  Per matrix, after one warm run of each form, `repeats` rounds that alternate, in one
process,
  (i)    the handle's product alone and (l), (u) each plan's solve alone: `steps` calls between one pair of events / steps;
  (pcg)  pcg(tol = 0, max_steps = steps) and
  (tri)  pcg_tri(tol = 0, max_steps = steps), each at check_every = 1, 10 and steps: the host's clock around the whole call (it
         returns after a synchronise; workspace allocation, step 0 and the history copies included) / steps;
then cg, pcg and pcg_tri to tol = 1e-8 at check_every = 1 and 10: steps, and the host's clock around the call (median of `repeats`).
The expectation, derived and written down before the first run (profiles/pcg_tri_measured.txt has it in full): a (tri) step is a
(pcg) step minus its two reads of m plus five vector passes -- three more passes of 8 n bytes at the 5.2 TB/s of
profiles/r01_copy_bandwidth.txt -- plus the two solves; at n = 1003 it is the (pcg) step plus two launches plus the solves' launches.
"met" is a (tri) step within 1.10 x of (pcg) + the passes + (l) + (u) as measured in the same process.  Development aid only;
bench.py is the measured contract.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBS = 5.2                   # profiles/r01_copy_bandwidth.txt: copy 256 MB 5476, 1024 MB 4811, 2048 MB 5160 GB/s
EXTRA_PASSES = 3                 # vector passes of a K16 step beyond K14's twelve: fifteen, without the two reads of m
LAUNCH_MS = 0.0021               # back-to-back host wall per launch (README)
CASES = {"headline": (16763552, 50), "small": (1003, 50)}       # (at n = 1003 SGS reaches rr = 0 exactly at step 79: tol = 0 stops there)
TOL = 1e-8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,small")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import cg_method as cg
    import smvp_toolkit_amd as sm

    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say("# device %s; ms per step; (i) = spmv alone, (l) / (u) = the lower / upper solve alone, by events; (pcg) = smvp_csr_pcg with m = "
        "smvp_csr_diagonal, (tri) = smvp_csr_pcg_tri with the two plans of the handle itself and the same m, both tol 0, host clock "
        "around the call / steps" % (sm.device_info(0)[0],))
    say("# expectation (derived, not measured): (tri) = (pcg) + %d vector passes at %.1f TB/s + (l) + (u), and %d launches more at "
        "n = 1003; met = within 1.10 x" % (EXTRA_PASSES, COPY_TBS, 2))
    for case in [c for c in a.cases.split(",") if c]:
        n, steps = CASES[case]
        t0 = time.time()
        M = cg.spd(n)
        A = sm.CsrMatrix(n, n, *M.csr)
        b = torch.from_numpy(cg.rhs(n)).cuda()
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        m = A.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
        L, U = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
        name = "spd(%d)" % n
        everys = sorted({1, 10, steps})
        say("# %s: nnz=%d, %d steps, plan %s (%d launches per product); lower solve %d launches (%d chains, %d levels), upper %d (%d, %d); "
            "built in %.1f s" % (name, M.nnz, steps, A.describe()[0][:70], A.launches(), L.info()["launches"], L.info()["chains"],
                                 L.info()["levels"], U.info()["launches"], U.info()["chains"], U.info()["levels"], time.time() - t0))

        def by_events(call):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        p, q = b.clone(), torch.empty_like(b)
        alone = {"i": lambda: A.spmv(p, q), "l": lambda: L.solve(p, q), "u": lambda: U.solve(p, q)}

        def library(form, every, max_steps=steps, tol=0.0):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if form == "tri":
                r = A.pcg_tri(b, x, L, U, m=m, max_steps=max_steps, tol=tol, check_every=every)[0]
            elif form == "pcg":
                r = A.pcg(b, x, m, max_steps=max_steps, tol=tol, check_every=every)[0]
            else:
                r = A.cg(b, x, max_steps=max_steps, tol=tol, check_every=every)[0]
            return (time.perf_counter() - t) * 1e3, r

        for call in alone.values():                                # warm: every code object loaded, every plan built once
            by_events(call)
        for form in ("pcg", "tri"):
            bits = None
            for e in everys:
                ms, r = library(form, e)
                assert r.steps == steps and r.reason == sm.CG_MAX_STEPS, (form, r.steps, r.reason)
                got = x.cpu().numpy().view(np.int64)
                assert bits is None or np.array_equal(bits, got), "d_x depends on check_every"
                bits = got
        ta = {k: [] for k in alone}
        tp, tt = {e: [] for e in everys}, {e: [] for e in everys}
        for rnd in range(a.repeats):
            for k, call in alone.items():
                ta[k].append(by_events(call))
            for e in everys:
                tp[e].append(library("pcg", e)[0] / steps)
                tt[e].append(library("tri", e)[0] / steps)
            say("%-14s round %d  (i) %.4f (l) %.4f (u) %.4f  " % (name, rnd, ta["i"][-1], ta["l"][-1], ta["u"][-1]) +
                "  ".join("every %d: (pcg) %.4f (tri) %.4f" % (e, tp[e][-1], tt[e][-1]) for e in everys))
        med = {k: float(np.median(v)) for k, v in ta.items()}
        say("%-14s median (i) %.4f (l) %.4f (u) %.4f ms" % (name, med["i"], med["l"], med["u"]))
        passes = EXTRA_PASSES * 8.0 * n / (COPY_TBS * 1e12) * 1e3
        extra_launches = 2 * LAUNCH_MS if n < 100000 else 0.0
        for e in everys:
            c, t = float(np.median(tp[e])), float(np.median(tt[e]))
            model = c + passes + extra_launches + med["l"] + med["u"]
            say("%-14s median check_every %4d: (pcg) %.4f ms/step, spread %.1f %%; (tri) %.4f ms/step, spread %.1f %%; (tri) / (pcg) = "
                "%.2f; expected (pcg) + %.4f + (l) + (u) = %.4f ms: %.2f x (%s)" % (
                    name, e, c, 100 * (max(tp[e]) - min(tp[e])) / c, t, 100 * (max(tt[e]) - min(tt[e])) / t, t / c,
                    passes + extra_launches, model, t / model, "met" if t <= 1.10 * model else "MISSED"))
        for every in (1, 10):                                      # (steps enqueued after the one that converged run in vain until the next look)
            for form in ("cg", "pcg", "tri"):
                runs = [library(form, every, 2000, TOL) for _ in range(a.repeats + 1)][1:]
                r = runs[0][1]
                ms = float(np.median([t for t, _ in runs]))
                say("%-14s to tol %g, check_every %2d: (%s) %d steps, reason %d, %.3f ms (median of %d; %.4f ms per step), rr / bb = %.3g" % (
                    name, TOL, every, form, r.steps, r.reason, ms, a.repeats, ms / max(r.steps, 1), r.rr / r.bb))
        L.close()
        U.close()
        A.close()
        del M, b, x, m, p, q
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
