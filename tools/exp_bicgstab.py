#!/usr/bin/env python3
"""K13 (smvp_csr_bicgstab) against twice the product alone and against the loop a caller composes today: wall time per step.

    python tools/exp_bicgstab.py [--cases headline,small] [--repeats 3] [--out FILE]

Matrices: tests/bicgstab_method.py's nonsym(n) -- 0 to 8 entries per row off the diagonal, not mirrored, a dominant diagonal, about
5 entries per row -- at the headline workload's row count (memplus x944: 16 763 552 rows; 100 steps) and at n = 1003 (150 steps),
where the launches and not the bytes decide the time.  Per matrix, after one warm run of each form, `repeats` rounds that alternate
  (i)   the handle's product alone, 2 * `steps` calls of spmv between one pair of events / steps: the two products of a step;
  (ii)  the loop a caller writes today on the same handle and stream: spmv, torch.dot, the host reads sigma, torch.add (s), torch.dot
        (ss, read), spmv, two torch.dot (ts, tt, read), two add_ (x), torch.add (r), two torch.dot (rr, rho, read), add_ and torch.add
        (p) -- six host reads per step; the host's clock around the loop / steps;
  (iii) bicgstab(tol = 0, max_steps = steps) at check_every = 1, 10 and steps: the host's clock around the whole call (it returns
        after a synchronise; workspace allocation, step 0 and the two history copies included) / steps.
A call of one step (max_steps = 1) is timed too: what a call costs before its steps, which (ii) has no counterpart of -- its vectors
come from torch's caching allocator before its clock starts.
Prints every round, the medians, the spreads and the ratios (iii) / (i) and (iii) / (ii); the cost beside the products, (iii) - (i),
against eighteen vector passes at the copy bandwidth of profiles/r01_copy_bandwidth.txt (5.2 TB/s at 256 MB to 2 GB).  Checks that
no run stopped early, that (iii) gives the same bits at every check_every, and that (ii) and (iii) agree to 1e-9 of |x| after
CHECK_STEPS steps (other orders of summation; later the residual is rounding noise and the two runs part).  Development aid only;
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
PASSES = 18                      # vector passes of a K13 step beside the two products
CHECK_STEPS = 8                  # the composed loop and the library are compared after this many steps
CASES = {"headline": (16763552, 100), "small": (1003, 150)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,small")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import bicgstab_method as bi
    import smvp_toolkit_amd as sm

    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    say("# device %s; ms per step; (i) = two spmv alone by events, (ii) = spmv + torch.dot / torch.add with six host reads per step, "
        "(iii) = smvp_csr_bicgstab tol 0, host clock around the call / steps" % (sm.device_info(0)[0],))
    for case in a.cases.split(","):
        n, steps = CASES[case]
        t0 = time.time()
        M = bi.nonsym(n)
        A = sm.CsrMatrix(n, n, *M.csr)
        b = torch.from_numpy(bi.rhs(n)).cuda()
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        name = "nonsym(%d)" % n
        everys = sorted({1, 10, steps})
        say("# %s: nnz=%d, %d steps, plan %s (%d launches per product), built in %.1f s" % (
            name, M.nnz, steps, A.describe()[0][:70], A.launches(), time.time() - t0))

        def products_alone():
            p, q = b.clone(), torch.empty_like(b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(2 * steps):
                A.spmv(p, q)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / steps

        def composed(steps=steps):
            """Breakdowns are not looked for: at tol 0 the library goes on as long as its numbers are finite and not zero too."""
            xs, r, v, t = torch.zeros_like(b), b.clone(), torch.empty_like(b), torch.empty_like(b)
            rhat, p, s = r.clone(), r.clone(), torch.empty_like(b)
            torch.cuda.synchronize()
            clock = time.perf_counter()
            rho = torch.dot(r, r).item()
            for _ in range(steps):
                A.spmv(p, v)
                alpha = rho / torch.dot(rhat, v).item()
                torch.add(r, v, alpha=-alpha, out=s)
                torch.dot(s, s).item()                             # ss: the half-step stop rule reads it
                A.spmv(s, t)
                omega = torch.dot(t, s).item() / torch.dot(t, t).item()
                xs.add_(p, alpha=alpha)
                xs.add_(s, alpha=omega)
                torch.add(s, t, alpha=-omega, out=r)
                torch.dot(r, r).item()                             # rr: the stop rule reads it
                rho_new = torch.dot(rhat, r).item()
                beta = (rho_new / rho) * (alpha / omega)
                p.add_(v, alpha=-omega)
                torch.add(r, p, alpha=beta, out=p)
                rho = rho_new
            torch.cuda.synchronize()
            return (time.perf_counter() - clock) * 1e3 / steps, xs

        def library(every, steps=steps):
            torch.cuda.synchronize()
            clock = time.perf_counter()
            r, rr, ss = A.bicgstab(b, x, max_steps=steps, tol=0.0, check_every=every)
            ms = (time.perf_counter() - clock) * 1e3 / steps
            assert r.steps == steps and r.reason == sm.BICGSTAB_MAX_STEPS, (r.steps, r.full, r.half, r.reason)
            return ms, r, rr

        products_alone()                                           # warm: every code object loaded, every plan built once
        composed()
        xs = composed(CHECK_STEPS)[1].cpu().numpy()
        library(1, CHECK_STEPS)
        err = np.abs(x.cpu().numpy() - xs).max() / np.abs(xs).max()
        assert err <= 1e-9, "the composed loop and the library disagree after %d steps: %g" % (CHECK_STEPS, err)
        bits = None
        for e in everys:
            library(e)
            got = x.cpu().numpy().view(np.int64)
            assert bits is None or np.array_equal(bits, got), "d_x depends on check_every"
            bits = got
        ti, tii, tiii, one = [], [], {e: [] for e in everys}, []
        for rnd in range(a.repeats):
            one.append(library(1, 1)[0])
            ti.append(products_alone())
            tii.append(composed()[0])
            for e in everys:
                tiii[e].append(library(e)[0])
            say("%-16s round %d  (i) %.4f  (ii) %.4f  " % (name, rnd, ti[-1], tii[-1]) +
                "  ".join("(iii) every %d: %.4f" % (e, tiii[e][-1]) for e in everys))
        mi, mii = float(np.median(ti)), float(np.median(tii))
        say("%-16s median (i) %.4f ms/step, spread %.1f %%; (ii) %.4f ms/step, spread %.1f %%, (ii) - (i) = %.4f" % (
            name, mi, 100 * (max(ti) - min(ti)) / mi, mii, 100 * (max(tii) - min(tii)) / mii, mii - mi))
        model = PASSES * 8.0 * n / (COPY_TBS * 1e12) * 1e3
        for e in everys:
            m = float(np.median(tiii[e]))
            say("%-16s median (iii) check_every %4d: %.4f ms/step, spread %.1f %%, (iii) / (i) = %.3f, (iii) / (ii) = %.3f, "
                "beside the products %.4f ms = %.3g x (%d passes at %.1f TB/s = %.3g ms)" % (
                    name, e, m, 100 * (max(tiii[e]) - min(tiii[e])) / m, m / mi, m / mii, m - mi, (m - mi) / model, PASSES, COPY_TBS, model))
        m1, m = float(np.median(one)), float(np.median(tiii[everys[-1]]))
        say("%-16s a call of one step takes %.4f ms (workspace, step 0, one step, the history copies): the steps after the first cost "
            "%.4f ms each at check_every %d, %.4f beside the products" % (name, m1, (m * steps - m1) / (steps - 1), everys[-1],
                                                                         (m * steps - m1) / (steps - 1) - mi))
        r, rr = library(everys[-1])[1:]
        say("%-16s rr_0 = %.6g, rr_%d = %.6g, bb = %.6g; (ii) and (iii) agree to %.1e of |x| after %d steps; d_x bit-equal at every "
            "check_every" % (name, rr[0], r.full, r.rr, r.bb, err, CHECK_STEPS))
        A.close()
        del M, b, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
