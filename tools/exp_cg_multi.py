#!/usr/bin/env python3
"""K20 (smvp_csr_cg_multi) against k calls of smvp_csr_cg / smvp_csr_pcg on the same handle -- the only way to the same k solutions
before K20 -- and against its own model: wall time per step.

    python tools/exp_cg_multi.py [--cases headline,small] [--ks 1,2,4,8,16] [--repeats 3] [--out FILE]

Matrices: tests/cg_method.py's spd(n) at the headline workload's row count (16 763 552 rows; 30 steps) and at n = 1003 (150 steps),
where the launches and not the bytes decide the time.  Per matrix and k, after one warm run of each form, `repeats` rounds that
alternate
  (i)   the block product alone, `steps` calls of spmm on k columns between one pair of events / steps;
  (ii)  k calls of cg(tol = 0, max_steps = steps, check_every = 10), one per column: the host's clock around the k calls / steps;
  (iii) one call of cg_multi on the k columns with the same options: the host's clock around the call / steps;
  (iv), (v)  the same two with m = the diagonal (k calls of pcg against cg_multi(m = ...)).
Every clock is around whole calls, which return after a synchronise: workspace allocation, step 0 and the history copies included.
Prints every round, the medians, the spreads, the ratios (ii) / (iii) and (iv) / (v) -- the speed-up; the cross-over is the first
k at which it passes 1 -- and the model: (i) + 10 k (12 k with m) vector passes at the copy bandwidth of
profiles/r01_copy_bandwidth.txt (5.2 TB/s at 256 MB to 2 GB).  Checks that no run stopped early and that every column of (iii)
agrees with its run of (ii) to 1e-9 of |x| (the products differ in their order of additions where the handle's plan is not the
serial loop), and says whether the bits agree.  Development aid only; bench.py is the measured contract.
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
CASES = {"headline": (16763552, 30), "small": (1003, 150)}
EVERY = 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,small")
    ap.add_argument("--ks", default="1,2,4,8,16")
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

    ks = [int(k) for k in a.ks.split(",")]
    say("# device %s; ms per step at tol 0, check_every %d; (i) = spmm(k) alone by events, (ii) = k calls of smvp_csr_cg, (iii) = one "
        "smvp_csr_cg_multi, (iv) = k calls of smvp_csr_pcg, (v) = smvp_csr_cg_multi with d_m; host clock around the calls / steps"
        % (sm.device_info(0)[0], EVERY))
    for case in a.cases.split(","):
        n, steps = CASES[case]
        t0 = time.time()
        M = cg.spd(n)
        A = sm.CsrMatrix(n, n, *M.csr)
        name = "spd(%d)" % n
        kmax = max(ks)
        Ball = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, (n, kmax))).cuda()
        m = torch.empty(n, dtype=torch.float64, device="cuda")
        A.diagonal(m)
        say("# %s: nnz=%d, %d steps, SpMV plan %s (%d launches per product), built in %.1f s" % (
            name, M.nnz, steps, A.describe()[0][:70], A.launches(), time.time() - t0))
        del M
        crossover = {"plain": None, "jacobi": None}
        for k in ks:
            B = Ball[:, :k].contiguous()
            cols = [B[:, v].contiguous() for v in range(k)]
            X = torch.empty((n, k), dtype=torch.float64, device="cuda")
            xs = [torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(k)]
            Q = torch.empty((n, k), dtype=torch.float64, device="cuda")

            def product_alone():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(steps):
                    A.spmm(B, Q)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / steps

            def singles(jacobi):
                torch.cuda.synchronize()
                t = time.perf_counter()
                for v in range(k):
                    r = (A.pcg(cols[v], xs[v], m, max_steps=steps, tol=0.0, check_every=EVERY) if jacobi else
                         A.cg(cols[v], xs[v], max_steps=steps, tol=0.0, check_every=EVERY))[0]
                    assert r.steps == steps and r.reason == sm.CG_MAX_STEPS, (r.steps, r.reason)
                return (time.perf_counter() - t) * 1e3 / steps

            def multi(jacobi):
                torch.cuda.synchronize()
                t = time.perf_counter()
                results = A.cg_multi(B, X, m=m if jacobi else None, max_steps=steps, tol=0.0, check_every=EVERY)[0]
                ms = (time.perf_counter() - t) * 1e3 / steps
                assert all(r.steps == steps and r.reason == sm.CG_MAX_STEPS for r in results), [(r.steps, r.reason) for r in results]
                return ms

            product_alone()                                        # warm: every code object loaded, every plan built once
            notes = []
            for jacobi in (False, True):
                singles(jacobi)
                multi(jacobi)
                got, want = X.cpu().numpy(), np.stack([x.cpu().numpy() for x in xs], axis=1)
                err = np.abs(got - want).max() / np.abs(want).max()
                assert err <= 1e-9, "cg_multi and the k single calls disagree: %g" % err
                notes.append("%s: columns agree to %.1e of |x|, bits %s" % ("jacobi" if jacobi else "plain", err,
                                                                           "equal" if np.array_equal(got.view(np.int64), want.view(np.int64)) else "differ"))
            t = {key: [] for key in ("i", "ii", "iii", "iv", "v")}
            for rnd in range(a.repeats):
                t["i"].append(product_alone())
                t["ii"].append(singles(False))
                t["iii"].append(multi(False))
                t["iv"].append(singles(True))
                t["v"].append(multi(True))
                say("%-14s k %2d round %d  (i) %.4f  (ii) %.4f  (iii) %.4f  (iv) %.4f  (v) %.4f" % (
                    name, k, rnd, t["i"][-1], t["ii"][-1], t["iii"][-1], t["iv"][-1], t["v"][-1]))
            med = {key: float(np.median(v)) for key, v in t.items()}
            spread = {key: 100 * (max(v) - min(v)) / med[key] for key, v in t.items()}
            one_pass = 8.0 * n / (COPY_TBS * 1e12) * 1e3
            for label, single, many, passes in (("plain", "ii", "iii", 10), ("jacobi", "iv", "v", 12)):
                model = med["i"] + passes * k * one_pass
                speedup = med[single] / med[many]
                if speedup > 1.0 and crossover[label] is None:
                    crossover[label] = k
                say("%-14s k %2d %-6s median: spmm %.4f (spread %.1f %%), %d x one-vector %.4f (%.1f %%), cg_multi %.4f (%.1f %%): speed-up "
                    "%.2f; beside the product %.4f ms = %.3g x (%d passes at %.1f TB/s = %.4g ms); model %.4f, measured / model %.2f" % (
                        name, k, label, med["i"], spread["i"], k, med[single], spread[single], med[many], spread[many], speedup,
                        med[many] - med["i"], (med[many] - med["i"]) / (passes * k * one_pass), passes * k, COPY_TBS, passes * k * one_pass,
                        model, med[many] / model))
            say("%-14s k %2d %s" % (name, k, "; ".join(notes)))
            del B, cols, X, xs, Q
            torch.cuda.empty_cache()
        say("%-14s cross-over (the first k of %s at which cg_multi is faster than k one-vector calls): plain k = %s, jacobi k = %s" % (
            name, ks, crossover["plain"], crossover["jacobi"]))
        A.close()
        del Ball, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
