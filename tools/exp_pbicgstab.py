#!/usr/bin/env python3
"""K18: smvp_csr_pbicgstab (Jacobi, symmetric Gauss-Seidel, ILU(0)) against smvp_csr_bicgstab: wall time per step, and steps and wall
time to tol = 1e-8.

    python tools/exp_pbicgstab.py [--cases headline,small,memplus,convdiff] [--repeats 3] [--solve-repeats 1] [--max-steps-plans 2000]
                                  [--out FILE]

Matrices: tests/bicgstab_method.py's nonsym(n) at the headline workload's row count (16 763 552 rows) and at n = 1003 -- as built for
the Jacobi step, with its repeated entries added up (tools/exp_ilu0.py's coalesce) for everything that needs a factor; the golden
sample memplus with its own values; tests/pbicgstab_method.py's convdiff(1024, 0.5).  Per step case, after one warm run of each form,
`repeats` rounds that alternate, in one process,
  (i)      the handle's product alone and (l), (u) the factor's LOWER / DIAG_UNIT and UPPER / DIAG_STORED solve alone: `steps` calls
           between one pair of events / steps;
  (k13)    bicgstab(tol = 0, max_steps = steps) and
  (jac)    pbicgstab(m = 1 ./ diagonal, tol = 0, max_steps = steps) on the matrix as built, at check_every = 1, 10 and steps;
  (k13c)   bicgstab and
  (ilu)    pbicgstab(first, second = ilu0().plans(), tol = 0, max_steps = plan_steps) on the coalesced matrix, at check_every = 1 and
           plan_steps: the host's clock around the whole call (it returns after a synchronise; workspace allocation, step 0 and the
           history copies included) / the steps the call enqueued (a run whose rr reaches 0 stops early, and says so).
Then, for every case, plain, Jacobi, SGS and ILU(0) to tol = 1e-8 at check_every 1 and 10: steps, reason and the host's clock around
the call (median of `solve-repeats` after one short warm call).
The expectation, derived and written down before the first run (profiles/pbicgstab_measured.txt has it in full): (jac) = (k13) + five
vector passes of 8 n bytes at the 5.2 TB/s of profiles/r01_copy_bandwidth.txt; (ilu) = (k13c) + one pass + 2 (l) + 2 (u); "met" is
within 1.10 x of that sum as measured in the same process.  Development aid only; bench.py is the measured contract.
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
JACOBI_PASSES = 5                # vector passes of a Jacobi step beyond K13's eighteen
PLAN_PASSES = 1                  # ... of a step with plans and no m: shat read by pb_full
STEP_CASES = {"headline": (16763552, 100, 10), "small": (1003, 100, 10)}      # n, steps, steps with plans (rr underflows soon after)
TOL = 1e-8
MAX_STEPS = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,small,memplus,convdiff")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--solve-repeats", type=int, default=1)
    ap.add_argument("--max-steps-plans", type=int, default=MAX_STEPS, help="max_steps of the runs to tolerance that use plans (a step "
                    "with plans on a grid costs hundreds of steps without)")
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import bicgstab_method as bi
    import exp_transposed as xt
    import pbicgstab_method as pb
    import smvp_toolkit_amd as sm
    from exp_ilu0 import coalesce

    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def wall(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = call()[0]
        return (time.perf_counter() - t) * 1e3, r

    def to_tolerance(name, H, b, x):
        """plain, Jacobi, SGS and ILU(0) on the handle H (plain CSR, rows sorted, a diagonal each) to tol = 1e-8."""
        n = H.rows
        d = H.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
        m = torch.reciprocal(d)
        SL, SU = H.trsv_plan(sm.TRSV_LOWER), H.trsv_plan(sm.TRSV_UPPER)
        f = H.ilu0()
        L, U = f.plans()
        say("# %s: SGS solves %d + %d launches (%d + %d levels), ILU(0) solves %d + %d launches; ILU(0) built in %.1f ms" % (
            name, SL.info()["launches"], SU.info()["launches"], SL.info()["levels"], SU.info()["levels"], L.info()["launches"],
            U.info()["launches"], f.info()["build_ms"]))
        forms = (("plain", lambda k, e: H.bicgstab(b, x, max_steps=k, tol=TOL, check_every=e)),
                 ("Jacobi", lambda k, e: H.pbicgstab(b, x, m=m, max_steps=k, tol=TOL, check_every=e)),
                 ("SGS", lambda k, e: H.pbicgstab(b, x, SL, SU, m=d, max_steps=k, tol=TOL, check_every=e)),
                 ("ILU(0)", lambda k, e: H.pbicgstab(b, x, L, U, max_steps=k, tol=TOL, check_every=e)))
        for what, run in forms:
            run(2, 1)                                              # warm: every code object loaded
            for every in (1, 10):                                  # (steps enqueued after the one that stopped run in vain until the next look)
                most = a.max_steps_plans if what in ("SGS", "ILU(0)") else MAX_STEPS
                runs = [wall(lambda: run(most, every)) for _ in range(a.solve_repeats)]
                r, ms = runs[0][1], float(np.median([t for t, _ in runs]))
                say("%-26s to tol %g, check_every %2d: %-7s %5d steps, reason %d, %10.3f ms (median of %d; %.4f ms per step), rr / bb = %.3g" % (
                    name, TOL, every, what, r.steps, r.reason, ms, a.solve_repeats, ms / max(r.steps, 1), r.rr / r.bb if r.bb else 0.0))
        for X in (L, U, f, SL, SU):
            X.close()

    say("# device %s; ms per step; (i) = spmv alone, (l) / (u) = the factor's lower / upper solve alone, by events; (k13) = smvp_csr_bicgstab, "
        "(jac) = smvp_csr_pbicgstab with m = 1 ./ smvp_csr_diagonal, (ilu) = smvp_csr_pbicgstab with ilu0().plans(), all tol 0, host clock "
        "around the call / the steps it enqueued" % (sm.device_info(0)[0],))
    say("# expectation (derived, not measured): (jac) = (k13) + %d vector passes at %.1f TB/s; (ilu) = (k13c) + %d pass + 2 (l) + 2 (u); "
        "met = within 1.10 x" % (JACOBI_PASSES, COPY_TBS, PLAN_PASSES))
    for case in [c for c in a.cases.split(",") if c]:
        t0 = time.time()
        if case in STEP_CASES:
            n, steps, plan_steps = STEP_CASES[case]
            M = bi.nonsym(n)
            name = "nonsym(%d)" % n
            A = sm.CsrMatrix(n, n, *M.csr)
            rp, ci, v = coalesce(n, *M.csr)
            Ac = sm.CsrMatrix(n, n, rp, ci, v)
            nnz, nnz_c = M.nnz, int(rp[-1])
            del M, rp, ci, v
        elif case == "memplus":
            name, n, cols, rp, ci, v = xt.sample("memplus.mtx")
            Ac, nnz_c = sm.CsrMatrix(n, cols, rp, ci, v), int(rp[-1])
        else:
            M = pb.convdiff(1024, 0.5)
            name, n, nnz_c = "convdiff(1024, 0.5)", M.n, M.nnz
            Ac = sm.CsrMatrix(n, n, *M.csr)
            del M
        b = torch.from_numpy(bi.rhs(n)).cuda()
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        if case not in STEP_CASES:
            say("# %s: rows=%d nnz=%d, plan %s; built in %.1f s" % (name, n, nnz_c, Ac.describe()[0][:70], time.time() - t0))
            to_tolerance(name, Ac, b, x)
            Ac.close()
            continue

        m = torch.reciprocal(A.diagonal(torch.empty(n, dtype=torch.float64, device="cuda")))
        f = Ac.ilu0()
        L, U = f.plans()
        everys, plan_everys = sorted({1, 10, steps}), sorted({1, plan_steps})
        say("# %s: nnz=%d (%d coalesced), %d steps (%d with plans), plan %s (%d launches per product); lower solve %d launches (%d chains, %d "
            "levels), upper %d (%d, %d); built in %.1f s" % (name, nnz, nnz_c, steps, plan_steps, A.describe()[0][:70], A.launches(),
                                                             L.info()["launches"], L.info()["chains"], L.info()["levels"], U.info()["launches"],
                                                             U.info()["chains"], U.info()["levels"], time.time() - t0))

        def by_events(call, reps=steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                call()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / reps

        p, q = b.clone(), torch.empty_like(b)
        alone = {"i": lambda: A.spmv(p, q), "ic": lambda: Ac.spmv(p, q), "l": lambda: L.solve(p, q), "u": lambda: U.solve(p, q)}
        forms = {"k13": lambda e: A.bicgstab(b, x, max_steps=steps, tol=0.0, check_every=e),
                 "jac": lambda e: A.pbicgstab(b, x, m=m, max_steps=steps, tol=0.0, check_every=e),
                 "k13c": lambda e: Ac.bicgstab(b, x, max_steps=plan_steps, tol=0.0, check_every=e),
                 "ilu": lambda e: Ac.pbicgstab(b, x, L, U, max_steps=plan_steps, tol=0.0, check_every=e)}

        def library(form, every):
            """ms per step ENQUEUED: a run that stops before its max_steps (rr = 0 at tol 0) still enqueues up to the next look."""
            ms, r = wall(lambda: forms[form](every))
            most = steps if form in ("k13", "jac") else plan_steps
            return ms / max(min(most, -(-r.steps // every) * every), 1), r

        for call in alone.values():                                # warm: every code object loaded, every plan built once
            by_events(call, 10)
        for form in forms:
            bits = None
            for e in (everys if form in ("k13", "jac") else plan_everys):
                r = library(form, e)[1]
                got = x.cpu().numpy().view(np.int64)
                assert bits is None or np.array_equal(bits, got), "d_x depends on check_every"
                bits = got
            say("# %s (%s): the run at tol 0 made %d steps, reason %d" % (name, form, r.steps, r.reason))
        ta = {k: [] for k in alone}
        tf = {form: {e: [] for e in (everys if form in ("k13", "jac") else plan_everys)} for form in forms}
        for rnd in range(a.repeats):
            for k, call in alone.items():
                ta[k].append(by_events(call, steps if k in ("i", "ic") else plan_steps * 2))
            for form in forms:
                for e in tf[form]:
                    tf[form][e].append(library(form, e)[0])
            say("%-18s round %d  (i) %.4f (ic) %.4f (l) %.4f (u) %.4f  " % (name, rnd, ta["i"][-1], ta["ic"][-1], ta["l"][-1], ta["u"][-1]) +
                "  ".join("%s every %d: %.4f" % (form, e, tf[form][e][-1]) for form in forms for e in tf[form]))
        med = {k: float(np.median(v)) for k, v in ta.items()}
        say("%-18s median (i) %.4f (ic) %.4f (l) %.4f (u) %.4f ms" % (name, med["i"], med["ic"], med["l"], med["u"]))
        pass_ms = 8.0 * n / (COPY_TBS * 1e12) * 1e3
        for e in everys:
            c, t = float(np.median(tf["k13"][e])), float(np.median(tf["jac"][e]))
            model = c + JACOBI_PASSES * pass_ms
            say("%-18s median check_every %4d: (k13) %.4f ms/step, spread %.1f %%; (jac) %.4f ms/step, spread %.1f %%; (jac) - (k13) = %.4f "
                "(%.2f x the %.4f ms of %d passes); expected (k13) + passes = %.4f ms: %.2f x (%s)" % (
                    name, e, c, 100 * (max(tf["k13"][e]) - min(tf["k13"][e])) / c, t, 100 * (max(tf["jac"][e]) - min(tf["jac"][e])) / t, t - c,
                    (t - c) / (JACOBI_PASSES * pass_ms), JACOBI_PASSES * pass_ms, JACOBI_PASSES, model, t / model,
                    "met" if t <= 1.10 * model else "MISSED"))
        for e in plan_everys:
            c, t = float(np.median(tf["k13c"][e])), float(np.median(tf["ilu"][e]))
            model = c + PLAN_PASSES * pass_ms + 2 * med["l"] + 2 * med["u"]
            say("%-18s median check_every %4d: (k13c) %.4f ms/step, spread %.1f %%; (ilu) %.4f ms/step, spread %.1f %%; (ilu) / (k13c) = %.2f; "
                "expected (k13c) + %.4f + 2 (l) + 2 (u) = %.4f ms: %.2f x (%s)" % (
                    name, e, c, 100 * (max(tf["k13c"][e]) - min(tf["k13c"][e])) / c, t, 100 * (max(tf["ilu"][e]) - min(tf["ilu"][e])) / t, t / c,
                    PLAN_PASSES * pass_ms, model, t / model, "met" if t <= 1.10 * model else "MISSED"))
        for X in (L, U, f):
            X.close()
        A.close()
        del p, q, m
        torch.cuda.empty_cache()
        to_tolerance(name + ", coalesced", Ac, b, x)
        Ac.close()
        del b, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
