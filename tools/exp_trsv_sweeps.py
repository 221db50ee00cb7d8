#!/usr/bin/env python3
"""K21: triangular solves by Jacobi sweeps (smvp_csr_trsv_create_sweeps) against the exact, level-scheduled plans of K15 -- one solve,
and time and steps to tol = 1e-8 inside the solvers that take plans.

    python tools/exp_trsv_sweeps.py [--part solve,tol] [--cases lap2d,spd,pwt459,headline,convdiff,memplus] [--exact-every 10]
                                    [--max-steps 4000] [--out FILE]

Part `solve`: one solve of the lower triangle, DIAG_STORED, with 0, 1, 2, 3, 4 and 8 sweeps against the exact plan of the same handle
in the same process, by device events.  Matrices: tests/pcg_tri_method.py's lap2d(1024), tests/cg_method.py's spd(n) at the headline's
row count, pwt x459 and memplus x944 (kron(I, A), values by tests/trsv_method.py's `dominant` rule, as tools/exp_trsv.py builds them).

Part `tol`: the host's clock around the whole call and the steps to tol = 1e-8 at check_every 1 and 10, with plans of 1, 2, 3 and 4
sweeps and the exact plans (the exact plans at --exact-every only: a step with them on a grid costs hundreds of plain ones), against
Jacobi (pcg / pbicgstab with m) and the plain solver: pcg_tri with SGS and with ILU(0) on lap2d(1024) and spd (its repeated entries
added up by tools/exp_ilu0.py's coalesce, which an ILU(0) needs); pbicgstab and gmres(30)
with ILU(0) on tests/pbicgstab_method.py's convdiff(1024, 0.5); pbicgstab with ILU(0) on memplus with its own values, which is not
diagonally dominant.

The expectation for one solve, derived and written down before the first run: sweeps + 1 launches, each the larger of the 2.1 us
launch floor (profiles/trsv_measured.txt) and its bytes at the 5.2 TB/s of profiles/r01_copy_bandwidth.txt.  A sweep's bytes: 12 per
entry inside the ranges (col_ind and val), 8 of bounds, 8 of b and 8 written per row, and the gathered x counted once per row of x (8
n); launch 0 reads no x and no val but the diagonal's: 4 per entry, 8 per row of val, and the same 24 per row.  "met" is within 1.5 x,
tools/exp_trsv.py's margin.  Nothing is gated.  Development aid only; bench.py is the measured contract."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "smvp-toolkit_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COPY_TBS = 5.2          # profiles/r01_copy_bandwidth.txt
LAUNCH_US = 2.1         # profiles/trsv_measured.txt: back-to-back host wall per launch
SWEEPS_SOLVE = (0, 1, 2, 3, 4, 8)
SWEEPS_TOL = (1, 2, 3, 4)
TOL = 1e-8
HEADLINE_ROWS = 16763552


def expected_us(n, entries, sweeps):
    first = max(LAUNCH_US, (4.0 * entries + 32.0 * n) / (COPY_TBS * 1e6))
    each = max(LAUNCH_US, (12.0 * entries + 32.0 * n) / (COPY_TBS * 1e6))
    return first + sweeps * each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="solve,tol")
    ap.add_argument("--cases", default="lap2d,spd,pwt459,headline,convdiff,memplus")
    ap.add_argument("--exact-every", type=int, default=10, help="the one check_every at which the exact plans run to tolerance (0: not at all)")
    ap.add_argument("--max-steps", type=int, default=4000)
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import cg_method as cg
    import exp_transposed as xt
    import pbicgstab_method as pb
    import pcg_tri_method as tri
    import smvp_toolkit_amd as sm
    import trsv_method as tm
    from exp_trsv import dominant_values

    sink = open(a.out, "a") if a.out else None
    parts, cases = a.part.split(","), [c for c in a.cases.split(",") if c]

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(fn):
        """ms per call: events around at least 100 calls after about 40 ms of untimed ones (fewer where one call takes long)."""
        one = xt.timed(torch, fn, 3)
        xt.timed(torch, fn, max(3, int(40.0 / max(one, 1e-3))))
        return xt.timed(torch, fn, max(5, min(100, int(400.0 / max(one, 1e-3)))))

    def wall(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = call()[0]
        return (time.perf_counter() - t) * 1e3, r

    def build(case):
        """(name, n, row_ptr, col_ind, val, the values are the matrix's own)"""
        if case == "lap2d":
            M = tri.lap2d(1024)
            return ("lap2d(1024)", M.n) + tuple(M.csr) + (True,)
        if case == "spd":
            M = cg.spd(HEADLINE_ROWS)
            return ("spd(%d)" % M.n, M.n) + tuple(M.csr) + (True,)
        if case == "convdiff":
            M = pb.convdiff(1024, 0.5)
            return ("convdiff(1024, 0.5)", M.n) + tuple(M.csr) + (True,)
        name, rows, cols, rp, ci, v = xt.CASES[case]()
        return name, rows, rp, ci, v, case == "memplus"

    say("# device %s; K21, smvp_csr_trsv_create_sweeps" % (sm.device_info(0)[0],))
    say("# expectation for one solve (derived, written before the first run): launch 0 = max(%.1f us, (4 B per entry in the ranges + 32 B per "
        "row) / %.1f TB/s), every sweep = max(%.1f us, (12 B per entry + 32 B per row) / %.1f TB/s); met = within 1.5 x" % (
            LAUNCH_US, COPY_TBS, LAUNCH_US, COPY_TBS))
    for case in cases:
        t0 = time.time()
        name, n, rp, ci, v, own = build(case)
        nnz = int(rp[-1])
        ci = np.ascontiguousarray(ci[:nnz])
        v = np.ascontiguousarray(v[:nnz], dtype=np.float64) if own else np.ascontiguousarray(dominant_values(n, rp, ci)[1][:nnz])
        A = sm.CsrMatrix(n, n, rp, ci, v)
        b = torch.from_numpy(tm.rhs(n)).cuda()
        x = torch.empty_like(b)
        say("# %s: rows=%d nnz=%d, plan %s; built in %.1f s" % (name, n, nnz, A.describe()[0][:60], time.time() - t0))
        if "solve" in parts and case in ("lap2d", "spd", "pwt459", "headline"):
            E = A.trsv_plan(sm.TRSV_LOWER)
            ie = E.info()
            ms_exact = timed(lambda: E.solve(b, x))
            say("%-20s exact plan: %d levels, %d launches (%d chains), %d entries, %d lanes a row: %.4f ms a solve" % (
                name, ie["levels"], ie["launches"], ie["chains"], ie["entries"], ie["lanes_per_row"], ms_exact))
            E.close()
            for s in SWEEPS_SOLVE:
                P = A.trsv_plan(sm.TRSV_LOWER, sweeps=s)
                i = P.info()
                ms = timed(lambda: P.solve(b, x))
                want = expected_us(n, i["entries"], s) / 1e3
                say("%-20s %d sweeps: %d launches, %d entries in the ranges, %d lanes a row, plan %.1f MB built in %.0f ms: %.4f ms a solve "
                    "(%.4f a launch), exact / this = %.1f; expected %.4f ms: %.2f x (%s)" % (
                        name, s, i["launches"], i["entries"], i["lanes_per_row"], i["plan_bytes"] / 1e6, i["build_ms"], ms, ms / (s + 1),
                        ms_exact / ms, want, ms / want, "met" if ms <= 1.5 * want else "MISSED"))
                P.close()
        if "tol" in parts and case in ("lap2d", "spd", "convdiff", "memplus"):
            if case == "spd":                                      # an ILU(0) needs every (i, j) once: the repeats added up, as tools/exp_pbicgstab.py does
                from exp_ilu0 import coalesce
                A.close()
                rp, ci, v = coalesce(n, rp, ci, v)
                A = sm.CsrMatrix(n, n, rp, ci, v)
                say("# %s, coalesced: nnz=%d" % (name, int(rp[-1])))
            d = A.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
            f = A.ilu0()
            symmetric = case in ("lap2d", "spd")
            if symmetric:
                solvers = [("pcg_tri", lambda P, k, e: A.pcg_tri(b, x, P[0], P[1], m=P[2], max_steps=k, tol=TOL, check_every=e))]
                base = [("cg", lambda k, e: A.cg(b, x, max_steps=k, tol=TOL, check_every=e)),
                        ("pcg, Jacobi", lambda k, e: A.pcg(b, x, d, max_steps=k, tol=TOL, check_every=e))]
                kinds = ("SGS", "ILU(0)")
            else:
                r = torch.reciprocal(d)
                solvers = [("pbicgstab", lambda P, k, e: A.pbicgstab(b, x, P[0], P[1], m=P[2], max_steps=k, tol=TOL, check_every=e))]
                base = [("bicgstab", lambda k, e: A.bicgstab(b, x, max_steps=k, tol=TOL, check_every=e)),
                        ("pbicgstab, Jacobi", lambda k, e: A.pbicgstab(b, x, m=r, max_steps=k, tol=TOL, check_every=e))]
                if case == "convdiff":
                    solvers.append(("gmres(30)", lambda P, k, e: A.gmres(b, x, P[0], P[1], m=P[2], restart=30, max_steps=k, tol=TOL, check_every=e)))
                    base += [("gmres(30)", lambda k, e: A.gmres(b, x, restart=30, max_steps=k, tol=TOL, check_every=e)),
                             ("gmres(30), Jacobi", lambda k, e: A.gmres(b, x, m=r, restart=30, max_steps=k, tol=TOL, check_every=e))]
                kinds = ("ILU(0)",)

            def report(what, every, ms, r):
                say("%-20s to tol %g, check_every %2d: %-34s %5d steps, reason %d, %11.3f ms (%.4f ms a step), rr / bb = %.3g" % (
                    name, TOL, every, what, r.steps, r.reason, ms, ms / max(r.steps, 1), r.rr / r.bb if r.bb else 0.0))

            for what, run in base:
                run(2, 1)
                for every in (1, 10):
                    report(what, every, *wall(lambda: run(a.max_steps, every)))
            for kind in kinds:
                for sweeps in SWEEPS_TOL + (None,):
                    if kind == "SGS":
                        P = (A.trsv_plan(sm.TRSV_LOWER, sweeps=sweeps), A.trsv_plan(sm.TRSV_UPPER, sweeps=sweeps), d)
                    else:
                        P = f.plans(sweeps=sweeps) + (None,)
                    for solver, run in solvers:
                        run(P, 2, 1)
                        for every in ((1, 10) if sweeps is not None else tuple(e for e in (a.exact_every,) if e)):
                            report("%s, %s, %s" % (solver, kind, "exact plans" if sweeps is None else "%d sweeps" % sweeps), every,
                                   *wall(lambda: run(P, a.max_steps, every)))
                    P[0].close()
                    P[1].close()
            f.close()
        A.close()
        del b, x, rp, ci, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
