#!/usr/bin/env python3
"""K23: the multicolour reordering (smvp_csr_color, smvp_perm_from_classes, smvp_csr_create_permuted) -- what it costs, what it does
to the levels of the triangular plans and of ILU(0), to one exact solve, to the product, and to time and steps to tol = 1e-8 inside
the solvers that take plans.

    python tools/exp_multicolor.py [--part build,tol] [--cases lap2d,convdiff,spd,pwt459,headline,memplus] [--max-steps 4000]
                                   [--sweeps 2] [--natural-max-steps 200] [--out FILE]

Part `build`: colouring time, colours, rounds; perm_from_classes and create_permuted against create_transposed on the same matrix;
levels of LOWER / UPPER before and after; one exact solve (LOWER, DIAG_STORED) and one ILU(0) factorisation on B against A, in the
same process by device events; the product on B against A and what AUTO picks.  Matrices as tools/exp_trsv_sweeps.py builds them:
lap2d(1024), convdiff(1024, 0.5), spd at the headline's row count, pwt x459 (coloured with its transposed handle: it stores one
triangle) and memplus x944 with trsv_method.dominant values.

Part `tol`: the host's clock around the whole call and the steps to tol = 1e-8 at check_every 10 -- the reordered system with exact
plans against the natural order with exact plans (stopped at --natural-max-steps: a step costs one launch per level, and
profiles/trsv_sweeps_measured.txt has their runs to tol), with K21's sweeps and unpreconditioned: pcg_tri and gmres(30) on
lap2d(1024), pbicgstab and gmres(30) on convdiff(1024, 0.5), pbicgstab on memplus with its own values.  The reordered runs include
neither the colouring nor the gathers of b and x (the build part gives those).

The expectation, derived and written down before the first run of this tool: a round of the colouring is the larger of the 2.1 us
launch floor (profiles/trsv_measured.txt) plus the host's read of the counter, and the round's bytes at the 5.2 TB/s of
profiles/r01_copy_bandwidth.txt -- 4 B of col_ind and 4 B of gathered colour per stored entry, 12 B per row (two row_ptr words,
the vertex's own colour); create_permuted costs what create_transposed costs on the same matrix (the same pipeline).  "met" is
within 1.5 x.  Nothing is gated.  Development aid only; bench.py is the measured contract."""
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
HOST_READ_US = 10.0     # a stream synchronise and a 4-byte copy back: the order of a looked step of the solvers (profiles/cg_measured.txt)
TOL = 1e-8
HEADLINE_ROWS = 16763552


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="build,tol")
    ap.add_argument("--cases", default="lap2d,convdiff,spd,pwt459,headline,memplus")
    ap.add_argument("--max-steps", type=int, default=4000)
    ap.add_argument("--sweeps", type=int, default=2, help="K21's sweeps in the natural order, for the comparison")
    ap.add_argument("--natural-max-steps", type=int, default=200,
                    help="the natural order's exact plans stop here (a step costs one launch per level: profiles/trsv_sweeps_measured.txt has their runs to tol)")
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
        one = xt.timed(torch, fn, 2)
        return xt.timed(torch, fn, max(3, min(100, int(300.0 / max(one, 1e-3)))))

    def wall(call):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def build(case):
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

    say("# device %s; K23, the multicolour reordering" % (sm.device_info(0)[0],))
    say("# expectation (derived, written before the first run): a round = max(%.1f us launch + %.0f us host read, (8 B per entry + 12 B per row) "
        "/ %.1f TB/s); create_permuted = create_transposed on the same matrix; met = within 1.5 x" % (LAUNCH_US, HOST_READ_US, COPY_TBS))
    for case in cases:
        t0 = time.time()
        name, n, rp, ci, v, own = build(case)
        nnz = int(rp[-1])
        ci = np.ascontiguousarray(ci[:nnz])
        v = np.ascontiguousarray(v[:nnz], dtype=np.float64) if own else np.ascontiguousarray(dominant_values(n, rp, ci)[1][:nnz])
        A = sm.CsrMatrix(n, n, rp, ci, v)
        say("# %s: rows=%d nnz=%d, plan %s; built in %.1f s" % (name, n, nnz, A.describe()[0][:60], time.time() - t0))
        ms_t, At = wall(lambda: A.transposed())
        use_at = case in ("pwt459",)
        color = torch.empty(n, dtype=torch.int32, device="cuda")
        A.color(color, At if use_at else None)                                  # (untimed first call)
        info = A.color(color, At if use_at else None)
        want_us = max(LAUNCH_US + HOST_READ_US, (8.0 * info["entries"] + 12.0 * n) / (COPY_TBS * 1e6))
        say("%-20s colouring%s: %d colours (classes of %d .. %d rows) in %d rounds, %d lanes a row, %.3f ms = %.1f us a round; expected %.1f us "
            "a FULL round: %.2f x (%s)" % (name, " with at" if use_at else "", info["colors"], info["smallest_class"], info["largest_class"],
                                           info["rounds"], info["lanes_per_row"], info["build_ms"], 1e3 * info["build_ms"] / max(info["rounds"], 1),
                                           want_us, 1e3 * info["build_ms"] / max(info["rounds"], 1) / want_us,
                                           "met" if 1e3 * info["build_ms"] / max(info["rounds"], 1) <= 1.5 * want_us else "MISSED"))
        ms_p, perm = wall(lambda: sm.perm_from_classes(color, info["colors"]))
        old_of_new, new_of_old, color_ptr = perm
        ms_b, B = wall(lambda: A.permuted(new_of_old))
        say("%-20s perm_from_classes %.2f ms; create_permuted %.1f ms against create_transposed %.1f ms: %.2f x (%s); B's plan %s" % (
            name, ms_p, ms_b, ms_t, ms_b / ms_t, "met" if ms_b <= 1.5 * ms_t else "MISSED", B.describe()[0][:60]))
        At.close()
        b = torch.from_numpy(tm.rhs(n)).cuda()
        bn, x, xn = torch.empty_like(b), torch.empty_like(b), torch.empty_like(b)
        ms_g = timed(lambda: sm.vector_gather(old_of_new, b, bn))
        pa, pb_ = timed(lambda: A.spmv(b, x)), timed(lambda: B.spmv(bn, xn))
        say("%-20s vector_gather %.4f ms; product on A %.4f ms, on B %.4f ms: B / A = %.2f" % (name, ms_g, pa, pb_, pb_ / pa))
        if "build" in parts:
            for uplo, un in ((sm.TRSV_LOWER, "LOWER"), (sm.TRSV_UPPER, "UPPER")):
                Ta, Tb = A.trsv_plan(uplo), B.trsv_plan(uplo)
                ia, ib = Ta.info(), Tb.info()
                line = "%-20s %s: levels %d -> %d, launches %d -> %d" % (name, un, ia["levels"], ib["levels"], ia["launches"], ib["launches"])
                if uplo == sm.TRSV_LOWER:
                    sa, sb = timed(lambda: Ta.solve(b, x)), timed(lambda: Tb.solve(bn, xn))
                    line += "; one exact solve %.4f ms -> %.4f ms: %.1f x" % (sa, sb, sa / sb)
                say(line)
                Ta.close()
                Tb.close()
            try:
                fa, fb = A.ilu0(), B.ilu0()
                ia, ib = fa.info(), fb.info()
                ta, tb = timed(lambda: fa.factor()), timed(lambda: fb.factor())
                say("%-20s ILU(0): levels %d -> %d, launches %d -> %d, one factorisation %.4f ms -> %.4f ms: %.1f x" % (
                    name, ia["levels"], ib["levels"], ia["launches"], ib["launches"], ta, tb, ta / tb))
                fa.close()
                fb.close()
            except sm.SmvpError as e:
                say("%-20s ILU(0): not on this matrix (%s)" % (name, str(e)[-80:]))
        if "tol" in parts and case in ("lap2d", "convdiff", "memplus"):
            def report(what, ms, r):
                r = r[0]
                say("%-20s to tol %g: %-46s %5d steps, reason %d, %11.3f ms (%.4f ms a step), rr / bb = %.3g" % (
                    name, TOL, what, r.steps, r.reason, ms, ms / max(r.steps, 1), r.rr / r.bb if r.bb else 0.0))

            k = a.max_steps
            solvers = []
            if case == "lap2d":
                solvers.append(("pcg_tri", lambda H, P, rhs, out, k: H.pcg_tri(rhs, out, P[0], P[1], m=P[2], max_steps=k, tol=TOL)))
                report("cg", *wall(lambda: A.cg(b, x, max_steps=k, tol=TOL)))
            else:
                solvers.append(("pbicgstab", lambda H, P, rhs, out, k: H.pbicgstab(rhs, out, P[0], P[1], m=P[2], max_steps=k, tol=TOL)))
                report("bicgstab", *wall(lambda: A.bicgstab(b, x, max_steps=k, tol=TOL)))
            if case != "memplus":
                solvers.append(("gmres(30)", lambda H, P, rhs, out, k: H.gmres(rhs, out, P[0], P[1], m=P[2], restart=30, max_steps=k, tol=TOL)))
                report("gmres(30)", *wall(lambda: A.gmres(b, x, restart=30, max_steps=k, tol=TOL)))
            for order, H, rhs, out in (("natural", A, b, x), ("multicolour", B, bn, xn)):
                d = H.diagonal(torch.empty(n, dtype=torch.float64, device="cuda"))
                f = H.ilu0()
                for kind in ("SGS", "ILU(0)"):
                    for sweeps in ((None, a.sweeps) if order == "natural" else (None,)):
                        if kind == "SGS":
                            P = (H.trsv_plan(sm.TRSV_LOWER, sweeps=sweeps), H.trsv_plan(sm.TRSV_UPPER, sweeps=sweeps), d)
                        else:
                            P = f.plans(sweeps=sweeps) + (None,)
                        cap = min(k, a.natural_max_steps) if order == "natural" and sweeps is None else k
                        for solver, run in solvers:
                            run(H, P, rhs, out, 2)                              # (untimed first call)
                            report("%s, %s, %s, %s" % (solver, kind, order, "exact plans" if sweeps is None else "%d sweeps" % sweeps),
                                   *wall(lambda: run(H, P, rhs, out, cap)))
                        P[0].close()
                        P[1].close()
                f.close()
        B.close()
        A.close()
        del b, x, bn, xn, rp, ci, v, color, old_of_new, new_of_old
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
