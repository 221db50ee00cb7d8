#!/usr/bin/env python3
"""K17: smvp_ilu0_factor against an expectation written down before the first run (profiles/ilu0_measured.txt), against the LOWER
/ DIAG_UNIT smvp_trsv_solve on the factor in the same process, and against smvp_csr_ilu0_host on one CPU core; then conjugate
gradients preconditioned with the factor against symmetric Gauss-Seidel, Jacobi and plain CG.

    python tools/exp_ilu0.py [--cases memplus,pwt,headline,pwt459,lap2d,spd] [--solve lap2d,spd] [--out FILE]

Matrices: those of tools/exp_trsv.py -- memplus and pwt (the golden samples), memplus x944 and pwt x459 (kron(I, A)), tests/cg_method.py's
spd(n) at the headline's row count with its repeated entries added up -- and tests/pcg_tri_method.py's lap2d(1024).  The structures
are the files'; the values of the four samples are tests/trsv_method.py's `dominant` rule, under which the factorisation exists.

The expectation for one factorisation, derived and not measured: per launch the larger of the launch floor (2.1 us, README) and
the launch's bytes at 5.2 TB/s (profiles/r01_copy_bandwidth.txt; 8 B read and 8 B written per value, 4 B per column, 12 B per
row, and per pivot one column, one diag_pos, one row_ptr and one u_kk: 20 B); plus, for every level, a serial term of PIVOT_US per
pivot of the level's longest row -- a pivot is a chain of dependent loads (the column, its diag_pos, u_kk), a division, a shuffle
and a binary search, guessed at 1.5 us before anything ran; plus a chain's levels x the per-level step K15 measured (1.16 us).
Pivots and matched updates are counted on the host for matrices of up to --count-limit entries.  Timing: device events around at
least 20 factorisations after about 40 ms of untimed ones.  Development aid only; bench.py is the measured
contract."""
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
LAUNCH_US = 2.1         # README: back-to-back host wall per launch on ibm32
LEVEL_US = 1.16         # profiles/trsv_measured.txt: a chain's per-level step on one-row levels
PIVOT_US = 1.5          # guessed before anything ran: three dependent loads, a division, a shuffle, a binary search


class DeviceDoubles:
    """n doubles at a device address as an object torch.as_tensor can wrap (the CUDA array interface)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def coalesce(rows, rp, ci, v):
    """Repeated (i, j) added up, every row's columns ascending (numpy: for matrices of 10^8 entries)."""
    row_of = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    key = row_of * rows + ci
    order = np.argsort(key, kind="stable")
    key, v = key[order], v[order]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    starts = np.flatnonzero(first)
    val = np.add.reduceat(v, starts)
    r, c = key[starts] // rows, key[starts] % rows
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=rows))]).astype(np.int32), c.astype(np.int32), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="memplus,pwt,headline,pwt459,lap2d")
    ap.add_argument("--solve", default="lap2d", help="cases on which pcg_tri with ILU(0) runs against SGS, Jacobi and plain CG")
    ap.add_argument("--count-limit", type=int, default=2_000_000, help="no host count of matched updates on more entries than this")
    ap.add_argument("--host-limit", type=int, default=200_000_000, help="no smvp_csr_ilu0_host run on more entries than this")
    ap.add_argument("--max-steps", type=int, default=4000)
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import cg_method as cg
    import exp_transposed as xt
    import exp_trsv
    import pcg_tri_method as tri
    import smvp_toolkit_amd as sm
    import trsv_method as tm

    sink = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(fn, least=20):
        one = xt.timed(torch, fn, 2)
        xt.timed(torch, fn, max(2, int(40.0 / max(one, 1e-3))))
        return xt.timed(torch, fn, max(least, int(200.0 / max(one, 1e-3))))

    def lap2d():
        M = tri.lap2d(1024)
        return ("lap2d(1024)", M.n, M.n) + tuple(M.csr)

    def spd():
        M = cg.spd(16763552)
        return ("spd(16763552), coalesced", M.n, M.n) + coalesce(M.n, *M.csr)

    builders = dict(xt.CASES, lap2d=lap2d, spd=spd)
    say("# device %s; smvp_ilu0_factor; ms per factorisation by events" % (sm.device_info(0)[0],))
    say("# expectation (derived): sum over launches of max(%.1f us, bytes / %.1f TB/s) + per level %.2f us x the pivots of its longest row"
        " + a chain's levels x %.2f us" % (LAUNCH_US, COPY_TBS, PIVOT_US, LEVEL_US))
    for case in [c for c in a.cases.split(",") if c]:
        t0 = time.time()
        name, rows, cols, rp, ci, v = builders[case]()
        nnz = int(rp[-1])
        ci = np.ascontiguousarray(ci[:nnz])
        if case in ("lap2d", "spd"):
            row_of, dv = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), np.ascontiguousarray(v[:nnz], dtype=np.float64)
        else:
            row_of, dv = exp_trsv.dominant_values(rows, rp, ci)
        pivots_of = np.bincount(row_of[ci < row_of], minlength=rows)
        lens = np.diff(rp)
        A = sm.CsrMatrix(rows, cols, rp, ci, dv)
        f = A.ilu0()
        info = f.info()
        L, U = f.plans()
        li = L.info()
        level_ptr, order = L.schedule()
        widths = np.diff(level_ptr)
        longest = np.maximum.reduceat(pivots_of[order], level_ptr[:-1]) if info["levels"] else np.zeros(0)
        per_level = (np.add.reduceat((28.0 * lens + 20.0 * pivots_of + 12.0)[order], level_ptr[:-1]) if info["levels"] else np.zeros(0))
        expect_us, l = 0.0, 0
        while l < info["levels"]:
            e = l
            while e < info["levels"] and widths[e] <= info["chain_width"]:
                e += 1
            chain = e > l
            e = e if chain else l + 1
            expect_us += max(LAUNCH_US, per_level[l:e].sum() / (COPY_TBS * 1e6)) + PIVOT_US * longest[l:e].sum() + (LEVEL_US * (e - l) if chain else 0.0)
            l = e
        ms = timed(lambda: f.factor())
        b = torch.from_numpy(tm.rhs(rows)).cuda()
        x = torch.empty_like(b)
        ms_solve = timed(lambda: L.solve(b, x), 100)
        say("# %s: rows=%d nnz=%d pivots=%d; %d levels, widest %d; longest row %d, most pivots in a row %d; %d lanes a row; create %.1f ms "
            "(smvp_csr_trsv_create on F: %.1f ms), owns %.2f MB; built in %.1f s" % (
                name, rows, nnz, info["pivots"], info["levels"], info["max_level_width"], lens.max(), pivots_of.max(), info["lanes_per_row"],
                info["build_ms"], li["build_ms"], info["plan_bytes"] / 1e6, time.time() - t0))
        say("%-18s %4d launches (%d chains)  factor %.4f ms; expected %.4f ms: %.2f x (%s); LOWER / UNIT solve on F, same launches: %.4f ms, "
            "factor / solve = %.1f" % (name, info["launches"], info["chains"], ms, expect_us / 1e3, ms / (expect_us / 1e3),
                                        "met" if ms <= 1.5 * expect_us / 1e3 else "missed", ms_solve, ms / ms_solve))
        if nnz <= a.host_limit:
            t = time.perf_counter()
            want = sm.ilu0_host(rows, rp, ci, dv)
            cpu_ms = (time.perf_counter() - t) * 1e3
            rp_d, ci_d, v_d = f.matrix.device_arrays()
            got = torch.as_tensor(DeviceDoubles(v_d, nnz), device="cuda").cpu().numpy()
            same = bool(((got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))).all())
            say("%-18s smvp_csr_ilu0_host, one core: %.1f ms (%.1f x the factorisation); every bit the same: %s" % (name, cpu_ms, cpu_ms / ms, same))
            del want, got
        if case in a.solve.split(","):
            dx = torch.empty_like(b)
            db = torch.from_numpy(cg.rhs(rows)).cuda()
            dm = A.diagonal(torch.empty(rows, dtype=torch.float64, device="cuda"))
            SL, SU = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)
            runs = (("pcg_tri, ILU(0)", lambda: A.pcg_tri(db, dx, L, U, max_steps=a.max_steps, tol=1e-8, check_every=1)),
                    ("pcg_tri, SGS", lambda: A.pcg_tri(db, dx, SL, SU, m=dm, max_steps=a.max_steps, tol=1e-8, check_every=1)),
                    ("pcg, Jacobi", lambda: A.pcg(db, dx, dm, max_steps=a.max_steps, tol=1e-8, check_every=1)),
                    ("cg", lambda: A.cg(db, dx, max_steps=a.max_steps, tol=1e-8, check_every=1)))
            for what, run in runs:
                run()
                torch.cuda.synchronize()
                t = time.perf_counter()
                r = run()[0]
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t) * 1e3
                say("%-18s %-16s tol 1e-8, check_every 1: %5d steps, reason %d, %.2f ms (%.4f ms a step)" % (
                    name, what, r.steps, r.reason, wall, wall / max(r.steps, 1)))
            SL.close()
            SU.close()
        for X in (L, U, f, A):
            X.close()
        del b, x, row_of, dv, ci, rp, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
