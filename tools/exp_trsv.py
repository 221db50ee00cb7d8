#!/usr/bin/env python3
"""K15: smvp_trsv_solve against an expectation written down before the first run, against smvp_csr_spmv on the same handle, a
captured graph, scipy on one CPU core and torch's sparse triangular solve.

    python tools/exp_trsv.py [--cases barrier,memplus,pwt,headline,pwt459,spd] [--sweep memplus,pwt] [--out FILE]

Matrices: memplus and pwt (the golden samples), memplus x944 (the headline workload) and pwt x459 (kron(I, A), as tools/exp_tiled.py
builds them), tests/cg_method.py's spd(n) at the headline's row count, and a bidiagonal chain of 4096 rows.  The structures are the
files'; the values are tests/trsv_method.py's `dominant` rule (off-diagonal magnitudes of a row sum to under 1/2, diagonals in [1, 2])
so that every solve stays finite and scipy's answer can be compared.  The lower triangle of each, DIAG_STORED.

The expectation for one solve, derived and not measured: the sum over its launches of max(launch floor, the launch's bytes / 5.2
TB/s), bytes = 12 per entry read + 16 per row + 4 per entry of `order`; the launch floor is the 2.1 us back-to-back host wall per
launch the project measured on ibm32 (README); a chain adds its levels x the per-level barrier step, which `barrier` measures first
on the bidiagonal chain (4096 levels, one launch).  Timing: device events around at least 100 solves after about 40 ms of untimed
ones.  Development aid only; bench.py is the measured contract."""
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
LEVEL_US_GUESS = 2.0    # a chain's per-level step, guessed before anything ran: two dependent loads (col_ind, then val and x) and a barrier


def dominant_values(rows, rp, ci, seed=20300):
    """trsv_method.dominant's rule, vectorised for matrices of 10^8 entries."""
    rng = np.random.default_rng(seed)
    row_of = np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp))
    off = ci[:len(row_of)] != row_of
    per_row = np.bincount(row_of[off], minlength=rows)
    v = rng.uniform(1.0, 2.0, len(row_of))
    v[off] = rng.uniform(-1.0, 1.0, int(off.sum())) * (0.499 / per_row[row_of[off]])
    return row_of, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="barrier,memplus,pwt,headline,pwt459,spd")
    ap.add_argument("--sweep", default="memplus,pwt", help="cases whose chain width is swept over 256 / 512 / 1024")
    ap.add_argument("--level-us", type=float, default=None, help="the per-level step of a chain (default: what `barrier` measures)")
    ap.add_argument("--scipy-limit", type=int, default=200_000_000, help="no scipy run on more entries than this")
    ap.add_argument("--torch-limit", type=int, default=5_000_000, help="no torch sparse triangular solve on more entries than this")
    ap.add_argument("--lanes-by-mean", action="store_true", help="plan option trsv_lanes_by_mean = 1: the lanes of a wide level's row from the mean row length alone")
    ap.add_argument("--out", default=None, help="append the output to this file too")
    a = ap.parse_args()
    import torch
    import cg_method as cg
    import exp_transposed as xt
    import smvp_toolkit_amd as sm
    import trsv_method as tm

    sink = open(a.out, "a") if a.out else None
    if a.lanes_by_mean:
        sm.set_option("trsv_lanes_by_mean", 1)

    def say(line):
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def timed(fn):
        """ms per call: events around at least 100 calls after about 40 ms of untimed ones."""
        one = xt.timed(torch, fn, 3)
        xt.timed(torch, fn, max(3, int(40.0 / max(one, 1e-3))))
        return xt.timed(torch, fn, max(100, int(200.0 / max(one, 1e-3))))

    def bidiagonal():
        n = 4096
        i = np.arange(n)
        M = tm.dominant("bidiagonal(4096)", n, np.concatenate([i[1:], i]), np.concatenate([i[:-1], i]), 20311)
        return ("bidiagonal(4096)", n, n) + M.csr

    def spd():
        M = cg.spd(16763552)
        return ("spd(16763552)", M.n, M.n) + tuple(M.csr)

    builders = dict(xt.CASES, barrier=bidiagonal, spd=spd)
    level_us = a.level_us
    say("# device %s; smvp_trsv_solve, lower triangle, DIAG_STORED; ms per solve by events" % (sm.device_info(0)[0],))
    say("# expectation (derived): sum over launches of max(%.1f us, (12 B per entry + 16 B per row + 4 B per order entry) / %.1f TB/s)"
        " + a chain's levels x the per-level step (guessed %.1f us before the first run; `barrier` measures it)" % (
            LAUNCH_US, COPY_TBS, LEVEL_US_GUESS))
    for case in [c for c in a.cases.split(",") if c]:
        t0 = time.time()
        name, rows, cols, rp, ci, v = builders[case]()
        nnz = int(rp[-1])
        keep_values = case in ("barrier", "spd")                     # dominant already / strictly dominant by construction
        row_of, dv = dominant_values(rows, rp, ci) if not keep_values else (np.repeat(np.arange(rows, dtype=np.int32), np.diff(rp)), v)
        ci, dv = np.ascontiguousarray(ci[:nnz]), np.ascontiguousarray(dv[:nnz], dtype=np.float64)
        in_triangle = np.bincount(row_of[ci <= row_of], minlength=rows)          # entries one solve reads, by row
        A = sm.CsrMatrix(rows, cols, rp, ci, dv)
        b = torch.from_numpy(tm.rhs(rows)).cuda()
        x, y = torch.empty_like(b), torch.empty_like(b)
        widths_of = {}
        for width in ([256] + ([512, 1024] if case in a.sweep.split(",") else [])):
            with sm.option("trsv_chain_width", width):
                P = A.trsv_plan(sm.TRSV_LOWER)
            info = P.info()
            level_ptr, order = P.schedule()
            per_level = np.add.reduceat(in_triangle[order], level_ptr[:-1]) if info["levels"] else np.zeros(0)
            widths = np.diff(level_ptr)
            expect_us, l = 0.0, 0
            while l < info["levels"]:                                            # the launches, as trsv_method.launches counts them
                e = l
                while e < info["levels"] and widths[e] <= info["chain_width"]:
                    e += 1
                chain = e > l
                e = e if chain else l + 1
                nbytes = 12.0 * per_level[l:e].sum() + 20.0 * widths[l:e].sum()
                expect_us += max(LAUNCH_US, nbytes / (COPY_TBS * 1e6)) + ((e - l) * (level_us if level_us is not None else LEVEL_US_GUESS) if chain else 0.0)
                l = e
            P.solve(b, x)
            torch.cuda.synchronize()
            ms = timed(lambda: P.solve(b, x))
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    P.solve(b, y, stream=s)
            torch.cuda.synchronize()
            ms_graph = timed(g.replay)
            assert torch.equal(x.view(torch.int64), y.view(torch.int64)), "the replayed graph gives other bits"
            del g
            if width == 256:
                say("# %s: rows=%d nnz=%d, the triangle holds %d entries (%.2f of the matrix); %d levels, widest %d; %d lanes a row; "
                    "analysed in %.1f ms, plan %.2f MB; built in %.1f s" % (
                        name, rows, nnz, info["entries"], info["entries"] / max(nnz, 1), info["levels"], info["max_level_width"],
                        info["lanes_per_row"], info["build_ms"], info["plan_bytes"] / 1e6, time.time() - t0))
            say("%-18s chain width %4d: %4d launches (%d chains)  solve %.4f ms, from a graph %.4f ms; expected %.4f ms: %.2f x (%s)" % (
                name, info["chain_width"], info["launches"], info["chains"], ms, ms_graph, expect_us / 1e3, ms / (expect_us / 1e3),
                "met" if ms <= 1.5 * expect_us / 1e3 else "missed"))
            widths_of[width] = ms
            if case == "barrier" and level_us is None:
                level_us = ms * 1e3 / info["levels"]
                say("# the per-level step of a chain: %.3f us (%.4f ms / %d levels); used for the chains of every case below" % (
                    level_us, ms, info["levels"]))
            if width != 256:
                P.close()
            else:
                first = P
        ms_spmv = timed(lambda: A.spmv(b, y))
        say("%-18s smvp_csr_spmv on the same handle (%s): %.4f ms; solve / spmv = %.2f" % (
            name, A.describe()[0][:40], ms_spmv, widths_of[256] / ms_spmv))
        first.solve(b, x)
        torch.cuda.synchronize()
        got = x.cpu().numpy()
        try:
            if nnz > a.scipy_limit:
                raise RuntimeError("more than --scipy-limit entries")
            import scipy.sparse as sp
            from scipy.sparse.linalg import spsolve_triangular
            L = sp.tril(sp.csr_matrix((dv, ci, rp[:rows + 1]), shape=(rows, cols)), format="csr")
            L.sum_duplicates()
            hb = b.cpu().numpy()
            t = time.perf_counter()
            want = spsolve_triangular(L, hb, lower=True)
            cpu_ms = (time.perf_counter() - t) * 1e3
            say("%-18s scipy.sparse.linalg.spsolve_triangular, one core: %.1f ms (%.0f x the solve); largest |difference| %.3g" % (
                name, cpu_ms, cpu_ms / widths_of[256], np.abs(want - got).max()))
            del L, want
        except Exception as e:                                                   # noqa: BLE001 -- reported, not hidden
            say("%-18s scipy: not run (%s: %s)" % (name, type(e).__name__, e))
        try:
            if nnz > a.torch_limit:
                raise RuntimeError("more than --torch-limit entries")
            keep = torch.from_numpy(ci <= row_of)
            Lt = torch.sparse_coo_tensor(torch.stack([torch.from_numpy(row_of.astype(np.int64))[keep], torch.from_numpy(ci.astype(np.int64))[keep]]),
                                         torch.from_numpy(dv)[keep], (rows, cols)).coalesce().to_sparse_csr().cuda()
            B = b.reshape(-1, 1).contiguous()
            sol = torch.triangular_solve(B, Lt, upper=False).solution
            torch.cuda.synchronize()
            ms_torch = timed(lambda: torch.triangular_solve(B, Lt, upper=False))
            say("%-18s torch.triangular_solve on a sparse CSR tensor: %.4f ms (%.1f x the solve); largest |difference| %.3g" % (
                name, ms_torch, ms_torch / widths_of[256], float((sol[:, 0] - x).abs().max())))
            del Lt, sol
        except Exception as e:                                                   # noqa: BLE001
            say("%-18s torch.triangular_solve on a sparse CSR tensor: not run (%s: %s)" % (name, type(e).__name__, str(e)[:120]))
        first.close()
        A.close()
        del b, x, y, row_of, dv, ci, rp, v
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
