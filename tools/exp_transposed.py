#!/usr/bin/env python3
"""The transposed product y = A^T x by both routes, against what they stand beside.

    python tools/exp_transposed.py [--cases headline,pwt459,config4,memplus,pwt,ibm32] [--window 0.3] [--repeats 3]
                                   [--host-route headline,memplus,pwt] [--only k8]

Matrices: memplus x944 and pwt x459 (kron(I, A) as tools/exp_tiled.py builds it), BASELINE config 4 (synth_csr uniform,
10 M x 10 M, 32 per row) and the reference's own inputs (x stays in cache).  Per matrix, in one process, the variants
alternated window by window, `repeats` windows of at least `window` seconds each, device events:

    K8        smvp_tjds_spmv_transposed on the TJDS handle (built by smvp_tjds_from_coo_device)
    forward   the default smvp_tjds_spmv on the SAME handle (A x: what the format's own product costs)
    At        smvp_csr_spmv on the handle smvp_csr_create_transposed made
    At(host)  smvp_csr_spmv on a handle smvp_csr_create made from the same transposed arrays in host memory (what a caller
              of the parent commit ends up with); kernel, description and plan bytes must equal At's

and the time of smvp_csr_create_transposed itself (three calls); with --host-route also the parent commit's route on the
host: smvp_coo_from_csr + swap + smvp_csr_from_coo + smvp_csr_create, once.  Prints ms per product of every window, the
share of 8 TB/s by algorithmic bytes and, for K8, gathers per second (one gather of x per entry).  --only k8 runs K8 alone
(for a profiler pass that should see one kernel).  Development aid only; bench.py is the measured contract.
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


def sample(name, copies=1):
    import oracle_binding as ob
    import smvp_toolkit_amd as sm
    from exp_tiled import tile_csr

    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
    rp, ci, v = sm.csr_from_coo(coo, m)
    if copies > 1:
        rp, ci, v = tile_csr(rp, ci, v, m, n, copies)
    return "%s x%d" % (name[:-4], copies) if copies > 1 else name[:-4], m * copies, n * copies, rp, ci, v


def config4():
    import smvp_toolkit_amd as sm

    N = 10_000_000
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 12345, N, N, 32)
    return "config 4", N, N, rp, ci, v


CASES = {"headline": lambda: sample("memplus.mtx", 944), "pwt459": lambda: sample("pwt.mtx", 459), "config4": config4,
         "memplus": lambda: sample("memplus.mtx"), "pwt": lambda: sample("pwt.mtx"), "ibm32": lambda: sample("ibm32.mtx")}


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def device_coo(torch, rows, d_rp, d_ci, d_v, nnz):
    buf = torch.zeros(16 * max(nnz, 1), dtype=torch.uint8, device="cuda")
    i32, f64 = buf.view(torch.int32).view(-1, 4), buf.view(torch.float64).view(-1, 2)
    lens = (d_rp[1:] - d_rp[:-1]).to(torch.int64)
    i32[:nnz, 0] = torch.repeat_interleave(torch.arange(rows, dtype=torch.int32, device="cuda"), lens)
    i32[:nnz, 1] = d_ci[:nnz]
    f64[:nnz, 1] = d_v[:nnz]
    return buf


class Raw:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,pwt459,config4,memplus,pwt,ibm32")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of products per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-route", default="", help="cases on which the host transposition of the parent commit is timed too")
    ap.add_argument("--only", default="", help="k8: run that variant alone")
    a = ap.parse_args()
    import torch
    import smvp_toolkit_amd as sm

    print("# device %s; window >= %.2f s, %d windows per variant, variants alternated" % (sm.device_info(0)[0], a.window, a.repeats),
          flush=True)
    for case in a.cases.split(","):
        name, rows, cols, rp, ci, v = CASES[case]()
        nnz = int(rp[-1])
        dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        d_rp, d_ci, d_v = dev(rp), dev(ci), dev(v)
        A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_v)
        d_coo = device_coo(torch, rows, d_rp, d_ci, d_v, nnz)
        T = sm.TjdsMatrix(sm.tjds_from_coo_device(d_coo, rows, cols, nnz))
        del d_coo
        gen = torch.Generator(device="cuda")
        gen.manual_seed(2025)
        x_rows = torch.rand(rows, dtype=torch.float64, device="cuda", generator=gen)
        x_cols = torch.rand(cols, dtype=torch.float64, device="cuda", generator=gen)
        y_rows = torch.empty(rows, dtype=torch.float64, device="cuda")
        y_cols = torch.empty(cols, dtype=torch.float64, device="cuda")
        T.set_x(x_cols)
        variants = {"K8": lambda: T.spmv_transposed(x_rows, y_cols), "forward": lambda: T.spmv(y_rows)}
        alg = {"K8": T.transposed_describe()[1], "forward": T.describe()[1]}
        print("# %s: rows=%d cols=%d nnz=%d diagonals=%d; K8 = %s, forward = %s" % (name, rows, cols, nnz, T._t.num_diag,
                                                                                    T.transposed_describe()[0], T.describe()[0]), flush=True)
        if a.only != "k8":
            # smvp_csr_create_transposed, three calls (the last one is kept)
            ms_create = []
            At = None
            for _ in range(3):
                if At is not None:
                    At.close()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                At = A.transposed()
                ms_create.append((time.perf_counter() - t0) * 1e3)
            p = At.device_arrays()
            t_arrays = [torch.as_tensor(Raw(p[0], cols + 1, "<i4"), device="cuda").cpu().numpy().copy(),
                        torch.as_tensor(Raw(p[1], nnz, "<i4"), device="cuda").cpu().numpy().copy(),
                        torch.as_tensor(Raw(p[2], nnz, "<f8"), device="cuda").cpu().numpy().copy()]
            Ah = sm.CsrMatrix(cols, rows, *t_arrays)
            same = (At.get_kernel() == Ah.get_kernel() and At.describe() == Ah.describe()
                    and At.plan_info()["plan_bytes"] == Ah.plan_info()["plan_bytes"])
            print("# %s: smvp_csr_create_transposed %s ms; transposed handle runs %s, plan %.0f bytes; same kernel / description / plan "
                  "bytes as the handle made from host arrays: %s" % (name, " ".join("%.1f" % t for t in ms_create), At.describe()[0],
                                                                     At.plan_info()["plan_bytes"], same), flush=True)
            assert same
            if case in a.host_route.split(","):
                t0 = time.perf_counter()
                coo = sm.coo_from_csr(rows, rp, ci, v)
                sw = sm.make_coo(coo["col"], coo["row"], coo["val"])
                hrp, hci, hv = sm.csr_from_coo(sw, cols)
                t1 = time.perf_counter()
                H = sm.CsrMatrix(cols, rows, hrp, hci, hv)
                t2 = time.perf_counter()
                ok = all(np.array_equal(g, w) for g, w in zip(t_arrays, (hrp, hci, hv)))
                H.close()
                print("# %s: host route (coo_from_csr + swap + csr_from_coo) %.0f ms + smvp_csr_create %.0f ms = %.0f ms, arrays equal "
                      "the device route's: %s; ratio to smvp_csr_create_transposed (median) %.0f x"
                      % (name, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t2 - t0) * 1e3, ok, (t2 - t0) * 1e3 / float(np.median(ms_create))),
                      flush=True)
                del coo, sw, hrp, hci, hv
            variants["At"] = lambda: At.spmv(x_rows, y_cols)
            variants["At(host)"] = lambda: Ah.spmv(x_rows, y_cols)
            alg["At"] = alg["At(host)"] = At.describe()[1]
        if a.only == "k8":
            variants = {"K8": variants["K8"]}
        reps = {}
        for k, fn in variants.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[k] = max(1, int(a.window / max(timed(torch, fn, 2) * 1e-3, 1e-6)) + 1)
        ms = {k: [] for k in variants}
        for _ in range(a.repeats):
            for k, fn in variants.items():
                ms[k].append(timed(torch, fn, reps[k]))
        print("%-14s %-9s %-30s %9s %8s %11s" % ("matrix", "variant", "ms per product, every window", "median", "% 8TB/s", "G gathers/s"),
              flush=True)
        for k in variants:
            med = float(np.median(ms[k]))
            print("%-14s %-9s %-30s %9.4f %8.1f %11s" % (name, k, " ".join("%.4f" % t for t in ms[k]), med,
                                                        alg[k] / (med * 1e-3) / 8e12 * 100,
                                                        "%.1f" % (nnz / (med * 1e-3) * 1e-9) if k == "K8" else "-"), flush=True)
        T.close()
        A.close()
        if a.only != "k8":
            At.close()
            Ah.close()
        del d_rp, d_ci, d_v, x_rows, x_cols, y_rows, y_cols
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
