#!/usr/bin/env python3
"""K11 (smvp_csr_power_method) against the iterate + normalize loop of smvp_csr_compute: wall time per step.

    python tools/exp_power_method.py [--cases headline,config4,ibm32] [--repeats 3]

Matrices: memplus x944 (kron(I, memplus) as tools/exp_tiled.py builds it), BASELINE config 4 (synth_csr uniform, 10 M x 10 M,
32 per row, seed 2024) with 100 steps, and ibm32.mtx with 1000 steps, where the launches and not the bytes decide the time.  Per
matrix, after one warm run of each form, `repeats` rounds that alternate
  (a) smvp_csr_compute(iterate, normalize, iters = steps), arrays built on the device: wall_ms of smvp_last_run_info / steps -- the
      timed loop alone (an event pair around every product, no set-up, no allocation);
  (b) power_method(tol = 0, max_steps = steps) on a handle made once, at check_every = 1, 10, 100 (and steps): the host's clock
      around the whole call (it returns after a synchronise; workspace allocation, the start vector's pass and the two history
      copies included) / steps.
Prints every round, the medians and (b) / (a).  Checks that (b)'s last iterate is (a)'s, bit for bit, and that no run stopped
early.  Development aid only; bench.py is the measured contract.
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


def headline():
    import oracle_binding as ob
    import smvp_toolkit_amd as sm
    from exp_tiled import tile_csr

    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path("memplus.mtx"))
    rp, ci, v = sm.csr_from_coo(coo, m)
    copies = (1 << 24) // m
    RP, CI, V = tile_csr(rp, ci, v, m, n, copies)
    return "memplus x%d" % copies, m * copies, RP, CI, V, 100


def config4():
    import smvp_toolkit_amd as sm

    N = 10_000_000
    rp, ci, v = sm.synth_csr(sm.SYNTH_UNIFORM, 2024, N, N, 32, threads=16)
    return "config 4", N, rp, ci, v, 100


def ibm32():
    import oracle_binding as ob
    import smvp_toolkit_amd as sm

    tc, m, n, coo = sm.mm_read_coo(ob.fixture_path("ibm32.mtx"))
    rp, ci, v = sm.csr_from_coo(coo, m)
    return "ibm32", m, rp, ci, v, 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="headline,config4,ibm32")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    import torch
    import smvp_toolkit_amd as sm

    print("# device %s; ms per step; (a) = smvp_csr_compute iterate + normalize, the timed loop's wall_ms / steps; (b) = "
          "smvp_csr_power_method tol 0, host clock around the call / steps" % (sm.device_info(0)[0],), flush=True)
    for case in a.cases.split(","):
        t0 = time.time()
        name, n, rp, ci, v, steps = {"headline": headline, "config4": config4, "ibm32": ibm32}[case]()
        nnz = int(rp[-1])
        coo = sm.coo_from_csr(n, rp, ci, v)
        A = sm.CsrMatrix(n, n, rp, ci, v)
        dx = torch.empty(n, dtype=torch.float64, device="cuda")
        everys = sorted({1, 10, 100, steps})
        print("# %s: n=%d nnz=%d, %d steps, plan %s (%d launches per product), built in %.1f s" % (
            name, n, nnz, steps, A.describe()[0][:70], A.launches(), time.time() - t0), flush=True)

        def loop():
            y, ms, st = sm.csr_compute(coo, n, n, iters=steps, iterate=True, normalize=True, device_convert=True)
            return sm.last_run_info().wall_ms / steps, y, float(np.sum(ms)) / steps

        def power(every):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r, lam, res = A.power_method(None, dx, steps, tol=0.0, check_every=every)
            ms = (time.perf_counter() - t) * 1e3 / steps
            assert r.steps == steps and r.reason == sm.POWER_MAX_STEPS, (r.steps, r.reason)
            return ms, r

        y = loop()[1]                                              # warm: every code object loaded, every plan built once
        for e in everys:
            power(e)
        assert np.array_equal(dx.cpu().numpy().view(np.int64), y.view(np.int64)), "the power method's iterate is not iterate + normalize's"
        ta, tp, tb = [], [], {e: [] for e in everys}
        for rnd in range(a.repeats):
            w, _, p = loop()
            ta.append(w)
            tp.append(p)
            for e in everys:
                tb[e].append(power(e)[0])
            print("%-14s round %d  (a) %.4f (products alone, by events: %.4f)  " % (name, rnd, w, p) +
                  "  ".join("(b) every %d: %.4f" % (e, tb[e][-1]) for e in everys), flush=True)
        ma = float(np.median(ta))
        r = power(everys[-1])[1]
        print("%-14s median (a) %.4f ms/step, spread %.1f %%; products alone %.4f" % (name, ma, 100 * (max(ta) - min(ta)) / ma, float(np.median(tp))))
        for e in everys:
            mb = float(np.median(tb[e]))
            print("%-14s median (b) check_every %4d: %.4f ms/step, spread %.1f %%, (b) / (a) = %.3f" % (
                name, e, mb, 100 * (max(tb[e]) - min(tb[e])) / mb, mb / ma))
        print("%-14s lambda_%d = %.17g at index %d, residual %.3g, scale %.17g; last iterate bit-equal to (a)'s" % (
            name, r.steps, r.eigenvalue, r.index, r.residual, r.scale), flush=True)
        A.close()
        del coo, dx
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
