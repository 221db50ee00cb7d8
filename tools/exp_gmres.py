#!/usr/bin/env python3
"""K19 measured: one GMRES(30) cycle on banded(n) -- smvp_csr_gmres(restart = 30, tol = 0, max_steps = 30, check_every = 30) -- timed
with events, and the yardstick of the code before K19: the only way to the same coefficients there was one smvp_vector_dot per
basis vector (the dot kernel, its fold and a host read each) and one axpy-sized pass per basis vector.

  python tools/exp_gmres.py time  [--n N] [--runs R]    median ms of the whole call over R runs, and the yardstick at j = 30
  python tools/exp_gmres.py cycle [--n N]               one warm-up call and one call, nothing else: the process to run under
                                                        `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/exp_gmres.py cycle`
  python tools/exp_gmres.py trace FILE [--n N]          reads a kernel trace (csv with Kernel_Name, Start_Timestamp, End_Timestamp)
                                                        and prints the share of the gm_* kernels in the second call and the GB/s of
                                                        gm_multidot and gm_update at j = 1, 15, 30 against their byte models

The byte models, in bytes for n rows: gm_multidot at column j reads (j + ceil(j / 4)) vectors; gm_update<false> reads j + 1 and writes 1
in its sweep, then reads j + ceil(j / 4) for the second pass's partials; gm_update<true> reads j + 1 and writes 1."""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "smvp-toolkit_amd", "python"), os.path.join(ROOT, "tests")]

RESTART = 30


def banded_csr(n):
    """bicgstab_method.banded(n) as CSR arrays, built without the COO detour."""
    i = np.arange(n)
    lens = np.full(n, 3)
    lens[0] = lens[-1] = 2
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.empty(row_ptr[-1], np.int32)
    val = np.empty(row_ptr[-1])
    d = row_ptr[:-1] + (i > 0)
    col[d], val[d] = i, 2.0 + (i % 7) / 8.0
    col[d[1:] - 1], val[d[1:] - 1] = i[1:] - 1, -0.75
    col[d[:-1] + 1], val[d[:-1] + 1] = i[:-1] + 1, -0.25
    return row_ptr, col, val


def setup(n):
    import torch

    import smvp_toolkit_amd as sm

    A = sm.CsrMatrix(n, n, *banded_csr(n))
    b = torch.from_numpy(np.random.default_rng(1).uniform(-1.0, 1.0, n)).cuda()
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    return torch, sm, A, b, x


def one_cycle(A, b, x):
    return A.gmres(b, x, restart=RESTART, max_steps=RESTART, tol=0.0, check_every=RESTART)


def timed(torch, fn, runs):
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), (max(out) - min(out)) / float(np.median(out))


def cmd_time(args):
    torch, sm, A, b, x = setup(args.n)
    print("# device %s; banded(%d); plan %s" % (torch.cuda.get_device_name(0), args.n, A.describe()[0][:80]))
    r, rr, tr = one_cycle(A, b, x)
    assert (r.steps, r.cycles, r.columns, r.reason) == (RESTART, 1, RESTART, sm.GMRES_MAX_STEPS), (r.steps, r.cycles, r.columns, r.reason)
    ms, spread = timed(torch, lambda: one_cycle(A, b, x), args.runs)
    print("smvp_csr_gmres, one cycle of %d steps: median %.3f ms over %d runs (spread %.1f %%): %.4f ms a step; rr_0 = %g, rr_30 = %g"
          % (RESTART, ms, args.runs, 100 * spread, ms / RESTART, rr[0], rr[-1]))
    y = torch.empty_like(x)
    pm, ps = timed(torch, lambda: [A.spmv(b, y) for _ in range(RESTART)], args.runs)
    print("the handle's product alone, %d times: median %.3f ms (spread %.1f %%)" % (RESTART, pm, 100 * ps))
    # the yardstick: what step j = 30 cost with the kernels the library had before -- 30 dots and 30 axpy-sized passes per pass of
    # Gram-Schmidt, serially dependent (the coefficient of each update comes back to the host)
    V = [torch.from_numpy(np.random.default_rng(10 + i).uniform(-1.0, 1.0, args.n)).cuda() for i in range(RESTART)]
    w = b.clone()

    def old_pass():
        for v in V:
            h = sm.vector_dot(v, w)
            w.add_(v, alpha=-float(h) * 1e-3)

    om, osp = timed(torch, old_pass, args.runs)
    print("yardstick at j = %d, one pass of Gram-Schmidt as %d x (smvp_vector_dot + one axpy pass): median %.3f ms (spread %.1f %%)"
          % (RESTART, RESTART, om, 100 * osp))

    def old_cgs():
        hs = [sm.vector_dot(v, w) for v in V]
        for v, h in zip(V, hs):
            w.add_(v, alpha=-float(h) * 1e-3)

    cm, cs = timed(torch, old_cgs, args.runs)
    print("yardstick at j = %d, classical order (the %d dots first, then the %d axpy passes): median %.3f ms (spread %.1f %%)"
          % (RESTART, RESTART, RESTART, cm, 100 * cs))
    A.close()


def cmd_cycle(args):
    torch, sm, A, b, x = setup(args.n)
    one_cycle(A, b, x)
    torch.cuda.synchronize()
    one_cycle(A, b, x)
    torch.cuda.synchronize()
    A.close()


def short(name):
    """gm_update<false> out of void smvp::(anonymous namespace)::gm_update<false>(double const*, ...) or of its mangled form."""
    plain = name.replace("(anonymous namespace)", "anon").split("(")[0].replace("void ", "").split("<")[0].split("::")[-1]
    if "gm_update" in name:
        tail = name.split("gm_update", 1)[1][:12]
        return "gm_update<true>" if ("true" in tail or "Lb1" in tail or "1>" in tail) else "gm_update<false>"
    for known in ("gm_multidot", "gm_fold", "gm_close", "gm_begin", "gm_residual", "gm_solve_y", "gm_form_u", "gm_add_x", "krylov_dot_parts"):
        if known in name:
            return known
    return plain[:60]


def cmd_trace(args):
    rows = list(csv.DictReader(open(args.file)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    begins = [i for i, r in enumerate(rows) if "krylov_dot_parts" in r["Kernel_Name"]]
    assert len(begins) == 2, "two calls expected in the trace, %d found" % len(begins)
    call = rows[begins[1]:]
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3       # noqa: E731  (us)
    total = sum(dur(r) for r in call)
    by = {}
    for r in call:
        name = short(r["Kernel_Name"])
        by[name] = by.get(name, 0.0) + dur(r)
    print("second call: %d launches, %.1f us of kernel time" % (len(call), total))
    for name, t in sorted(by.items(), key=lambda kv: -kv[1]):
        print("  %-48s %10.1f us  %5.1f %%" % (name[:48], t, 100 * t / total))
    orth = sum(t for name, t in by.items() if any(k in name for k in ("gm_multidot", "gm_fold", "gm_update", "gm_close")))
    print("orthogonalisation (gm_multidot, gm_fold, gm_update, gm_close): %.1f us = %.1f %% of the kernel time" % (orth, 100 * orth / total))
    vec = 8.0 * args.n
    for key, model in (("gm_multidot", lambda j: j + -(-j // 4)),
                       ("gm_update<false>", lambda j: (j + 2) + j + -(-j // 4)),
                       ("gm_update<true>", lambda j: j + 2)):
        pick = [r for r in call if short(r["Kernel_Name"]) == key]
        if len(pick) != RESTART:
            print("%s: %d launches in the call, %d expected" % (key, len(pick), RESTART))
            continue
        for j in (1, 15, 30):
            t = dur(pick[j - 1])
            print("%-18s j = %2d: %8.1f us, model %3d vectors = %7.1f MB: %7.1f GB/s" % (key, j, t, model(j), model(j) * vec / 1e6,
                                                                                    model(j) * vec / (t * 1e-6) / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["time", "cycle", "trace"])
    ap.add_argument("file", nargs="?")
    ap.add_argument("--n", type=int, default=4 * 1024 * 1024)
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    {"time": cmd_time, "cycle": cmd_cycle, "trace": cmd_trace}[args.cmd](args)


if __name__ == "__main__":
    main()
