"""The scenarios of tests/test_gpu_gmres.py that need the counted build: `python gmres_scenarios.py GROUP` in a fresh process whose
SMVP_LIB_PATH names lib/libsmvp_amd_counted.so.  tests/resource_scenarios.py and tests/fresh_memory_scenarios.py are imported, not
edited: the snapshots, the sweeps and the fill patterns are theirs.

  resources   a successful smvp_csr_gmres / smvp_tjds_gmres (plain, Jacobi, plans; every way out of the loop), every refusal, and
              each obtaining call of the work space failing in turn leave the counters where they were
  fresh       the same solves with the fill off and under both fill patterns give the same bits, which are the restatement's: no
              partial, word, history element or basis slot is read before it is written

"group GROUP ok" is the last line of a run that passed; a scenario that fails ends the process with status 1."""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs
import fresh_memory_scenarios as fm
import smvp_toolkit_amd as sm
from resource_scenarios import DONE, Failed, balanced, expect, status, unmoved


def calls(H, n, b, x0, m, plans, restart, max_steps, tol, every=3, stream=None, x=None):
    """(name, thunk -> status, thunk -> (steps, cycles, columns, reason)) of the GMRES entry point of H: plain, Jacobi, plans."""
    import torch

    fn = "smvp_%s_gmres" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds")
    if x is None:
        x = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
    rr, tr = np.zeros(max_steps + 1), np.zeros(max_steps + 2)
    o, r = sm.gmres_opts(max_steps, tol, every, restart), sm.GmresResult()
    P, S = sm._dev_ptr, sm._stream_ptr(stream)
    first, second = (plans[0]._t, plans[1]._t) if plans else (None, None)
    result = lambda: (r.steps, r.cycles, r.columns, r.reason)    # noqa: E731

    def call(f, dm, s):
        return lambda: status(fn, H._h, C.byref(o), P(b), P(x0), P(x), f, P(dm), s, C.byref(r), sm._p(rr), sm._p(tr), S)

    yield "gmres plain", call(None, None, None), result
    if m is not None:
        yield "gmres jacobi", call(None, m, None), result
    if plans:
        yield "gmres plans", call(first, m, second), result


def group_resources():
    import torch

    import bicgstab_method as bi
    import gmres_method as gm

    M = bi.nonsym(300)
    A, T, plans = rs.solver_handles(M)
    db, dm = rs.dev(bi.rhs(300)), rs.dev(np.ones(300))
    d0 = rs.dev(bi.rhs(300, 7))
    taken = set()
    # every way out of the host loop: converged in mid-cycle, max_steps in mid-cycle and at a cycle's end, stopped at step 0
    for H, name in ((A, "csr"), (T, "tjds")):
        for label, b, x0, restart, max_steps, tol, every in (("converges", db, None, 5, 80, 1e-10, 3), ("from an x0", db, d0, 30, 80, 1e-10, 1000),
                                                             ("max_steps in mid-cycle", db, None, 4, 6, 0.0, 4),
                                                             ("max_steps at a cycle's end", db, None, 3, 6, 0.0, 1),
                                                             ("zero b", rs.dev(np.zeros(300)), None, 5, 10, 1e-10, 3)):
            for fn, call, result in calls(H, 300, b, x0, dm, plans, restart, max_steps, tol, every):
                what = "%s %s, %s" % (name, fn, label)
                with balanced(what):
                    rc = call()
                    expect(rc == sm.OK, "%s: status %d (%s)" % (what, rc, rs.last_error()))
                taken.add(result()[3])
    N = bi.nan_value()
    An, Tn, _ = rs.solver_handles(N)
    for H, name in ((An, "csr"), (Tn, "tjds")):
        for fn, call, result in calls(H, 300, db, None, None, None, 5, 10, 1e-10):
            with balanced("%s %s, a NaN matrix value" % (name, fn)):
                expect(call() == sm.OK, "%s %s, a NaN value: %s" % (name, fn, rs.last_error()))
            taken.add(result()[3])
    Z = sm.CsrMatrix(3, 3, np.array([0, 1, 1, 1], np.int32), np.zeros(1, np.int32), np.zeros(1))
    for fn, call, result in calls(Z, 3, rs.dev(np.ones(3)), None, None, None, 5, 10, 1e-10):
        with balanced("csr %s, the zero matrix" % fn):
            expect(call() == sm.OK, "csr %s, the zero matrix: %s" % (fn, rs.last_error()))
        taken.add(result()[3])
    Z.close()
    expect(taken == {gm.CONVERGED, gm.MAX_STEPS, gm.BREAKDOWN, gm.NONFINITE}, "the runs ended with the reasons %r only" % taken)
    DONE.append("every way out was taken")
    # the refusals: not one counted call is made
    x = torch.zeros(300, dtype=torch.float64, device="cuda")
    buf = torch.zeros(301, dtype=torch.float64, device="cuda")
    P = sm._dev_ptr
    eye2 = sm.CsrMatrix(2, 2, np.arange(3, dtype=np.int32), np.arange(2, dtype=np.int32), np.ones(2))
    small = (eye2.trsv_plan(sm.TRSV_LOWER), eye2.trsv_plan(sm.TRSV_UPPER))
    for H, name in ((A, "csr"), (T, "tjds")):
        fn = "smvp_%s_gmres" % name
        ok, r = sm.gmres_opts(10, 1e-10, 3, 5), sm.GmresResult()
        bad = {}
        for field, value in (("restart", 0), ("restart", 65), ("max_steps", 0), ("check_every", 0), ("tol", float("nan")), ("struct_size", 8)):
            o = sm.gmres_opts(10, 1e-10, 3, 5)
            setattr(o, field, value)
            bad["%s = %r" % (field, value)] = o
        refusals = [("null handle", lambda: status(fn, None, C.byref(ok), P(db), None, P(x), None, None, None, C.byref(r), None, None, None)),
                    ("null opts", lambda: status(fn, H._h, None, P(db), None, P(x), None, None, None, C.byref(r), None, None, None)),
                    ("null result", lambda: status(fn, H._h, C.byref(ok), P(db), None, P(x), None, None, None, None, None, None, None)),
                    ("null d_b", lambda: status(fn, H._h, C.byref(ok), None, None, P(x), None, None, None, C.byref(r), None, None, None)),
                    ("null d_x", lambda: status(fn, H._h, C.byref(ok), P(db), None, None, None, None, None, C.byref(r), None, None, None)),
                    ("d_b is d_x", lambda: status(fn, H._h, C.byref(ok), P(x), None, P(x), None, None, None, C.byref(r), None, None, None)),
                    ("d_m is d_x", lambda: status(fn, H._h, C.byref(ok), P(db), None, P(x), None, P(x), None, C.byref(r), None, None, None)),
                    ("d_x0 and d_x overlapping in part", lambda: status(fn, H._h, C.byref(ok), P(db), P(buf[:300]), P(buf[1:]), None, None, None,
                                                                        C.byref(r), None, None, None)),
                    ("plans of another size", lambda: status(fn, H._h, C.byref(ok), P(db), None, P(x), small[0]._t, None, small[1]._t,
                                                             C.byref(r), None, None, None))]
        for label, o in bad.items():
            refusals.append((label, (lambda o: lambda: status(fn, H._h, C.byref(o), P(db), None, P(x), None, None, None, C.byref(r), None, None,
                                                              None))(o)))
        for label, call in refusals:
            with unmoved("%s gmres, %s, is refused without a counted call" % (name, label)):
                rc = call()
                expect(rc == sm.ERR_INVALID, "%s gmres, %s: status %d, SMVP_ERR_INVALID expected" % (name, label, rc))
    for mode_on, mode_off, label in ((lambda: T.set_mode(sm.TJDS_MODE_ATOMIC), lambda: T.set_mode(sm.TJDS_MODE_ROW_GATHER), "in ATOMIC mode"),
                                     (lambda: T.set_ref_quirks(True), lambda: T.set_ref_quirks(False), "with ref-quirks on")):
        mode_on()
        for fn, call, _ in calls(T, 300, db, None, dm, plans, 5, 10, 1e-10):
            with unmoved("tjds %s %s is refused without a counted call" % (fn, label)):
                expect(call() == sm.ERR_UNSUPPORTED, "tjds %s %s was not refused" % (fn, label))
        mode_off()
    from test_gpu_transposed import inner_csr_handle

    inner = inner_csr_handle(T, 300, 300, T.nnz)
    ok, r = sm.gmres_opts(10, 1e-10, 3, 5), sm.GmresResult()
    with unmoved("csr gmres on a handle that is not plain CSR is refused without a counted call"):
        expect(status("smvp_csr_gmres", inner, C.byref(ok), P(db), None, P(x), None, None, None, C.byref(r), None, None, None) == sm.ERR_UNSUPPORTED,
               "csr gmres on a handle that is not plain CSR: not SMVP_ERR_UNSUPPORTED")
    # a capturing stream: refused before anything is enqueued or taken, and the capture stays valid
    side = torch.cuda.Stream()
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((300,), -12345.678, dtype=torch.float64, device="cuda")
    captured = [("%s %s" % (name, fn), call) for H, name in ((A, "csr"), (T, "tjds"))
                for fn, call, _ in calls(H, 300, db, None, dm, plans, 5, 10, 1e-10, stream=side, x=dx)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dZ.add_(1.0)                               # (keeps the captured graph from being empty)
            for label, call in captured:
                with unmoved("%s on a capturing stream is refused without a counted call" % label):
                    rc = call()
                    expect(rc == sm.ERR_INVALID and "captur" in rs.last_error(), "%s on a capturing stream: status %d (%s)" % (label, rc, rs.last_error()))
            dZ.add_(1.0)
    g.replay()
    torch.cuda.synchronize()
    expect(dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == -12345.678).all(),
           "the capture did not stay valid, or a refused call wrote d_x")
    DONE.append("the capture stayed valid")
    del g
    with balanced("the same stream outside a capture is fine"):
        for label, call in captured:
            expect(call() == sm.OK, "%s on the same stream outside the capture: %s" % (label, rs.last_error()))
    # each obtaining call of the work space failing in turn: device memory and pinned host memory
    for H, name in ((A, "csr"), (T, "tjds")):
        for fn, call, _ in calls(H, 300, db, None, dm, plans, 5, 12, 1e-10):
            rs.sweep_call("smvp_%s_%s" % (name, fn.replace(" ", ", ")), call, kinds=(rs.DEVICE, rs.PINNED))
    for Q in small + plans:
        Q.close()
    for Hh in (eye2, T, A, Tn, An):
        Hh.close()


def group_fresh():
    import torch

    import bicgstab_method as bi
    import gmres_method as gm
    import pbicgstab_method as pb
    import test_gpu_gmres as k19
    import test_gpu_pbicgstab as k18
    from test_gpu_bicgstab import BOTH, handle, start_vector

    def solved(M, Cs, kind, fmt, a, b, x0, restart, max_steps, tol, every):
        def run():
            P = k19.PLAIN if kind == "plain" else k18.plans_of(torch, kind, Cs)
            H, product = handle(torch, M, fmt, a, b)
            rhs = bi.rhs(M.n)
            got = k19.solve(torch, H, M.n, rhs, P, x0, restart, max_steps, tol, every)
            fm.arm(0)                                  # (the restatement's products: the check, not the run under test)
            k19.same(got, k19.restated(product, rhs, P, x0, restart, max_steps, tol), "the restatement", rhs)
            H.close()
            P.close()
            return {"result": tuple(int(v) for v in got[:4]), "rr_each": got[4], "restart_each": got[5], "x": got[6],
                    "rr": float(got[7]), "bb": float(got[8])}
        return run

    M, Cs = pb.case_of("convdiff(32, 0.5)")
    N = bi.nonsym(1003)
    for fmt, a, b in BOTH:
        for kind, restart, max_steps, tol, every in (("plain", 30, 45, 0.0, 7), ("plain", 3, 40, 1e-6, 1000), ("jacobi", 5, 12, 0.0, 5),
                                                     ("ilu0", 4, 60, 1e-8, 3), ("sgs", 30, 60, 1e-8, 1000)):
            for x0 in (None, start_vector(M.n)):
                what = "gmres, convdiff(32, 0.5), %s, %s, restart %d, max_steps %d, tol %g, x0 %s" % (
                    kind, fmt, restart, max_steps, tol, "NULL" if x0 is None else "random")
                fm.scenario(what, solved(M, Cs, kind, fmt, a, b, x0, restart, max_steps, tol, every))
        fm.scenario("gmres, nonsym(1003), %s, restart 64 of which few columns are used" % fmt,
                    solved(N, None, "plain", fmt, a, b, None, 64, 64, 1e-10, 1000))
        fm.scenario("gmres, nonsym(1003), %s, stopped at step 0" % fmt, solved(N, None, "plain", fmt, a, b, None, 5, 10, 1e30, 3))
    expect(gm.CONVERGED == sm.GMRES_CONVERGED, "the reasons")


GROUPS = {"resources": group_resources, "fresh": group_fresh}


def main(argv):
    import gc

    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: gmres_scenarios.py {%s}" % " | ".join(GROUPS))
        return 2
    if not hasattr(sm.lib(), "smvp_test_resources") or not hasattr(sm.lib(), "smvp_test_fill_allocations"):
        print("FAIL: %s is not the counted build (set SMVP_LIB_PATH to lib/libsmvp_amd_counted.so)" % sm.LIB_PATH)
        return 2
    assert torch.cuda.is_available(), "the scenarios need the GPU"
    torch.zeros(1, device="cuda")
    group = argv[1]
    start, fills = rs.snap(), fm.stats()
    try:
        if group == "fresh":
            fm.probe_both_patterns()
        GROUPS[group]()
        gc.collect()
        torch.cuda.synchronize()
        end = fm.stats()
        expect(end[2] == 0, "%d fills failed" % end[2])
        if group == "fresh":
            expect(end[0] > fills[0], "no allocation was filled in the whole group")
        rs.require_same(start, rs.snap(), "the whole group %s: everything obtained was given back" % group)
        expect(rs.snap()[rs.FOREIGN] == 0, "foreign frees")
    except Failed as e:
        for what in (DONE + fm.DONE)[-3:]:
            print("ok   " + what)
        print("FAIL " + str(e))
        return 1
    except Exception:                                # anything else (a HIP error out of torch, say) is a crash, not a failed scenario
        import traceback

        traceback.print_exc()
        print("CRASH in group %s after %d scenarios" % (group, len(DONE) + len(fm.DONE)))
        return 3
    print("%d scenarios" % (len(DONE) + len(fm.DONE)))
    print("group %s ok" % group)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
