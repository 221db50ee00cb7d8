"""The scenarios of LSQR (K22) that need the counted build: `python lsqr_scenarios.py GROUP` in a fresh process whose SMVP_LIB_PATH
names lib/libsmvp_amd_counted.so.  tests/resource_scenarios.py and tests/fresh_memory_scenarios.py are imported, not edited: the
snapshots, the sweeps and the fill patterns are theirs.

  resources   a successful smvp_csr_lsqr / smvp_tjds_lsqr (every way out of the loop), every refusal, and each obtaining call of
              the work space failing in turn leave the counters where they were
  fresh       the same solves with the fill off and under both fill patterns give the same bits, which are the restatement's: no
              partial, word, history element or element of x or w is read before it is written

"group GROUP ok" is the last line of a run that passed; a scenario that fails ends the process with status 1."""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs
import fresh_memory_scenarios as fm
import smvp_toolkit_amd as sm
from resource_scenarios import DONE, Failed, balanced, expect, status, unmoved


def routes(A):
    """((name, entry point, handles), ...) and the objects to close: the CSR pair h, ht = transposed(h), and the TJDS handle."""
    H = sm.CsrMatrix(A.m, A.n, *A.csr)
    HT = H.transposed()
    T = sm.TjdsMatrix(sm.tjds_from_coo(A.coo, A.m, A.n))
    return (("csr", "smvp_csr_lsqr", (H._h, HT._h)), ("tjds", "smvp_tjds_lsqr", (T._h,))), (HT, H, T)


def call_of(fn, handles, n, b, x0, max_steps, tol, atol, every=3, stream=None, x=None):
    """(thunk -> status, thunk -> (steps, updates, reason)) of one call."""
    import torch

    if x is None:
        x = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
    rn, arn = np.zeros(max_steps + 1), np.zeros(max_steps + 1)
    o, r = sm.lsqr_opts(max_steps, tol, atol, every), sm.LsqrResult()
    P, S = sm._dev_ptr, sm._stream_ptr(stream)
    return (lambda: status(fn, *handles, C.byref(o), P(b), P(x0), P(x), C.byref(r), sm._p(rn), sm._p(arn), S),
            lambda: (r.steps, r.updates, r.reason))


def group_resources():
    import torch

    import lsqr_method as lm

    A = lm.tall(300, 140)
    named, objects = routes(A)
    m, n = A.m, A.n
    db, d0 = rs.dev(lm.rhs(m)), rs.dev(lm.rhs(n, 7))
    consistent = rs.dev(A.spmv(lm.rhs(n, 5)))
    taken = set()
    # every way out of the host loop: each rule at a looked step and between looks, max_steps, stopped at step 0
    for name, fn, handles in named:
        for label, b, x0, max_steps, tol, atol, every in (("least squares", db, None, 80, 1e-10, 1e-10, 3), ("from an x0", db, d0, 80, 1e-10, 1e-10, 1000),
                                                          ("converges", consistent, None, 80, 1e-10, 0.0, 4), ("max_steps", db, None, 6, 0.0, 0.0, 4),
                                                          ("max_steps = 1", db, None, 1, 0.0, 0.0, 1),
                                                          ("zero b", rs.dev(np.zeros(m)), None, 10, 1e-10, 1e-10, 3),
                                                          ("a NaN in b", rs.dev(np.full(m, np.nan)), None, 10, 1e-10, 1e-10, 3)):
            call, result = call_of(fn, handles, n, b, x0, max_steps, tol, atol, every)
            what = "%s lsqr, %s" % (name, label)
            with balanced(what):
                rc = call()
                expect(rc == sm.OK, "%s: status %d (%s)" % (what, rc, rs.last_error()))
            taken.add(result()[2])
    expect(taken == {lm.CONVERGED, lm.LEAST_SQUARES, lm.MAX_STEPS, lm.NONFINITE}, "the runs ended with the reasons %r only" % taken)
    DONE.append("every way out was taken")
    # the refusals: not one counted call is made
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    buf = torch.zeros(m + n + 1, dtype=torch.float64, device="cuda")
    P = sm._dev_ptr
    H, HT, T = objects[1], objects[0], objects[2]
    for name, fn, handles in named:
        ok, r = sm.lsqr_opts(10, 1e-10, 1e-10, 3), sm.LsqrResult()
        bad = {}
        for field, value in (("max_steps", 0), ("check_every", 0), ("tol", float("nan")), ("atol", -1.0), ("struct_size", 8)):
            o = sm.lsqr_opts(10, 1e-10, 1e-10, 3)
            setattr(o, field, value)
            bad["%s = %r" % (field, value)] = o

        def args(h=handles, o=ok, b=db, x0=None, xx=x, res=r):
            return lambda: status(fn, *h, C.byref(o) if o is not None else None, P(b), P(x0), P(xx), C.byref(res) if res is not None else None,
                                  None, None, None)

        refusals = [("null handle", args(h=(None,) + handles[1:])), ("null opts", args(o=None)), ("null result", args(res=None)),
                    ("null d_b", args(b=None)), ("null d_x", args(xx=None)), ("d_b and d_x overlapping", args(b=buf[:m], xx=buf[:n])),
                    ("d_x0 and d_x overlapping in part", args(x0=buf[:n], xx=buf[1:n + 1]))]
        if name == "csr":
            refusals += [("null ht", args(h=(H._h, None))), ("ht of the wrong shape", args(h=(H._h, H._h)))]
        for label, o in bad.items():
            refusals.append((label, args(o=o)))
        for label, call in refusals:
            with unmoved("%s lsqr, %s, is refused without a counted call" % (name, label)):
                rc = call()
                expect(rc == sm.ERR_INVALID, "%s lsqr, %s: status %d, SMVP_ERR_INVALID expected" % (name, label, rc))
    for mode_on, mode_off, label in ((lambda: T.set_mode(sm.TJDS_MODE_ATOMIC), lambda: T.set_mode(sm.TJDS_MODE_ROW_GATHER), "in ATOMIC mode"),
                                     (lambda: T.set_ref_quirks(True), lambda: T.set_ref_quirks(False), "with ref-quirks on")):
        mode_on()
        call, _ = call_of("smvp_tjds_lsqr", (T._h,), n, db, None, 10, 1e-10, 1e-10)
        with unmoved("tjds lsqr %s is refused without a counted call" % label):
            expect(call() == sm.ERR_UNSUPPORTED, "tjds lsqr %s was not refused" % label)
        mode_off()
    from test_gpu_transposed import inner_csr_handle

    inner = inner_csr_handle(T, m, n, T.nnz)
    block = sm.CsrMatrix(m, n, *A.csr, first_row=2)
    for label, handles in (("a handle that is not plain CSR", (inner, HT._h)), ("a row block", (block._h, HT._h))):
        call, _ = call_of("smvp_csr_lsqr", handles, n, db, None, 10, 1e-10, 1e-10)
        with unmoved("csr lsqr on %s is refused without a counted call" % label):
            expect(call() == sm.ERR_UNSUPPORTED, "csr lsqr on %s: not SMVP_ERR_UNSUPPORTED" % label)
    block.close()
    # a capturing stream: refused before anything is enqueued or taken, and the capture stays valid
    side = torch.cuda.Stream()
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((n,), -12345.678, dtype=torch.float64, device="cuda")
    captured = [("%s lsqr" % name, call_of(fn, handles, n, db, None, 10, 1e-10, 1e-10, stream=side, x=dx)[0]) for name, fn, handles in named]
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
    for name, fn, handles in named:
        for label, x0 in (("from zeros", None), ("from an x0", d0)):
            rs.sweep_call("%s, %s" % (fn, label), call_of(fn, handles, n, db, x0, 12, 1e-10, 1e-10)[0], kinds=(rs.DEVICE, rs.PINNED))
    for Hh in objects:
        Hh.close()


def group_fresh():
    import torch

    import lsqr_method as lm
    import test_gpu_lsqr as k22
    from test_gpu_bicgstab import BOTH

    def solved(A, rhs, fmt, a, b, x0, max_steps, tol, atol, every, alias=False):
        def run():
            R = k22.Route(torch, A, fmt, a, b)
            got = k22.solve(torch, R, rhs, x0, max_steps, tol, atol, every, alias=alias)
            fm.arm(0)                                  # (the restatement's products: the check, not the run under test)
            k22.same(got, k22.restated(R, rhs, x0, max_steps, tol, atol), "the restatement")
            R.close()
            return {"result": tuple(int(v) for v in got[:3]), "rnorm_each": got[3], "arnorm_each": got[4], "x": got[5],
                    "norms": np.array(got[6])}
        return run

    tall, wide = lm.tall(1003, 517), lm.wide(131, 257)
    for fmt, a, b in BOTH:
        for A, name in ((tall, "tall(1003, 517)"), (wide, "wide(131, 257)")):
            for max_steps, tol, atol, every in ((40, 1e-10, 1e-10, 7), (9, 0.0, 0.0, 1000), (6, 0.0, 0.0, 1), (1, 0.0, 0.0, 1)):
                for x0 in (None, k22.start_vector(A.n)):
                    what = "lsqr, %s, %s, max_steps %d, tol %g, check_every %d, x0 %s" % (name, fmt, max_steps, tol, every,
                                                                                          "NULL" if x0 is None else "random")
                    fm.scenario(what, solved(A, lm.rhs(A.m), fmt, a, b, x0, max_steps, tol, atol, every))
        fm.scenario("lsqr, tall, %s, d_x is d_x0" % fmt, solved(tall, lm.rhs(1003), fmt, a, b, k22.start_vector(517), 12, 0.0, 0.0, 5, True))
        fm.scenario("lsqr, tall, %s, stopped at step 0" % fmt, solved(tall, lm.rhs(1003), fmt, a, b, None, 10, 1e30, 0.0, 3))
        fm.scenario("lsqr, tall, %s, a zero b: no vh_1 is formed" % fmt, solved(tall, np.zeros(1003), fmt, a, b, None, 10, 0.0, 0.0, 3))
        Z = lm.dense_rect([[2.0, 0.0], [0.0, 2.0]])
        fm.scenario("lsqr, diag(2, 2), %s, a zero beta in mid-run: no vh_2 is formed" % fmt,
                    solved(Z, np.array([3.0, 4.0]), fmt, a, b, None, 10, 0.0, 0.0, 3))
    expect(lm.CONVERGED == sm.LSQR_CONVERGED, "the reasons")


GROUPS = {"resources": group_resources, "fresh": group_fresh}


def main(argv):
    import gc

    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: lsqr_scenarios.py {%s}" % " | ".join(GROUPS))
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
