"""The scenarios of tests/test_gpu_cg_multi.py that need the counted build: `python cg_multi_scenarios.py GROUP` in a fresh process
whose SMVP_LIB_PATH names lib/libsmvp_amd_counted.so.  tests/resource_scenarios.py and tests/fresh_memory_scenarios.py are imported,
not edited: the snapshots, the sweeps and the fill patterns are theirs.

  resources   a successful smvp_csr_cg_multi / smvp_tjds_cg_multi (plain and Jacobi; every way out, mixed in one block), every
              refusal, and each obtaining call of the workspace failing in turn leave the counters where they were; the
              block-product plan the first call builds stays with the handle and goes with it
  fresh       the same solves with the fill off and under both fill patterns give the same bits, which are the restatement's: no
              partial, word, status block or history element is read before it is written

"group GROUP ok" is the last line of a run that passed; a scenario that fails ends the process with status 1.  An error of the
device is no scenario's verdict: nothing is run after it and the process ends with status 3."""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs
import fresh_memory_scenarios as fm
import smvp_toolkit_amd as sm
from resource_scenarios import DONE, Failed, balanced, expect, status, unmoved


def fn_of(H):
    return "smvp_%s_cg_multi" % ("csr" if isinstance(H, sm.CsrMatrix) else "tjds")


def call_of(H, k, B, X0, X, m, max_steps, tol, every=3, stream=None, results=None):
    """(thunk -> status, the k result blocks) of one call on contiguous (n, k) device blocks; the thunk keeps its operands alive."""
    o = sm.cg_opts(max_steps, tol, every)
    r = (sm.PcgResult * k)() if results is None else results
    rr, rz, sigma = np.zeros(k * (max_steps + 1)), np.zeros(k * (max_steps + 1)), np.zeros(k * max_steps)
    P, S = sm._dev_ptr, sm._stream_ptr(stream)
    return (lambda: status(fn_of(H), H._h, C.byref(o), k, P(B), k, P(X0), k, P(X), k, P(m), r, sm._p(rr), sm._p(rz), sm._p(sigma), S)), r


def handles(M):
    """(CSR handle, TJDS handle) of a square power_iteration.Matrix."""
    return sm.CsrMatrix(M.n, M.n, *M.csr), sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))


def group_resources():
    import torch

    import cg_method as cg
    import cg_multi_method as cm
    import pcg_method as pcg

    n, k = 300, 5
    M = cg.spd(n)
    db = rs.dev(np.random.default_rng(3).uniform(-1.0, 1.0, (n, k)))
    d0 = rs.dev(np.random.default_rng(4).uniform(-2.0, 2.0, (n, k)))
    dm = rs.dev(pcg.diagonal(M))
    x = torch.zeros((n, k), dtype=torch.float64, device="cuda")
    # the first call on a fresh handle builds the block-product plan, which stays with the handle and goes with it
    for name in ("csr", "tjds"):
        with balanced("%s: a fresh handle, its first cg_multi, closed" % name):
            A, T = handles(M)
            H, other = (A, T) if name == "csr" else (T, A)
            other.close()
            call, _ = call_of(H, k, db, None, x, None, 40, 1e-10)
            rc = call()
            expect(rc == sm.OK, "%s, the first call: status %d (%s)" % (name, rc, rs.last_error()))
            H.close()
    A, T = handles(M)
    for H in (A, T):                                     # from here on the plans exist: a call gives back all it takes
        rc = call_of(H, k, db, None, x, None, 2, 0.0)[0]()
        expect(rc == sm.OK, "warming %s: %s" % (fn_of(H), rs.last_error()))
    taken = set()
    for H, name in ((A, "csr"), (T, "tjds")):
        for label, B, X0, m, max_steps, tol, every in (("converges", db, None, None, 60, 1e-10, 3), ("jacobi from an X0", db, d0, dm, 60, 1e-10, 1000),
                                                       ("X is X0", db, x, dm, 60, 1e-10, 7), ("max_steps", db, None, None, 4, 0.0, 3),
                                                       ("zero B", rs.dev(np.zeros((n, k))), None, dm, 10, 1e-10, 1)):
            what = "%s cg_multi, %s" % (name, label)
            call, r = call_of(H, k, B, X0, x, m, max_steps, tol, every)
            with balanced(what):
                rc = call()
                expect(rc == sm.OK, "%s: status %d (%s)" % (what, rc, rs.last_error()))
            taken |= {b.reason for b in r}
    S = cm.signed_diagonal()
    As, Ts = handles(S)
    dmix, xs = rs.dev(cm.mixed_block()), torch.zeros((S.n, 6), dtype=torch.float64, device="cuda")
    dabs = rs.dev(np.abs(cm.signed_diagonal_values()))
    for H, name in ((As, "csr"), (Ts, "tjds")):
        expect(call_of(H, 6, dmix, None, xs, None, 1, 0.0)[0]() == sm.OK, "warming %s on the signed diagonal" % name)
        for m, expected in ((None, cm.MIXED_PLAIN), (dabs, cm.MIXED_JACOBI)):
            call, r = call_of(H, 6, dmix, None, xs, m, cm.MIXED_STEPS, cm.MIXED_TOL, 2)
            with balanced("%s cg_multi, every way out in one block%s" % (name, "" if m is None else ", jacobi")):
                expect(call() == sm.OK, "%s, the mixed block: %s" % (name, rs.last_error()))
            got = [(b.steps, b.updates, b.reason) for b in r]
            expect(got == expected, "%s, the mixed block ended with %r, %r expected" % (name, got, expected))
            taken |= {b.reason for b in r}
    expect(taken == {sm.CG_CONVERGED, sm.CG_MAX_STEPS, sm.CG_BREAKDOWN, sm.CG_NONFINITE}, "the runs ended with the reasons %r only" % taken)
    DONE.append("every way out was taken")
    # the refusals: not one counted call is made
    P = sm._dev_ptr
    buf = torch.zeros(n * k + 1, dtype=torch.float64, device="cuda")
    lo, hi = buf[:n * k].view(n, k), buf[1:].view(n, k)
    for H, name in ((A, "csr"), (T, "tjds")):
        fn = fn_of(H)
        ok, r = sm.cg_opts(10, 1e-10, 3), (sm.PcgResult * k)()
        rest = (r, None, None, None, None)
        bad = {}
        for field, value in (("max_steps", 0), ("check_every", 0), ("tol", float("nan")), ("struct_size", 8)):
            o = sm.cg_opts(10, 1e-10, 3)
            setattr(o, field, value)
            bad["%s = %r" % (field, value)] = o
        refusals = [("null handle", lambda: status(fn, None, C.byref(ok), k, P(db), k, None, 0, P(x), k, None, *rest)),
                    ("null opts", lambda: status(fn, H._h, None, k, P(db), k, None, 0, P(x), k, None, *rest)),
                    ("null results", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, None, 0, P(x), k, None, None, None, None, None, None)),
                    ("null d_B", lambda: status(fn, H._h, C.byref(ok), k, None, k, None, 0, P(x), k, None, *rest)),
                    ("null d_X", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, None, 0, None, k, None, *rest)),
                    ("k = 0", lambda: status(fn, H._h, C.byref(ok), 0, P(db), k, None, 0, P(x), k, None, *rest)),
                    ("ldb below k", lambda: status(fn, H._h, C.byref(ok), k, P(db), k - 1, None, 0, P(x), k, None, *rest)),
                    ("ldx below k", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, None, 0, P(x), k - 1, None, *rest)),
                    ("ldx0 below k", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, P(d0), k - 1, P(x), k, None, *rest)),
                    ("d_B is d_X", lambda: status(fn, H._h, C.byref(ok), k, P(x), k, None, 0, P(x), k, None, *rest)),
                    ("d_m inside d_X", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, None, 0, P(x), k, P(x[1:]), *rest)),
                    ("d_X0 and d_X overlapping in part", lambda: status(fn, H._h, C.byref(ok), k, P(db), k, P(lo), k, P(hi), k, None, *rest))]
        for label, o in bad.items():
            refusals.append((label, (lambda o: lambda: status(fn, H._h, C.byref(o), k, P(db), k, None, 0, P(x), k, None, *rest))(o)))
        for label, call in refusals:
            with unmoved("%s cg_multi, %s, is refused without a counted call" % (name, label)):
                rc = call()
                expect(rc == sm.ERR_INVALID, "%s cg_multi, %s: status %d, SMVP_ERR_INVALID expected" % (name, label, rc))
    from test_gpu_transposed import inner_csr_handle

    T3 = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, n, n))
    inner = inner_csr_handle(T3, n, n, T3.nnz)
    ok, r = sm.cg_opts(10, 1e-10, 3), (sm.PcgResult * k)()
    with unmoved("csr cg_multi on a handle that is not plain CSR is refused without a counted call"):
        expect(status("smvp_csr_cg_multi", inner, C.byref(ok), k, P(db), k, None, 0, P(x), k, None, r, None, None, None, None) == sm.ERR_UNSUPPORTED,
               "csr cg_multi on a handle that is not plain CSR: not SMVP_ERR_UNSUPPORTED")
    T3.close()
    # a capturing stream: refused before anything is enqueued or taken, and the capture stays valid
    side = torch.cuda.Stream()
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((n, k), -12345.678, dtype=torch.float64, device="cuda")
    captured = [("%s, %s" % (name, "plain" if m is None else "jacobi"), call_of(H, k, db, None, dx, m, 10, 1e-10, stream=side)[0])
                for H, name in ((A, "csr"), (T, "tjds")) for m in (None, dm)]
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
           "the capture did not stay valid, or a refused call wrote d_X")
    DONE.append("the capture stayed valid")
    del g
    with balanced("the same stream outside a capture is fine"):
        for label, call in captured:
            expect(call() == sm.OK, "%s on the same stream outside the capture: %s" % (label, rs.last_error()))
    # each obtaining call of the workspace failing in turn: device memory and pinned host memory
    for H, name in ((A, "csr"), (T, "tjds")):
        for m, label in ((None, "plain"), (dm, "jacobi")):
            rs.sweep_call("smvp_%s_cg_multi, %s" % (name, label), call_of(H, k, db, d0, x, m, 12, 1e-10)[0], kinds=(rs.DEVICE, rs.PINNED))
    for Hh in (Ts, As, T, A):
        Hh.close()


def group_fresh():
    import torch

    import cg_multi_method as cm
    import test_gpu_cg_multi as k20

    def solved(name, args, fmt, a, b, k, with_m, x0, wide, every, max_steps=k20.MAX_STEPS, tol=k20.TOL):
        def run():
            M = k20.matrix(name, *args)
            H = k20.handle(M, fmt, a, b)
            B = k20.rhs_block(M.n)[:, :k]
            X0 = k20.start_block(M.n)[:, :k] if x0 != "none" else None
            m = k20.jacobi(name, *args) if with_m else None
            got = k20.solve(torch, H, B, X0, m, max_steps, tol, every, alias=x0 == "alias", wide=wide)
            want = k20.restated(name, args, fmt, with_m, x0 != "none", k20.KMAX, max_steps, tol)[:k]
            k20.same(got, want, "the restatement", B, with_m)
            H.close()
            return {"result": [(r.steps, r.updates, r.reason, float(r.rr), float(r.rz), float(r.bb)) for r in got.results],
                    "rr_each": got.rr, "rz_each": got.rz, "sigma_each": got.sigma, "X": got.X}
        return run

    def mixed(fmt, a, b, with_m):
        def run():
            M, B = cm.signed_diagonal(), cm.mixed_block()
            m = np.abs(cm.signed_diagonal_values()) if with_m else None
            H = k20.handle(M, fmt, a, b)
            got = k20.solve(torch, H, B, None, m, cm.MIXED_STEPS, cm.MIXED_TOL, 2, wide=True)
            k20.same(got, cm.run(cm.product_of(M, fmt), B, None, m, cm.MIXED_STEPS, cm.MIXED_TOL), "the restatement", None, with_m)
            H.close()
            return {"result": [(r.steps, r.updates, r.reason, float(r.rr), float(r.rz), float(r.bb)) for r in got.results],
                    "rr_each": got.rr, "rz_each": got.rz, "sigma_each": got.sigma, "X": got.X}
        return run

    for fmt, a, b in k20.BOTH:
        for j, (name, args) in enumerate(k20.MATRICES):
            for k, with_m, x0, wide, every in ((1, False, "none", False, 1000), (3, True, "own", True, 3), (16, False, "alias", False, 7),
                                               (17, True, "none", True, 4), (33, j == 1, "own", j != 1, 1000)):
                what = "cg_multi, %s, %s, k = %d, %s, x0 %s, %s, check_every %d" % (
                    name, fmt, k, "jacobi" if with_m else "plain", x0, "column slices" if wide else "ld = k", every)
                fm.scenario(what, solved(name, args, fmt, a, b, k, with_m, x0, wide, every))
        fm.scenario("cg_multi, spd(1003), %s, stopped by max_steps" % fmt, solved("spd", (1003,), fmt, a, b, 5, True, "own", False, 2, 4, 0.0))
        fm.scenario("cg_multi, spd(1003), %s, every column stopped at step 0" % fmt,
                    solved("spd", (1003,), fmt, a, b, 5, False, "none", True, 3, 10, 1e30))
        for with_m in (False, True):
            fm.scenario("cg_multi, the signed diagonal, %s, every way out in one block%s" % (fmt, ", jacobi" if with_m else ""),
                        mixed(fmt, a, b, with_m))
    expect(cm.CONVERGED == sm.CG_CONVERGED and cm.NONFINITE == sm.CG_NONFINITE, "the reasons")


GROUPS = {"resources": group_resources, "fresh": group_fresh}


def main(argv):
    import gc

    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: cg_multi_scenarios.py {%s}" % " | ".join(GROUPS))
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
