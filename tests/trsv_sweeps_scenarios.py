"""The resource scenarios of tests/test_gpu_trsv_sweeps.py: `python trsv_sweeps_scenarios.py GROUP` in a fresh process whose
SMVP_LIB_PATH names lib/libsmvp_amd_counted.so, on the counters and helpers of tests/resource_scenarios.py.  A sweeps plan
(smvp_csr_trsv_create_sweeps, K21) owns four device buffers -- begin, end and two scratch vectors; every comparison is exact."""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs
from resource_scenarios import DEVICE, BYTES, LIVE, at, balanced, dev, expect, require_same, snap, status, sweep_create

sm = rs.sm


def matrices():
    import cg_method as cg
    import ilu0_method as im

    G = im.as_matrix(im.grid(24))
    Mx = cg.spd(300)
    m, nn, coo, csr = rs.sample("memplus.mtx")
    return (("spd(300)", Mx.n, Mx.csr), ("lap2d(24)", G.n, G.csr), ("memplus", m, csr))


def group_balance():
    import torch

    for name, n, csr in matrices():
        for sweeps in (0, 1, 2, 5):
            with balanced("%s: create, solves and destroy of plans of %d sweeps" % (name, sweeps)):
                A = sm.CsrMatrix(n, n, *csr)
                b = dev(np.random.default_rng(5).uniform(-1.0, 1.0, n))
                x = torch.empty(n, dtype=torch.float64, device="cuda")
                bare = snap()
                for uplo in (sm.TRSV_LOWER, sm.TRSV_UPPER):
                    for diag in (sm.TRSV_DIAG_STORED, sm.TRSV_DIAG_UNIT):
                        P = A.trsv_plan(uplo, diag, sweeps=sweeps)
                        planned = snap()
                        expect(at(planned, DEVICE, LIVE) - at(bare, DEVICE, LIVE) == 4, "%s: a sweeps plan holds other than four device buffers" % name)
                        P.solve(b, x)
                        P.solve(x, x)
                        torch.cuda.synchronize()
                        require_same(planned, snap(), "%s: solves of %d sweeps (uplo %d, diag %d)" % (name, sweeps, uplo, diag), counters=True)
                        P.close()
                        require_same(bare, snap(), "%s: the plan destroyed" % name)
                A.close()
    with balanced("sweeps plans of an ILU(0), and of a matrix without rows"):
        import ilu0_method as im

        G = im.as_matrix(im.grid(24))
        A = sm.CsrMatrix(G.n, G.n, *G.csr)
        f = A.ilu0()
        L, U = f.plans(sweeps=3)
        b = dev(np.ones(G.n))
        U.solve(L.solve(b, b), b)
        torch.cuda.synchronize()
        U.close()
        L.close()
        f.close()
        A.close()
        E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        P = E.trsv_plan(sm.TRSV_LOWER, sweeps=2)
        P.close()
        E.close()


def group_refused():
    for name, n, csr in matrices()[:2]:
        A = sm.CsrMatrix(n, n, *csr)
        for uplo, diag, sweeps in ((sm.TRSV_LOWER, sm.TRSV_DIAG_STORED, 3), (sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT, 0)):
            def create():
                out = C.c_void_p()
                rc = status("smvp_csr_trsv_create_sweeps", C.byref(out), A._h, uplo, diag, sweeps, None)
                return rc, out.value

            before = snap()
            rc, obj = create()
            expect(rc == sm.OK and at(snap(), DEVICE, rs.OBTAINS) - at(before, DEVICE, rs.OBTAINS) == 4,
                   "%s: smvp_csr_trsv_create_sweeps makes other than four device allocations" % name)
            sm.lib().smvp_trsv_destroy(C.c_void_p(obj))
            sweep_create("smvp_csr_trsv_create_sweeps on %s (uplo %d, diag %d, %d sweeps)" % (name, uplo, diag, sweeps), create,
                         lambda t: sm.lib().smvp_trsv_destroy(C.c_void_p(t)))
        A.close()


def group_plan_bytes():
    for name, n, csr in matrices():
        A = sm.CsrMatrix(n, n, *csr)
        bare = snap()
        for sweeps in (0, 4):
            P = A.trsv_plan(sm.TRSV_LOWER, sweeps=sweeps)
            now = snap()
            held, allocs = at(now, DEVICE, BYTES) - at(bare, DEVICE, BYTES), at(now, DEVICE, LIVE) - at(bare, DEVICE, LIVE)
            reported = P.info()["plan_bytes"]
            print("plan_bytes %-40s reported %12.0f  held %12d  allocations %d" % ("%s, %d sweeps" % (name, sweeps), reported, held, allocs))
            expect(allocs == 4 and reported == held == max(n, 4) * 24, "%s, %d sweeps: plan_bytes %r, held %d in %d allocations" % (
                name, sweeps, reported, held, allocs))
            P.close()
            require_same(bare, snap(), "%s: the plan destroyed" % name)
        A.close()
    rs.DONE.append("plan_bytes of sweeps plans")


GROUPS = {"balance": group_balance, "refused": group_refused, "plan_bytes": group_plan_bytes}


def main(argv):
    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: trsv_sweeps_scenarios.py {%s}" % " | ".join(GROUPS))
        return 2
    if not hasattr(sm.lib(), "smvp_test_resources"):
        print("FAIL: %s is not the counted build (set SMVP_LIB_PATH to lib/libsmvp_amd_counted.so)" % sm.LIB_PATH)
        return 2
    assert torch.cuda.is_available(), "the scenarios need the GPU"
    torch.zeros(1, device="cuda")
    start = snap()
    try:
        GROUPS[argv[1]]()
        import gc

        gc.collect()
        torch.cuda.synchronize()
        require_same(start, snap(), "the whole group %s" % argv[1])
        expect(snap()[rs.FOREIGN] == 0, "foreign frees")
    except rs.Failed as e:
        for what in rs.DONE[-3:]:
            print("ok   " + what)
        print("FAIL " + str(e))
        return 1
    print("%d scenarios" % len(rs.DONE))
    print("group %s ok" % argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
