"""The scenarios of tests/test_gpu_multicolor.py that need the counted build: `python multicolor_scenarios.py GROUP` in a fresh
process whose SMVP_LIB_PATH names lib/libsmvp_amd_counted.so.  tests/resource_scenarios.py and tests/fresh_memory_scenarios.py are
imported, not edited: the snapshots, the sweeps and the fill patterns are theirs.

  resources   smvp_csr_color allocates one counter and frees it on every way out; smvp_perm_from_classes one workspace;
              smvp_csr_create_permuted gives back everything but the handle it returns, which smvp_csr_destroy releases;
              smvp_vector_gather allocates nothing.  Every refusal leaves the counters alone, and each device allocation failing in
              turn gives SMVP_ERR_ALLOC or SMVP_ERR_HIP with nothing held and *out NULL
  fresh       the colours, B's arrays and the gathered vectors with the fill off and under both fill patterns are the same, and the
              restatement's: nothing is read before it is written

"group GROUP ok" is the last line of a run that passed; a scenario that fails ends the process with status 1, an error of the device
ends it with status 3 and the caller starts no further group."""
import ctypes as C
import sys

import numpy as np

import resource_scenarios as rs                      # (first: it puts the package and the tests on sys.path)
import coloring_method as cm
import fresh_memory_scenarios as fm
import smvp_toolkit_amd as sm
from resource_scenarios import DEVICE, DONE, LIVE, OBTAINS, Failed, at, balanced, expect, require_same, snap, status, unmoved


def ints(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def patterns():
    return cm.lap2d(32), cm.messy(), cm.sample("memplus")


def color_call(A, At, d, seed=0, max_rounds=4096, info=True):
    o = sm.ColorOpts()
    sm.lib().smvp_color_opts_default(C.byref(o))
    o.seed, o.max_rounds = seed, max_rounds
    i = sm.ColorInfo()
    i.struct_size = C.sizeof(sm.ColorInfo)
    return status("smvp_csr_color", A._h, None if At is None else At._h, C.byref(o), sm._dev_ptr(d), C.byref(i) if info else None, None), i


def group_resources():
    import torch

    for P in patterns():
        A = sm.CsrMatrix(P.n, P.n, *P.csr)
        At = A.transposed()
        d = torch.empty(P.n, dtype=torch.int32, device="cuda")
        want, colors, depth = P.reference(True, 0)
        with balanced("%s: smvp_csr_color, with and without ht and info" % P.name):
            for ht in (None, At):
                for info in (True, False):
                    before = snap()
                    rc, i = color_call(A, ht, d, info=info)
                    expect(rc == sm.OK, "smvp_csr_color on %s: status %d (%s)" % (P.name, rc, rs.last_error()))
                    now = snap()
                    expect(at(now, DEVICE, OBTAINS) - at(before, DEVICE, OBTAINS) == 1, "%s: smvp_csr_color allocates other than the counter" % P.name)
                    require_same(before, now, "%s: smvp_csr_color" % P.name)
            expect((d.cpu().numpy() == want).all(), "%s: the colours" % P.name)
        with balanced("%s: a run cut short by max_rounds leaks nothing" % P.name):
            if depth > 1:
                rc, _ = color_call(A, At, d, max_rounds=1)
                expect(rc == sm.ERR_UNSUPPORTED, "%s: max_rounds = 1 gives status %d" % (P.name, rc))
        with unmoved("%s: refused smvp_csr_color calls make no counted call" % P.name):
            o = sm.ColorOpts()
            sm.lib().smvp_color_opts_default(C.byref(o))
            o.max_rounds = 0
            expect(status("smvp_csr_color", A._h, None, C.byref(o), sm._dev_ptr(d), None, None) == sm.ERR_INVALID, "max_rounds = 0")
            expect(status("smvp_csr_color", None, None, None, sm._dev_ptr(d), None, None) == sm.ERR_INVALID, "a NULL handle")
            expect(status("smvp_csr_color", A._h, None, None, None, None, None) == sm.ERR_INVALID, "a NULL d_color")
        rs.sweep_call("smvp_csr_color on %s" % P.name, lambda: color_call(A, At, d)[0], codes=(sm.ERR_ALLOC,))
        # classes to a permutation: one workspace
        dcol = ints(want)
        o1, o2 = (torch.empty(P.n, dtype=torch.int32, device="cuda") for _ in range(2))
        ptr = np.zeros(colors + 1, np.int32)

        def perm(classes=colors, src=dcol):
            return status("smvp_perm_from_classes", 0, P.n, classes, sm._dev_ptr(src), sm._dev_ptr(o1), sm._dev_ptr(o2), sm._p(ptr), None)

        with balanced("%s: smvp_perm_from_classes" % P.name):
            before = snap()
            expect(perm() == sm.OK, "smvp_perm_from_classes on %s: %s" % (P.name, rs.last_error()))
            expect(at(snap(), DEVICE, OBTAINS) - at(before, DEVICE, OBTAINS) == 1, "%s: smvp_perm_from_classes makes other than one allocation" % P.name)
            w = cm.perm_from_classes(want, colors)
            expect((o1.cpu().numpy() == w[0]).all() and (o2.cpu().numpy() == w[1]).all() and (ptr == w[2]).all(), "%s: the permutation" % P.name)
            expect(perm(classes=colors - 1) == sm.ERR_INVALID if colors > 1 else True, "%s: a class out of range" % P.name)
        with unmoved("%s: refused smvp_perm_from_classes calls make no counted call" % P.name):
            expect(status("smvp_perm_from_classes", 0, -1, colors, sm._dev_ptr(dcol), sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID, "n < 0")
            expect(status("smvp_perm_from_classes", 0, P.n, colors, None, sm._dev_ptr(o1), sm._dev_ptr(o2), None, None) == sm.ERR_INVALID, "NULL d_class")
        rs.sweep_call("smvp_perm_from_classes on %s" % P.name, perm, codes=(sm.ERR_ALLOC,))
        # B as a handle
        def create(p=o2):
            out = C.c_void_p()
            rc = status("smvp_csr_create_permuted", C.byref(out), A._h, sm._dev_ptr(p), None)
            return rc, out.value

        with balanced("%s: smvp_csr_create_permuted, products on B, smvp_csr_destroy" % P.name):
            B = A.permuted(o2)
            x, y, z = rs.dev(np.random.default_rng(4).random(P.n)), torch.empty(P.n, dtype=torch.float64, device="cuda"), torch.empty(P.n, dtype=torch.float64, device="cuda")
            B.spmv(x, y)
            held = snap()
            with unmoved("%s: smvp_vector_gather allocates nothing" % P.name):
                sm.vector_gather(o1, x, z)
                sm.vector_gather(o2, z, y)
                expect(status("smvp_vector_gather", 0, P.n, sm._dev_ptr(o1), sm._dev_ptr(x), sm._dev_ptr(x), None) == sm.ERR_INVALID, "overlap")
            torch.cuda.synchronize()
            expect(y.cpu().numpy().tobytes() == x.cpu().numpy().tobytes(), "%s: there and back" % P.name)
            require_same(held, snap(), "%s: gathers" % P.name)
            B.close()
        with balanced("%s: a refused permutation builds nothing" % P.name):
            bad = o2.clone()
            bad[3] = bad[4]
            rc, obj = create(bad)
            expect(rc == sm.ERR_INVALID and not obj, "%s: a repeated index gives status %d" % (P.name, rc))
        rs.sweep_create("smvp_csr_create_permuted on %s" % P.name, create, lambda h: sm.lib().smvp_csr_destroy(C.c_void_p(h)))
        At.close()
        A.close()
    with balanced("a matrix without rows"):
        E = sm.CsrMatrix(0, 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0))
        e = torch.empty(0, dtype=torch.int32, device="cuda")
        E.color(e)
        sm.perm_from_classes(e, 0)
        E.permuted(e).close()
        E.close()


def group_fresh():
    import torch

    from test_gpu_transposed import arrays_of

    def whole(P, at, seed):
        def run():
            A = sm.CsrMatrix(P.n, P.n, *P.csr)
            At = A.transposed() if at else None
            R = A.multicolored(At, seed)
            x = rs.dev(np.random.default_rng(6).standard_normal(P.n))
            xn, xo = torch.empty_like(x), torch.empty_like(x)
            R.to_new(x, xn)
            R.to_old(xn, xo)
            torch.cuda.synchronize()
            out = {"color_ptr": np.asarray(R.color_ptr), "old_of_new": R.old_of_new.cpu().numpy(), "new_of_old": R.new_of_old.cpu().numpy(),
                   "B": tuple(arrays_of(torch, R.matrix)), "x_new": xn.cpu().numpy(), "x_old": xo.cpu().numpy(),
                   "info": (R.info["colors"], R.info["largest_class"], R.info["smallest_class"], R.info["lanes_per_row"], R.info["entries"])}
            fm.arm(0)                                  # (the check, not the run under test)
            want, colors, _ = P.reference(at, seed)
            w = cm.perm_from_classes(want, colors)
            expect(R.colors == colors and (out["new_of_old"] == w[1]).all() and (out["color_ptr"] == w[2]).all(), "%s: the permutation" % P.name)
            for g, h in zip(out["B"], cm.permuted_csr(P.n, *P.csr, w[1])):
                expect(g.tobytes() == np.ascontiguousarray(h).tobytes(), "%s: B's arrays" % P.name)
            expect(out["x_old"].tobytes() == x.cpu().numpy().tobytes(), "%s: there and back" % P.name)
            R.close()
            if At is not None:
                At.close()
            A.close()
            return out
        return run

    for P in patterns():
        for at, seed in ((False, 0), (True, 0xffffffff)):
            fm.scenario("multicolored, %s, %s at, seed %#x" % (P.name, "with" if at else "without", seed), whole(P, at, seed))


GROUPS = {"resources": group_resources, "fresh": group_fresh}


def main(argv):
    import gc

    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: multicolor_scenarios.py {%s}" % " | ".join(GROUPS))
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
