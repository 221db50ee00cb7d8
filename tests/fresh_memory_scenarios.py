"""The scenarios of tests/test_gpu_fresh_memory.py: `python fresh_memory_scenarios.py GROUP` in a fresh process whose SMVP_LIB_PATH
names lib/libsmvp_amd_counted.so.  No result of the library may depend on what a fresh allocation of its own holds.

tests/resource_count.cpp routes every hipMalloc / hipHostMalloc of the library through a wrapper; smvp_test_fill_allocations arms
it to fill each new block before the library sees it: mode 1 = every 32-bit word 0x00000001, mode 2 = every byte 0xFF.  A
scenario builds its objects and calls them from scratch three times -- fill off, mode 1, mode 2 (mode 2 only after mode 1 has
passed: an index nobody wrote then reads 1 and shows as a wrong number before it could read -1) -- so everything the library
allocates for it is allocated under that mode.  Each run applies the check the path's own GPU test applies (the oracle's or the
numpy restatement's bits where the header promises bits, parity.check_y's bound where it promises none: TJDS ATOMIC and
ref-quirks, binned rows summed in bins), and everything a run hands back -- y / Y / x, step counts, reasons, result blocks and
histories, device arrays, schedules, plan_info -- must be the same value, bit for bit, in all three runs; only results whose
order of additions changes from run to run (keys that start with "~") and times are left out of that.  What torch allocates is not
filled (it calls the runtime itself): the operands and results are the tests' own and are poisoned and guarded as everywhere.

The purpose is wrong numbers, never faults.  An error of the device -- an SmvpError with SMVP_ERR_HIP, or anything torch raises
-- is no scenario's verdict: nothing is run after it, neither the scenario again nor the next one, and the process ends with
status 3.  A wrong number (a failed check, a difference between two runs, a refusal by the library) is a failure: it
names the scenario, the mode, how many obtaining calls the run had made and -- found by running the scenario again
with the fill limited to a window of allocation ordinals, halved until one is left -- the one allocation whose fill alone
reproduces it: that block is read before it is written, or a later block that got the same memory back after a free is
(ordinals count from 0 at the start of each run, device and pinned memory in one sequence).  By hand:
`python fresh_memory_scenarios.py GROUP --only TEXT --window FIRST LAST` runs the scenarios whose name contains TEXT and fills only
the obtaining calls FIRST ... LAST (LAST -1 = no end).

Where the scenarios depart from a plain cross product: the spill and corner matrices of the binned plan have a group of their
own (csr_large), so that no child comes near its time limit.  In group solvers the sizes are n = 1, 257, 1003 and TRIP + 1, but
at TRIP + 1 pcg_tri and the plan form of pbicgstab stand on diagonal-only plans (as test_gpu_pcg_tri.py does at that size) and
ILU(0) is not run: the restatement's triangular solves and factorisation are Python loops over the entries, minutes at half a
million rows.  Symmetric Gauss-Seidel and ILU(0) run at the three smaller sizes.

"group GROUP ok" is the last line of a run that passed.  Exit status 1 = a scenario failed (the process stops at the first), 2 =
usage, 3 = an error that is no scenario's verdict (the caller starts no further group after it).  `--observe FILE` (group csr)
appends what a fresh 1 MiB block held before and after the group's allocate / free traffic.
"""
import ctypes as C
import os
import sys
import time
import zlib

import numpy as np

STARTED = time.time()
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import resource_scenarios as rs      # noqa: E402  (sets the package's path; its matrices, plans and option helpers are reused)
import oracle_binding as ob          # noqa: E402
import smvp_toolkit_amd as sm        # noqa: E402
from parity import check_guards, check_y, guarded_y     # noqa: E402

Failed, expect, dev, options = rs.Failed, rs.expect, rs.dev, rs.options
MODES = (0, 1, 2)
MODE_NAMES = {0: "fill off", 1: "every word 0x00000001", 2: "every byte 0xFF"}
WINDOW = [0, -1]
ONLY = [None]
DONE, REFUSED = [], []


# ------------------------------------------------------------------------------------------------------------------ the switch
def lib():
    L = rs.lib()
    L.smvp_test_fill_allocations.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
    L.smvp_test_fill_stats.argtypes = [C.POINTER(C.c_longlong)]
    L.smvp_test_fill_stats.restype = None
    L.smvp_test_probe_fill.argtypes = [C.c_size_t, C.POINTER(C.c_ubyte)]
    return L


def arm(mode, first=0, last=-1):
    expect(lib().smvp_test_fill_allocations(mode, first, last) == 0, "smvp_test_fill_allocations(%d) was refused" % mode)


def stats():
    """(fills done, bytes filled, fills failed) since the process began."""
    v = (C.c_longlong * 3)()
    lib().smvp_test_fill_stats(v)
    return tuple(v)


def obtained():
    s = rs.snap()
    return rs.at(s, rs.DEVICE, rs.OBTAINS) + rs.at(s, rs.PINNED, rs.OBTAINS)


def probe(n):
    """What a fresh device allocation of n bytes holds when the library gets it."""
    out = (C.c_ubyte * max(n, 1))()
    rc = lib().smvp_test_probe_fill(n, out)
    expect(rc == 0, "smvp_test_probe_fill(%d): HIP error %d" % (n, rc))
    return np.frombuffer(out, dtype=np.uint8, count=n).copy()


def pattern(mode, n):
    return np.full(n, 0xFF, np.uint8) if mode == 2 else np.tile(np.array([1, 0, 0, 0], np.uint8), n // 4 + 1)[:n]


def probe_both_patterns():
    """The fill reaches device memory, byte for byte, a tail of 1 ... 3 bytes included: a silent no-op cannot pass."""
    for mode in (1, 2):
        for n in (1, 5, 4099):
            before = stats()
            arm(mode)
            got = probe(n)
            arm(0)
            after = stats()
            bad = np.flatnonzero(got != pattern(mode, n))
            expect(not len(bad), "probe of %d bytes, %s: byte %d is %#04x" % (n, MODE_NAMES[mode], bad[0] if len(bad) else -1,
                                                                          got[bad[0]] if len(bad) else 0))
            expect(after == (before[0] + 1, before[1] + n, before[2]), "probe of %d bytes, %s: the fill's counters went from %r to %r"
                   % (n, MODE_NAMES[mode], before, after))
    before = stats()
    probe(4099)
    expect(stats() == before, "the fill is off and an allocation was filled")
    DONE.append("the probe read back both patterns")


# ------------------------------------------------------------------------------------------------------------- comparing runs
def drop_times(d):
    return {k: v for k, v in d.items() if k != "build_ms"}


def differ(a, b, where=""):
    """'' or where two results differ; arrays and floats by their bits."""
    if isinstance(a, dict) and isinstance(b, dict):
        if set(a) != set(b):
            return "%s: keys %r against %r" % (where, sorted(a), sorted(b))
        for k in a:
            if not str(k).startswith("~"):
                d = differ(a[k], b[k], "%s[%r]" % (where, k))
                if d:
                    return d
        return ""
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)):
        if len(a) != len(b):
            return "%s: %d values against %d" % (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            d = differ(x, y, "%s[%d]" % (where, i))
            if d:
                return d
        return ""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return "%s: %s %s against %s %s" % (where, a.dtype, a.shape, b.dtype, b.shape)
        if a.tobytes() != b.tobytes():
            fa, fb = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
            ne = np.flatnonzero((fa.view(np.uint8).reshape(a.size, -1) != fb.view(np.uint8).reshape(b.size, -1)).any(axis=1))
            return "%s: %d elements differ, first at %d: %r against %r" % (where, len(ne), ne[0], fa[ne[0]], fb[ne[0]])
        return ""
    if isinstance(a, float) and isinstance(b, float):
        return "" if np.float64(a).tobytes() == np.float64(b).tobytes() else "%s: %r against %r" % (where, a, b)
    return "" if a == b else "%s: %r against %r" % (where, a, b)


SCENARIO_ERRORS = (AssertionError, sm.SmvpError, ValueError)      # (Failed is an Exception of its own: caught by name below)


class DeviceError(Exception):
    """The GPU reported an error: no scenario's verdict.  Nothing is run after it -- no narrowing, no further scenario; main ends
    the process with status 3 and the caller starts no further group."""


def wrong_number(e, what):
    """The text of a scenario's failure -- a wrong number: a failed check, a refusal by the library -- after making sure that
    it is one.  A HIP error is none: the library reports every one of them, a fault that comes out of a synchronise included, as
    SMVP_ERR_HIP, and the helpers of the other GPU tests turn a status into an AssertionError, so the device is asked as well (a
    fault is sticky: the synchronise raises out of torch, which nothing here catches).  Either way it ends the process."""
    import torch

    if isinstance(e, sm.SmvpError) and e.code == sm.ERR_HIP:
        raise DeviceError("%s: %s" % (what, e))
    torch.cuda.synchronize()
    return "%s: %s" % (type(e).__name__, e)


def narrowed(run, mode, first, calls):
    """The ordinal of the one obtaining call whose fill makes run() give a wrong number under `mode`, by halving the window; None
    where no single one does (the result depends on several blocks, or only on their combination).  Called only after a wrong
    number, never after an error of the device, and an error of the device in one of its runs ends it (wrong_number)."""
    import torch

    def fails(lo, hi):
        arm(mode, lo, hi)
        try:
            out = run()
            torch.cuda.synchronize()
            return bool(differ(first, out))
        except SCENARIO_ERRORS + (Failed,) as e:
            wrong_number(e, "narrowing to ordinals %d ... %d" % (lo, hi))
            return True
        finally:
            arm(0)

    lo, hi = 0, calls - 1
    if hi < 0 or not fails(lo, hi):
        return None
    while lo < hi:
        mid = (lo + hi) // 2
        if fails(lo, mid):
            hi = mid
        elif fails(mid + 1, hi):
            lo = mid + 1
        else:
            return None
    return lo


def scenario(what, run):
    """run() builds its objects from scratch, calls them, checks them as their own GPU test does and returns what they handed
    back; it runs under each mode in turn."""
    import torch

    if ONLY[0] is not None and ONLY[0] not in what:
        return
    first = None
    for mode in MODES:
        before, calls = stats(), obtained()
        arm(mode, WINDOW[0], WINDOW[1])
        problem = None
        try:
            out = run()
            torch.cuda.synchronize()
        except SCENARIO_ERRORS + (Failed,) as e:
            problem = wrong_number(e, "%s, %s" % (what, MODE_NAMES[mode]))
        finally:
            arm(0)
        made = obtained() - calls
        if problem is None and mode:
            d = differ(first, out)
            problem = "differs from the run with the fill off at " + d if d else None
        if problem is not None:
            where = ""
            if mode and WINDOW == [0, -1]:
                one = narrowed(run, mode, first, made)
                where = "; no single allocation's fill reproduces it" if one is None else \
                    ("; filling allocation ordinal %d of the run alone reproduces it (--only ... --window %d %d): that block, or a later one "
                     "that got its memory back after a free, is read before it is written" % (one, one, one))
            raise Failed("%s, %s (%d obtaining calls in the run): %s%s" % (what, MODE_NAMES[mode], made, problem, where))
        after = stats()
        expect(after[2] == before[2], "%s, %s: %d fills failed" % (what, MODE_NAMES[mode], after[2] - before[2]))
        if mode and WINDOW == [0, -1]:
            expect(after[0] > before[0], "%s, %s: the library obtained %d blocks and none was filled" % (what, MODE_NAMES[mode], made))
        if mode == 0:
            expect(after[0] == before[0], "%s: a block was filled with the fill off" % what)
            first = out
    DONE.append(what)


def unfilled(call, what):
    """call() with the fill armed by the caller: it obtains nothing, so the fill's counters must not move."""
    before, calls = stats(), obtained()
    out = call()
    expect(stats() == before and obtained() == calls, "%s allocates nothing, and the counters moved from %r to %r" % (what, before, stats()))
    return out


# --------------------------------------------------------------------------------------------------------------- CSR sources
class Source:
    """A matrix, an operand and the reference of y = A x, computed once and left unchanged.  exact: integer operands whose sums
    are exact in any order (mixed_structures): every path gives the reference's bits."""

    def __init__(self, label, rows, cols, csr, x, row0=0, ref=None, exact=False, sorted_rows=False):
        self.label, self.rows, self.cols, self.csr, self.row0, self.exact, self.sorted_rows = label, rows, cols, csr, row0, exact, sorted_rows
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        rp, ci, v = csr
        self.ref = ob.csr_spmv(rp, ci, v, self.x) if ref is None else ref
        self.scale = ob.csr_spmv(rp, ci, np.abs(v), np.abs(self.x))
        self.terms = np.diff(rp)
        for a in (self.x, self.ref, self.scale):
            a.setflags(write=False)

    def check(self, y, what, serial=False):
        from special_values import check_bits

        if self.exact:
            check_bits(y, self.ref, what)
        else:
            check_y(y, self.ref, self.scale, self.terms, exact=serial and self.sorted_rows)


def sample_source(name):
    m, n, coo, csr = rs.sample(name + ".mtx")
    return Source(name, m, n, csr, np.random.default_rng(67890).random(n), sorted_rows=True)


def small_sources():
    import mixed_structures as ms
    import special_values as sv
    import spmm_cases as sc

    yield sample_source("ibm32")
    yield sample_source("memplus")
    name = ms.BLOCKS[0]
    rows, cols, row0, _ = ms.structure(name)
    coo, x, _ = ms.operands(name, "exact")
    yield Source("mixed " + name, rows, cols, ms.csr_of(name, coo), x, row0=row0, ref=ms.reference(name), exact=True)
    fz = sc.block_fuzz(3)
    yield Source("spmm fuzz 3", fz[0], fz[1], fz[2:5], np.random.default_rng(3).standard_normal(fz[1]))
    for name in sv.SMALL:
        if name.startswith("edge:"):
            rows, cols, rp, ci, _ = sv.structure(name)
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            yield Source(name, rows, cols, (rp, ci, rng.uniform(-1, 1, len(ci))), rng.random(cols), sorted_rows=True)


def large_sources():
    """The matrices of test_binned_spill_paths and test_binned_corner_structures with the bands those tests multiply them at:
    (Source, bands)."""
    import parity

    for kind in parity.SPILL_KINDS:
        rows, cols, band, rp, ci, v = parity.spill_matrix(kind)
        yield Source("spill " + kind, rows, cols, (rp, ci, v), np.random.default_rng(404).standard_normal(cols)), (band,)
    for name, rows, cols, bands, rp, ci, v, x in parity.corner_structures():
        yield Source("corner " + name, rows, cols, (rp, ci, v), x), bands


def binned_plans(bands):
    for band in bands:
        for near in (0, 1):
            for overlap in (0, 1):
                yield "BINNED band %d near=%d overlap=%d" % (band, near, overlap), {"binned_near": near, "binned_overlap": overlap}, sm.CSR_KERNEL_BINNED, band


def other_family(plan):
    """A plan of another kernel family, to re-plan to and back from."""
    if plan[2] == sm.CSR_KERNEL_VECTOR:
        return "STREAM 1024", {}, sm.CSR_KERNEL_STREAM, 1024
    return "VECTOR", {}, sm.CSR_KERNEL_VECTOR, 0


def csr_products(torch, A, src, dx, what, serial):
    """Two products (the tile kernel's sweep direction alternates) into guarded, poisoned y."""
    out = []
    for i in range(2):
        buf, dy = guarded_y(torch, src.rows)
        A.spmv(dx, dy)
        torch.cuda.synchronize()
        check_guards(buf, src.rows)
        y = dy.cpu().numpy()
        src.check(y, "%s, product %d" % (what, i + 1), serial)
        out.append(y)
    return out


def csr_scenario(torch, src, plan, dx):
    other = other_family(plan)
    serial = plan[0] == "COLSWEEP"                 # the column sweep without parts sums a sorted row left to right: the serial loop's bits
    what = "csr %s, %s" % (src.label, plan[0])

    def run():
        out = {}
        A = sm.CsrMatrix(src.rows, src.cols, *src.csr, first_row=src.row0)
        try:
            for leg in ("planned", "planned again after %s" % other[0]):
                try:
                    rs.set_plan(A, plan)
                except sm.SmvpError as e:
                    if e.code != sm.ERR_UNSUPPORTED:
                        raise
                    out[leg] = "refused as unsupported"
                    if what not in REFUSED:
                        REFUSED.append(what)
                    continue
                out[leg] = (A.get_kernel(), A.describe()[0], A.launches(), drop_times(A.plan_info()), csr_products(torch, A, src, dx, what + ", " + leg, serial))
                rs.set_plan(A, other)
                out[leg + ", the other family"] = csr_products(torch, A, src, dx, "%s, %s, then %s" % (what, leg, other[0]), False)
        finally:
            A.close()
        return out

    scenario(what, run)


def zero_share(block):
    return float((block == 0).mean())


def group_csr(observe=None):
    import torch

    seen = []
    if observe:
        seen.append(("at process start", zero_share(probe(1 << 20))))
    for src in small_sources():
        dx = dev(src.x)
        plans = list(rs.csr_plans(src.rows)) + list(binned_plans((0, 1, 3, 100)))
        for plan in plans:
            csr_scenario(torch, src, plan, dx)
        del dx
    if observe:
        seen.append(("after the allocate / free traffic of the small matrices of group csr", zero_share(probe(1 << 20))))
        with open(observe, "a") as f:
            for when, share in seen:
                f.write("%s: %.6f of the bytes of a fresh 1 MiB block are zero\n" % (when, share))


def group_csr_large():
    """The spill and corner matrices have a process of their own: millions of entries each, and the bands their own tests use
    on top of the others'."""
    import torch

    for src, bands in large_sources():
        dx = dev(src.x)
        for plan in list(rs.csr_plans(src.rows)) + list(binned_plans(sorted(set((0, 1, 3, 100) + tuple(bands))))):
            csr_scenario(torch, src, plan, dx)
        del dx
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------- TJDS
def tjds_sources():
    """(label, rows, cols, coo, t, Source of the same entries, (reference, scale, terms) of the ref-quirks product or None: the
    reference's quirks need a square matrix)."""
    import mixed_structures as ms
    import test_gpu_parity as gp

    for name in ("ibm32", "memplus"):
        m, n, coo, csr = rs.sample(name + ".mtx")
        src = Source(name, m, n, csr, np.random.default_rng(67890).random(n), sorted_rows=True)
        quirky = ob.tjds_spmv(ob.tjds_build(coo, m, n), src.x, refquirks=True)
        yield name, m, n, coo, sm.tjds_from_coo(coo, m, n), src, (quirky,) + tuple(gp.refquirks_yardsticks(coo, m, n, src.x))
    # repeated pairs and more columns than rows; more rows than columns (x_perm has max(rows, cols) elements of which set_x writes
    # `cols`).  Exact operands: every order of ATOMIC's adds gives the same bits.  (The ref-quirks product reads its operand by row
    # and is refused on a matrix that is not square.)
    for name in (ms.WHOLE[2], "tall:0"):
        rows, cols, _, _ = ms.structure(name)
        coo, x, _ = ms.operands(name, "exact")
        src = Source("mixed " + name, rows, cols, ms.csr_of(name, coo), x, ref=ms.reference(name), exact=True)
        yield "mixed " + name, rows, cols, coo, sm.tjds_from_coo(coo, rows, cols), src, None


def tjds_scenario(torch, label, t, src, quirk_yardsticks, mode, index, tile, cache, quirks, dx):
    what = "tjds %s, mode %d, tjds_index %d, tile %d, value cache %d, ref-quirks %s" % (label, mode, index, tile, cache, "on" if quirks else "off")
    reproducible = mode != sm.TJDS_MODE_ATOMIC and not quirks       # (ref-quirks always runs the atomic form)
    same_bits_anyway = reproducible or src.exact                     # integer operands: every order of the adds gives the same bits
    def run():
        out = {}
        with options({"tjds_index": index}):
            T = sm.TjdsMatrix(t)
        try:
            T.set_mode(mode)
            if tile:
                T.set_tile(tile)
            if cache:
                T.set_value_cache(cache)
            if quirks:
                T.set_ref_quirks(True)
            out["describe"], out["plan_info"] = T.describe()[0], drop_times(T.plan_info())
            for zero in (True, False) if reproducible else (True,):
                buf, dy = guarded_y(torch, src.rows)
                T.set_x(dx)
                if zero:
                    T.zero_y(dy)
                T.spmv(dy)
                torch.cuda.synchronize()
                check_guards(buf, src.rows)
                y = dy.cpu().numpy()
                if quirks:
                    check_y(y, *quirk_yardsticks)
                else:
                    src.check(y, what)
                out[("y" if same_bits_anyway else "~y") + (" after zero_y" if zero else " without zero_y")] = y
            if reproducible:
                expect(not differ(out["y after zero_y"], out["y without zero_y"]), what + ": the product depends on zero_y where the mode needs none")
        finally:
            T.close()
        return out

    scenario(what, run)


def group_tjds():
    import torch

    import spmm_cases as sc
    import test_gpu_spmm_transposed as k9m
    import test_gpu_tjds_spmm as k10m
    import test_gpu_transposed as k8m
    import tjds_spmm
    import transposed as tr

    for label, rows, cols, coo, t, src, yard in tjds_sources():
        dx = dev(src.x)
        for quirks in (False, True) if yard is not None else (False,):
            for index in (0, 1, 2):
                for tile in (0, 256, 1024, 2048):
                    for cache in (0, 2):
                        if index == 2 and cache:           # 32-bit columns in row order: no tile-ordered stream, no cache (refused)
                            continue
                        tjds_scenario(torch, label, t, src, yard, sm.TJDS_MODE_ROW_GATHER, index, tile, cache, quirks, dx)
                for mode in (sm.TJDS_MODE_TWO_PHASE, sm.TJDS_MODE_ATOMIC):
                    tjds_scenario(torch, label, t, src, yard, mode, index, 0, 0, quirks, dx)
    # K10's plan (built by the first smvp_tjds_spmm), and K8 / K9, which work on the handle's own arrays and obtain nothing
    fz = sc.block_fuzz(3)
    rows, cols = fz[0], fz[1]
    coo = sm.coo_from_csr(rows, *fz[2:5])
    t = sm.tjds_from_coo(coo, rows, cols)
    rng = np.random.default_rng(61)
    for k in (1, 3, 17):
        X, Xr = rng.standard_normal((cols, k)), rng.standard_normal((rows, k))
        ref10, ref9 = tjds_spmm.reference_block(t, X), k9m.reference_block(coo, rows, cols, Xr)
        ref8 = tr.reference(coo, rows, cols, Xr[:, 0].copy())

        def run_k10():
            T = sm.TjdsMatrix(t)
            try:
                Y = k10m.k10(torch, T, X)
                tjds_spmm.assert_block(Y, ref10, "K10, k = %d" % k)
                Y2 = k10m.k10(torch, T, X, ldx=k + 3, ldy=k + 2)          # the plan is there now
                tjds_spmm.assert_block(Y2, ref10, "K10 again, k = %d" % k)
                return {"Y": Y, "Y again": Y2, "describe": T.spmm_describe(k)[0], "plan": drop_times(T.spmm_describe(k)[2])}
            finally:
                T.close()

        def run_k8_k9():
            T = sm.TjdsMatrix(t)
            try:
                y = unfilled(lambda: k8m.k8(torch, T, Xr[:, 0].copy()), "K8 (smvp_tjds_spmv_transposed)")
                tr.assert_bits(y, ref8, "K8")
                Y = unfilled(lambda: k9m.k9(torch, T, Xr), "K9 (smvp_tjds_spmm_transposed), k = %d" % k)
                k9m.assert_block(Y, ref9, "K9, k = %d" % k)
                return {"y": y, "Y": Y}
            finally:
                T.close()

        scenario("tjds spmm fuzz 3: K10 and its plan, k = %d" % k, run_k10)
        scenario("tjds spmm fuzz 3: K8 and K9 obtain nothing, k = %d" % k, run_k8_k9)


# ------------------------------------------------------------------------------------------------------------ the other objects
def coo_bytes(coo):
    raw = np.ascontiguousarray(coo, dtype=sm.COO_DTYPE).view(np.uint8)
    return dev(raw) if raw.size else dev(np.zeros(16, np.uint8))


def group_objects():
    import torch

    import ilu0_method as im
    import mixed_structures as ms
    import spmm_cases as sc
    import test_gpu_ilu0 as k17
    import test_gpu_spmm as k7m
    import test_gpu_transposed as k8m
    import test_gpu_trsv as k15
    import transposed as tr
    import trsv_method as tm

    # ---- create_transposed: the arrays it builds on the device, and products on the new handle
    for name in ("ibm32", "memplus"):
        m, n, coo, csr = rs.sample(name + ".mtx")
        xr = np.random.default_rng(5).standard_normal(m)
        want, ref = tr.transposed_csr(coo, n), tr.reference(coo, m, n, xr)
        scale = ob.csr_spmv(want[0], want[1], np.abs(want[2]), np.abs(xr))

        def run_transposed():
            A = sm.CsrMatrix(m, n, *csr)
            At = A.transposed()
            try:
                arrays = k8m.arrays_of(torch, At)
                k8m.assert_arrays(arrays, want, name)
                A.close()                                              # the transposed handle outlives its source
                y1 = k8m.spmm1(torch, At, xr)
                tr.assert_bits(y1, ref, name + ": spmm k = 1 on the transposed handle")
                y = k8m.spmv(torch, At, xr)
                check_y(y, ref, scale, np.diff(want[0]))
                return {"arrays": arrays, "spmm k = 1": y1, "spmv": y, "kernel": At.get_kernel(), "plan": drop_times(At.plan_info())}
            finally:
                At.close()
                A.close()

        scenario("create_transposed of %s" % name, run_transposed)
    # ---- the device converters on sorted, shuffled and repeated COO
    m, n, coo, _ = rs.sample("memplus.mtx")
    rep = ms.WHOLE[2]
    rrows, rcols, _, rcoo = ms.structure(rep)
    inputs = [("memplus, sorted", m, n, np.sort(coo, order=["row", "col"])),
              ("memplus, shuffled", m, n, coo[np.random.default_rng(8).permutation(len(coo))]),
              ("mixed %s, repeated pairs" % rep, rrows, rcols, rcoo)]
    for label, rows, cols, entries in inputs:
        hrp, hci, hv = sm.csr_from_coo(entries, rows)
        h = sm.tjds_from_coo(entries, rows, cols)

        def run_csr_converter():
            d_coo = coo_bytes(entries)
            before = d_coo.clone()
            rp, ci, v = sm.csr_from_coo_device(d_coo, rows, cols, len(entries))
            torch.cuda.synchronize()
            out = {"row_ptr": rp.cpu().numpy(), "col_ind": ci.cpu().numpy(), "val": v.cpu().numpy()}
            assert np.array_equal(out["row_ptr"], hrp) and np.array_equal(out["col_ind"][:len(hci)], hci), "row_ptr / col_ind differ from the host converter's"
            assert out["val"][:len(hv)].tobytes() == hv.tobytes(), "val differs from the host converter's"
            assert torch.equal(d_coo, before), "the input was modified"
            return out

        def run_tjds_converter():
            d_coo = coo_bytes(entries)
            before = d_coo.clone()
            t = sm.tjds_from_coo_device(d_coo, rows, cols, len(entries))
            torch.cuda.synchronize()
            assert (t.num_diag, t.ref_num_tjdiag, t.last_diag_single) == (h.num_diag, h.ref_num_tjdiag, h.last_diag_single)
            out = {"counts": (t.num_diag, t.ref_num_tjdiag, t.last_diag_single)}
            for f in ("perm", "start_pos", "row_ind", "val"):
                out[f] = getattr(t, f).cpu().numpy()
                want = getattr(h, f)
                assert out[f][:len(want)].tobytes() == np.ascontiguousarray(want).tobytes(), f + " differs from the host converter's"
            assert torch.equal(d_coo, before), "the input was modified"
            return out

        scenario("csr_from_coo_device on %s" % label, run_csr_converter)
        scenario("tjds_from_coo_device on %s" % label, run_tjds_converter)
    # ---- K7 (smvp_csr_spmm): its plan is built by the first call
    fz = sc.block_fuzz(3)
    rows, cols, (rp, ci, v) = fz[0], fz[1], fz[2:5]
    rng = np.random.default_rng(62)
    for k in (1, 3, 17):
        X = rng.standard_normal((cols, k))
        ref = k7m.oracle(rp, ci, v, X)

        def run_k7():
            A = sm.CsrMatrix(rows, cols, rp, ci, v)
            try:
                Y = k7m.spmm(torch, A, X, k, k, k)
                k7m.assert_bits(Y, ref, "K7, k = %d" % k)
                Y2 = k7m.spmm(torch, A, X, k, k + 3, k + 2)
                k7m.assert_bits(Y2, ref, "K7 again, k = %d" % k)
                return {"Y": Y, "Y again": Y2, "describe": A.spmm_describe(k)[0], "plan": drop_times(A.spmm_describe(k)[2])}
            finally:
                A.close()

        scenario("csr spmm fuzz 3: K7 and its plan, k = %d" % k, run_k7)
    # ---- gather_spread and far_share (sampled and counted on the device at create)
    name = ms.BLOCKS[0]
    brows, bcols, brow0, _ = ms.structure(name)
    bcsr, share = ms.csr_of(name), ms.regime(name)["far_share"]

    def run_shares():
        A = sm.CsrMatrix(brows, bcols, *bcsr, first_row=brow0)
        try:
            far, spread = A.far_share(), A.gather_spread()
            assert abs(far - share) <= 1e-6, (far, share)
            assert spread == -1.0 or 0.0 <= spread <= 1.0, spread
            return {"far_share": far, "gather_spread": spread, "kernel": A.get_kernel()}
        finally:
            A.close()

    scenario("gather_spread and far_share of mixed %s" % name, run_shares)
    # ---- trsv_plan: both triangles, both diagonal settings, chain widths 1x and 4x, with solves
    w = k15.chain_width()
    for M in (tm.wide_thin_wide(w), tm.sample("memplus")):
        for width in (w, 4 * w):
            for uplo in (sm.TRSV_LOWER, sm.TRSV_UPPER):
                for diag in (sm.TRSV_DIAG_STORED, sm.TRSV_DIAG_UNIT):
                    def run_trsv():
                        with options({"trsv_chain_width": width}):
                            H = k15.handle_of(M)
                            try:
                                P = H.trsv_plan(uplo, diag)
                                level_ptr, order = P.schedule()
                                info = drop_times(P.info())
                                P.close()
                                b, want = M.reference(uplo, diag)
                                P = H.trsv_plan(uplo, diag)
                                x = k15.solve_once(torch, P, M.n, b)
                                P.close()
                                checked = drop_times(k15.check_plan(torch, H, M, uplo, diag, calls=("again",)))
                                tr.assert_bits(x, want, M.name)
                                assert info == checked and info["chain_width"] == width
                                return {"level_ptr": level_ptr, "order": order, "info": info, "x": x}
                            finally:
                                H.close()

                    scenario("trsv_plan on %s, uplo %d, diag %d, chain width %d" % (M.name, uplo, diag, width), run_trsv)
    # ---- ilu0(): the factor, factor() twice over, both solves
    for i in (9, 0):
        M = im.case(w, i)
        want = im.factor(M).csr[2]
        F = im.factor(M)
        b = tm.rhs(M.n)

        def run_ilu0():
            H = k17.handle_of(M)
            f = H.ilu0()
            try:
                out = {"after create": k17.values_of(torch, f)}
                tr.assert_bits(out["after create"], want, M.name + ": after create")
                for again in (1, 2):
                    f.factor()
                    out["factor() %d" % again] = k17.values_of(torch, f)
                    tr.assert_bits(out["factor() %d" % again], want, M.name + ": factor() again")
                out["matrix"] = k8m.arrays_of(torch, f.matrix)
                out["info"] = drop_times(f.info())
                L, U = f.plans()
                try:
                    out["schedules"] = (L.schedule(), U.schedule(), drop_times(L.info()), drop_times(U.info()))
                    y = k17.solve_once(torch, L, M.n, b)
                    tr.assert_bits(y, tm.solve(F, tm.LOWER, tm.UNIT, b), M.name + ": the LOWER / UNIT solve")
                    x = k17.solve_once(torch, U, M.n, y)
                    tr.assert_bits(x, tm.solve(F, tm.UPPER, tm.STORED, y), M.name + ": the UPPER / STORED solve")
                    out["solves"] = (y, x)
                finally:
                    L.close()
                    U.close()
                return out
            finally:
                f.close()
                H.close()

        scenario("ilu0 of %s: create, factor() twice, both solves" % M.name, run_ilu0)
    # ---- the timed entry points: per-call scratch, the timing rings, the repeating kernel at -n 1000
    m, n, coo, csr = rs.sample("ibm32.mtx")
    ones_ref = ob.csr_spmv(*csr, np.ones(n))
    for fn in (sm.csr_compute, sm.tjds_compute):
        for timing in (sm.TIMING_EVENTS, sm.TIMING_DEVICE):
            for iters in (3, 1000):
                def run_timed():
                    y, ms_, st = fn(coo, m, n, iters=iters, timing=timing)
                    info = sm.last_run_info()
                    assert np.array_equal(y, ones_ref), "y differs from the oracle's (a pattern matrix: exact)"
                    assert len(ms_) == iters and np.all(ms_ > 0) and np.all(np.isfinite(ms_)), "a product without a time of its own"
                    assert info.timing == timing
                    return {"y": y, "how": (info.timing, info.repeat_launches, info.repeat_gave_up, info.graph_replays)}

                scenario("%s on ibm32, timing %d, -n %d" % (fn.__name__, timing, iters), run_timed)
    # ---- three virtual ranks on one GPU, both push forms
    m, n, coo, csr = rs.sample("memplus.mtx")
    x = np.random.default_rng(4).random(n)
    ref = ob.csr_spmv(*csr, x)
    scale, terms = ob.csr_spmv(csr[0], csr[1], np.abs(csr[2]), np.abs(x)), np.diff(csr[0])
    for fmt in ("csr", "tjds"):
        for exchange in (sm.EXCHANGE_COPIES, sm.EXCHANGE_DIRECT):
            def run_sharded():
                S = sm.ShardedMatrix(fmt, 3, m, n, coo=coo, csr=csr, devices=[0, 0, 0], chunks=2, exchange=exchange)
                try:
                    S.set_x(x)
                    out = {}
                    for gather in (sm.GATHER_OVERLAPPED, sm.GATHER_AFTER):
                        for _ in range(2):                       # back to back: the full vectors are written again
                            S.spmv(allgather=gather)
                        S.synchronize()
                        for slot in range(3):
                            y = S.get_y(slot, gathered=True)
                            check_y(y, ref, scale, terms)
                            out["gather %d, rank %d" % (gather, slot)] = y
                    S.spmv(allgather=sm.GATHER_OVERLAPPED)
                    S.feed_back(normalize=True)
                    S.spmv(allgather=sm.GATHER_OVERLAPPED)
                    S.synchronize()
                    out["after feed_back"] = S.get_y(2, gathered=True)
                    assert np.isfinite(out["after feed_back"]).all()
                    out["layout"] = [np.asarray(a) if hasattr(a, "__len__") else a for a in S.layout()]
                    return out
                finally:
                    S.close()

            scenario("sharded %s, 3 virtual ranks, exchange %s" % (fmt, sm.EXCHANGE_NAMES[exchange]), run_sharded)


# ------------------------------------------------------------------------------------------------------------------ the solvers
def group_solvers():
    """Every solver against its numpy restatement, whose product argument is the same handle's single product (built under the
    same mode), bit for bit -- through the helpers of the solvers' own GPU tests, which poison the histories and d_x and check
    that nothing beyond the filled elements is written.  A run that stops early leaves history slots and work space unwritten."""
    import torch

    import bicgstab_method as bi
    import cg_method as cg
    import pbicgstab_method as pb
    import pcg_method as pcg
    import pcg_tri_method as tri
    import power_iteration as pi
    import power_method as pm
    import test_gpu_bicgstab as k13
    import test_gpu_cg as k12
    import test_gpu_pbicgstab as k18
    import test_gpu_pcg as k14
    import test_gpu_pcg_tri as k16
    import test_gpu_power_method as k11
    import trsv_method as trsv
    from transposed import assert_bits

    BOTH = k12.BOTH                                   # CSR AUTO and TJDS ROW_GATHER
    SIZES = (1, 257, 1003, cg.TRIP + 1)
    EVERY = (1, 3)

    def tag(fmt, every):
        return "%s, check_every %d" % ("CSR AUTO" if fmt == "csr" else "TJDS ROW_GATHER", every)

    # ---- the order-defined dot
    for n in SIZES:
        a, b = k12.dot_operands(n)
        want = cg.dot(a, b)

        def run_dot():
            da, db = dev(a), dev(b)
            got = [sm.vector_dot(da, db), sm.vector_dot(da, db), sm.vector_dot(da, da)]
            assert_bits(got[:2], [want, want], "smvp_vector_dot, n = %d" % n)
            assert_bits(got[2:], [cg.dot(a, a)], "a vector with itself")
            return [float(g) for g in got]

        scenario("vector_dot, n = %d" % n, run_dot)

    # ---- one scenario per (solver, system, handle, check_every): the handle, its plans and the call's work space are new each time.
    # The restatement is a function of what the handle's product gives it and of nothing else, and its serial triangular solves take
    # seconds: it runs once per (system, handle), with the operands and results of its products kept; a later run first holds its
    # own handle's product to those, bit for bit -- its restatement would then be the same numbers -- and fails if one differs.
    # The key is the scenario's name and the handle: check_every is no argument of these restatements (the power method's takes it,
    # and has it in its key), and of the plans P a restatement reads host data only, the same in every run -- the Cases' arrays,
    # m, and for ILU(0) ilu0_method's own factor of the Case (Plans.triples), never the factor the device made.  A device factor
    # that a fill has changed therefore shows as got != want, not as another reference.
    restated = {}

    def restatement(key, product, compute):
        if key not in restated:
            log = []

            def logged(x):
                y = product(x)
                log.append((np.array(x, dtype=np.float64, copy=True), y.copy()))
                return y

            restated[key] = (log, compute(logged))
        log, want = restated[key]
        for x, y in log:
            d = differ(product(x), y)
            expect(not d, "%s: a product of this run's handle differs from the same product of the first run%s" % (key, d))
        return want

    def solver_scenario(what, M, build, restate, call, same):
        for fmt, a, b in BOTH:
            for every in EVERY:
                def run():
                    H, product = k12.handle(torch, M, fmt, a, b)
                    P = build() if build else None
                    try:
                        got = call(H, P, every)
                        same(got, restatement("%s, %s" % (what, fmt), product, lambda prod: restate(prod, P)), what)
                        return got
                    finally:
                        if P is not None:
                            P.close()
                        H.close()

                scenario("%s, %s" % (what, tag(fmt, every)), run)

    for n in SIZES:
        big = n > 100000                              # one element past the first trip of the vector passes' grid: a few steps at tol 0
        steps, tol = (3, 0.0) if big else (30, 1e-10)
        M = k12.matrix("spd", n, 20280 + n) if n < 300 else k12.matrix("spd", n)
        rhs, x0 = cg.rhs(n), k12.start_vector(n)
        N = k13.matrix("nonsym", n, 20290 + n) if n < 300 else k13.matrix("nonsym", n)
        rhs_n = bi.rhs(n)
        jac = pcg.diagonal(M)
        for start, sname in ((None, "x0 NULL"), (x0, "an x0")):
            solver_scenario("cg on spd(%d), %s" % (n, sname), M, None,
                            lambda product, P, start=start: cg.run(product, rhs, start, steps, tol),
                            lambda H, P, every, start=start: k12.solve(torch, H, n, rhs, start, steps, tol, every),
                            lambda g, w, what: k12.same(g, w, what, rhs))
        solver_scenario("pcg (Jacobi) on spd(%d)" % n, M, None,
                        lambda product, P: pcg.run(product, rhs, None, jac, steps, tol),
                        lambda H, P, every: k14.solve(torch, H, n, rhs, jac, None, steps, tol, every),
                        lambda g, w, what: k14.same(g, w, what, rhs))
        solver_scenario("bicgstab on nonsym(%d)" % n, N, None,
                        lambda product, P: bi.run(product, rhs_n, None, steps, tol),
                        lambda H, P, every: k13.solve(torch, H, n, rhs_n, None, steps, tol, every),
                        lambda g, w, what: k13.same(g, w, what, rhs_n))
        # (the restatement's triangular solve is a Python loop over the entries: at the large size the plans stand on the diagonal alone,
        # as in test_gpu_pcg_tri.py -- the vector passes and their work space are what that size is for)
        Cs = None if big else trsv.of_matrix("spd(%d)" % n, M)
        tri_plans = tri.diagonal_only(jac) if big else tri.sgs(Cs)
        solver_scenario("pcg_tri (%s) on spd(%d)" % ("diagonal-only plans" if big else "SGS", n), M, lambda: k16.Plans(*tri_plans),
                        lambda product, P: P.run(product, rhs, None, steps, tol),
                        lambda H, P, every: k16.solve(torch, H, n, rhs, P, None, steps, tol, every),
                        lambda g, w, what: k16.same(g, w, what, rhs))
        Cn = trsv.of_matrix("nonsym(%d)" % n, N)
        for kind in ("jacobi", "diagonal-only plans" if big else "sgs"):
            build = (lambda: k18.Plans(*tri.diagonal_only(pcg.diagonal(N)))) if kind.startswith("diagonal") else (lambda kind=kind: k18.plans_of(torch, kind, Cn))
            solver_scenario("pbicgstab (%s) on nonsym(%d)" % (kind, n), N, build,
                            lambda product, P: P.run(product, rhs_n, None, steps, tol),
                            lambda H, P, every: k18.solve(torch, H, n, rhs_n, P, None, steps, tol, every),
                            lambda g, w, what: k18.same(g, w, what, rhs_n))
        E = k11.matrix("edge", n) if n < 300 else M
        p0 = pi.ones(E)
        psteps = 4 if big else 9
        for fmt, a, b in BOTH:
            for every in EVERY:
                def run_power():
                    H, product = k11.handle(torch, E, fmt, a, b)
                    try:
                        got = k11.power(torch, H, n, p0, psteps, 1e-9, every)
                        want = restatement("power_method, n = %d, %s, check_every %d" % (n, fmt, every), product,
                                           lambda prod: pm.run(prod, p0, psteps, 1e-9, every))
                        k11.same(got, want, "power_method, n = %d" % n)
                        return got
                    finally:
                        H.close()

                scenario("power_method on a matrix of %d rows, %s" % (n, tag(fmt, every)), run_power)
    # pbicgstab with the library's own ILU(0), on systems that admit one (a stored diagonal in every row, columns ascending): the
    # coalesced nonsym(n) at the three sizes whose restatement -- a factorisation and four triangular solves a step, Python loops over
    # the entries -- takes seconds, and the convection-diffusion grid of test_gpu_pbicgstab.py (63 thin levels).  Not at TRIP + 1.
    for name in ["nonsym(%d), coalesced" % n for n in SIZES if n < 100000] + ["convdiff(32, 0.5)"]:
        M, Cs = pb.case_of(name)
        rhs_n = bi.rhs(M.n)
        solver_scenario("pbicgstab (ILU(0)) on %s" % name, M, lambda: k18.plans_of(torch, "ilu0", Cs),
                        lambda product, P: P.run(product, rhs_n, None, k18.MAX_STEPS, k18.TOL),
                        lambda H, P, every: k18.solve(torch, H, M.n, rhs_n, P, None, k18.MAX_STEPS, k18.TOL, every),
                        lambda g, w, what: k18.same(g, w, what, rhs_n))

    # ---- one run per stop rule (max_steps = 10, as the solvers' own tests run them)
    for name, M, rhs, tol, want in k12.stop_cases():
        solver_scenario("cg stop case '%s'" % name, M, None,
                        lambda product, P: cg.run(product, rhs, None, 10, tol),
                        lambda H, P, every: k12.solve(torch, H, M.n, rhs, None, 10, tol, every),
                        lambda g, w, what, want=want: (k12.same(g, w, what), expect(tuple(g[:3]) == want, "%s: ended with %r" % (what, g[:3]))))
    for name, M, rhs, m, tol, want in k14.stop_cases():
        solver_scenario("pcg stop case '%s'" % name, M, None,
                        lambda product, P: pcg.run(product, rhs, None, m, 10, tol),
                        lambda H, P, every: k14.solve(torch, H, M.n, rhs, m, None, 10, tol, every),
                        lambda g, w, what, want=want: (k14.same(g, w, what), expect(tuple(g[:3]) == want, "%s: ended with %r" % (what, g[:3]))))
    for name, M, rhs, tol, want, _ in k13.stop_cases():
        solver_scenario("bicgstab stop case '%s'" % name, M, None,
                        lambda product, P: bi.run(product, rhs, None, 10, tol),
                        lambda H, P, every: k13.solve(torch, H, M.n, rhs, None, 10, tol, every),
                        lambda g, w, what, want=want: (k13.same(g, w, what), expect(tuple(g[:4]) == want, "%s: ended with %r" % (what, g[:4]))))
    for name, M, rhs, triple, tol, want in tri.stop_cases():
        solver_scenario("pcg_tri stop case '%s'" % name, M, lambda triple=triple: k16.Plans(*triple),
                        lambda product, P: P.run(product, rhs, None, 10, tol),
                        lambda H, P, every: k16.solve(torch, H, M.n, rhs, P, None, 10, tol, every),
                        lambda g, w, what, want=want: (k16.same(g, w, what), expect(tuple(g[:3]) == want, "%s: ended with %r" % (what, g[:3]))))
    for name, M, rhs, triple, tol, want, _ in pb.stop_cases():
        solver_scenario("pbicgstab stop case '%s'" % name, M, lambda triple=triple: k18.Plans(*triple),
                        lambda product, P: P.run(product, rhs, None, 10, tol),
                        lambda H, P, every: k18.solve(torch, H, M.n, rhs, P, None, 10, tol, every),
                        lambda g, w, what, want=want: (k18.same(g, w, what), expect(tuple(g[:4]) == want, "%s: ended with %r" % (what, g[:4]))))
    for name, M, x0, want in k11.special_cases():
        for fmt, a, b in BOTH:
            for every in EVERY:
                def run_special():
                    H, product = k11.handle(torch, M, fmt, a, b)
                    try:
                        got = k11.power(torch, H, M.n, x0, 6, 0.0, every)
                        want_run = restatement("power special case '%s', %s, check_every %d" % (name, fmt, every), product,
                                               lambda prod: pm.run(prod, x0, 6, 0.0, every))
                        k11.same(got, want_run, "power special case '%s'" % name)
                        if want and every == 1:
                            assert got[:2] == want[:2] and (want[2] is None or got[2] == want[2]), got[:3]
                        return got
                    finally:
                        H.close()

                scenario("power special case '%s', %s" % (name, tag(fmt, every)), run_special)


GROUPS = {"csr": group_csr, "csr_large": group_csr_large, "tjds": group_tjds, "objects": group_objects, "solvers": group_solvers}


def main(argv):
    import torch

    args = list(argv[1:])
    observe = None
    try:
        if "--only" in args:
            i = args.index("--only")
            ONLY[0] = args[i + 1]
            del args[i:i + 2]
        if "--window" in args:
            i = args.index("--window")
            WINDOW[:] = [int(args[i + 1]), int(args[i + 2])]
            del args[i:i + 3]
        if "--observe" in args:
            i = args.index("--observe")
            observe = args[i + 1]
            del args[i:i + 2]
    except (IndexError, ValueError):
        args = []
    if len(args) != 1 or args[0] not in GROUPS or (observe and args[0] != "csr"):
        print("usage: fresh_memory_scenarios.py {%s} [--only TEXT] [--window FIRST LAST] [--observe FILE (group csr)]" % " | ".join(GROUPS))
        return 2
    if not hasattr(sm.lib(), "smvp_test_fill_allocations"):
        print("FAIL: %s is not the counted build (set SMVP_LIB_PATH to lib/libsmvp_amd_counted.so)" % sm.LIB_PATH)
        return 2
    assert torch.cuda.is_available(), "the scenarios need the GPU"
    torch.zeros(1, device="cuda")
    group, t0 = args[0], STARTED                     # (the seconds printed at the end include the imports)
    start, fills = rs.snap(), stats()
    try:
        if observe:
            group_csr(observe)                       # (the block at process start is read before anything else is allocated)
            probe_both_patterns()
        else:
            probe_both_patterns()
            GROUPS[group]()
        import gc

        gc.collect()
        torch.cuda.synchronize()
        end = stats()
        expect(end[2] == 0, "%d fills failed" % end[2])
        expect(end[0] > fills[0], "no allocation was filled in the whole group")
        rs.require_same(start, rs.snap(), "the whole group %s: everything obtained was given back" % group)
    except Failed as e:
        for what in DONE[-3:]:
            print("ok   " + what)
        print("FAIL " + str(e))
        return 1
    except Exception:                                # anything else (a HIP error out of torch, say) is a crash, not a failed scenario
        import traceback

        traceback.print_exc()
        print("CRASH in group %s after %d scenarios; the last: %r" % (group, len(DONE), DONE[-1:]))
        return 3
    for what in REFUSED:
        print("note: %s: the plan was refused as unsupported for this matrix under every mode alike" % what)
    print("%d scenarios, each under %s, in %.0f s; %d fills of %d bytes, %d failed" % (len(DONE), " / ".join(MODE_NAMES[m] for m in MODES),
                                                                                       time.time() - t0, end[0] - fills[0], end[1] - fills[1], end[2]))
    print("group %s ok" % group)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
