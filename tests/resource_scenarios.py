"""The scenarios of tests/test_gpu_resources.py: `python resource_scenarios.py GROUP` in a fresh process whose SMVP_LIB_PATH names
lib/libsmvp_amd_counted.so (tests/resource_count.cpp: the library's own objects with every HIP call that obtains or returns a
resource counted).  Every comparison is exact equality of counter snapshots; a scenario that fails prints what differs -- the kind
of resource, objects and bytes -- and ends the process with status 1.  "group GROUP ok" is the last line of a run that passed.

Not counted: what torch allocates (it calls the runtime itself), and the RCCL communicators of the sharded layer (reached through
dlopen()ed pointers, not through imported symbols).
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "smvp-toolkit_amd", "python"))
sys.path.insert(0, HERE)

import oracle_binding as ob           # noqa: E402
import smvp_toolkit_amd as sm         # noqa: E402

KINDS = ("device memory", "pinned host memory", "stream", "event", "graph", "graph exec")
DEVICE, PINNED, STREAM, EVENT, GRAPH, GRAPH_EXEC = range(6)
LIVE, BYTES, OBTAINS, RELEASES = range(4)
FOREIGN, REFUSED, N_VALUES = 24, 25, 26
# (graphs have no switch: where the timed run cannot have a graph it goes on with plain launches and succeeds, so there is no
# failure to hold it to; its graphs and graph execs are counted like everything else)
SWITCH = {DEVICE: "smvp_test_fail_device_alloc", PINNED: "smvp_test_fail_host_alloc", STREAM: "smvp_test_fail_stream_create",
          EVENT: "smvp_test_fail_event_create"}

DONE = []


class Failed(Exception):
    pass


def lib():
    L = sm.lib()
    L.smvp_test_resources.argtypes = [C.POINTER(C.c_longlong), C.c_int]
    return L


def snap():
    v = (C.c_longlong * N_VALUES)()
    assert lib().smvp_test_resources(v, N_VALUES) == N_VALUES
    return tuple(v)


def at(s, kind, what):
    return s[4 * kind + what]


def arm(kind, nth):
    getattr(lib(), SWITCH[kind])(int(nth))


def difference(before, after, counters=False):
    """What differs between two snapshots, in words ('' = nothing): live objects and bytes per kind and the foreign frees; with
    `counters` the calls as well."""
    out = []
    for k, name in enumerate(KINDS):
        dl, db = at(after, k, LIVE) - at(before, k, LIVE), at(after, k, BYTES) - at(before, k, BYTES)
        if dl or db:
            out.append("%s: %+d live object(s), %+d bytes" % (name, dl, db))
        if counters:
            do, dr = at(after, k, OBTAINS) - at(before, k, OBTAINS), at(after, k, RELEASES) - at(before, k, RELEASES)
            if do or dr:
                out.append("%s: %d obtaining and %d releasing call(s) made" % (name, do, dr))
    if after[FOREIGN] != before[FOREIGN]:
        out.append("%d foreign free(s): something the library never obtained was released" % (after[FOREIGN] - before[FOREIGN]))
    return "; ".join(out)


def require_same(before, after, what, counters=False):
    d = difference(before, after, counters)
    if d:
        raise Failed("%s: %s" % (what, d))


@contextlib.contextmanager
def balanced(what):
    """Everything taken inside the block is given back by its end, in every kind, with no foreign free."""
    import torch

    before = snap()
    yield
    torch.cuda.synchronize()
    require_same(before, snap(), what)
    DONE.append(what)


@contextlib.contextmanager
def unmoved(what):
    """Not one counted call is made inside the block."""
    before = snap()
    yield
    require_same(before, snap(), what, counters=True)
    DONE.append(what)


def expect(cond, what):
    if not cond:
        raise Failed(what)


def status(fn, *args):
    return getattr(sm.lib(), fn)(*args)


def last_error():
    return sm.lib().smvp_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------------------------------------ the matrices
def sample(name):
    """(rows, cols, coo, (row_ptr, col_ind, val)) of a golden sample."""
    _, m, n, coo = sm.mm_read_coo(ob.fixture_path(name))
    return m, n, coo, sm.csr_from_coo(coo, m)


def synth():
    M = 1 << 16
    rp, ci, v = sm.synth_csr(sm.SYNTH_MEMPLUS_SHAPED, 12345, M, M)
    coo = sm.make_coo(np.repeat(np.arange(M), np.diff(rp)), ci, v)
    return M, M, coo, (rp, ci, v)


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


def csr_product(A, x):
    import torch

    y = torch.full((max(A.rows, 1),), float("nan"), dtype=torch.float64, device="cuda")
    A.spmv(x, y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:A.rows]


def tjds_product(T, x):
    import torch

    y = torch.full((max(T.rows, 1),), float("nan"), dtype=torch.float64, device="cuda")
    T.set_x(x)
    T.zero_y(y)
    T.spmv(y)
    torch.cuda.synchronize()
    return y.cpu().numpy()[:T.rows]


def same_bits(a, b, what):
    expect(a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all(), "%s: the product's bits differ" % what)


# the plans of a CSR handle: (name, plan options, kernel, param).  STREAM_CARRY has no 256-entry tiles.
def csr_plans(rows):
    S = sm
    yield "VECTOR", {}, S.CSR_KERNEL_VECTOR, 0
    yield "VECTOR 8", {}, S.CSR_KERNEL_VECTOR, 8
    for tile in (0, 256, 1024, 2048):
        yield "STREAM %d" % tile, {}, S.CSR_KERNEL_STREAM, tile
    yield "STREAM 1024 col16=0", {"csr_col16": 0}, S.CSR_KERNEL_STREAM, 1024
    yield "STREAM 1024 rowrel=0", {"csr_rowrel": 0}, S.CSR_KERNEL_STREAM, 1024
    yield "STREAM 2048 col16=0 rowrel=0", {"csr_col16": 0, "csr_rowrel": 0}, S.CSR_KERNEL_STREAM, 2048
    for tile in (0, 1024, 2048):
        yield "STREAM_CARRY %d" % tile, {}, S.CSR_KERNEL_STREAM_CARRY, tile
    yield "COLSWEEP", {}, S.CSR_KERNEL_COLSWEEP, 0
    for parts in (2, 4, 8):
        yield "COLSWEEP parts %d" % parts, {}, S.CSR_KERNEL_COLSWEEP, sm.sweep_parts(1024, parts)
    for near in (0, 1):
        for overlap in (0, 1):
            yield "BINNED near=%d overlap=%d" % (near, overlap), {"binned_near": near, "binned_overlap": overlap}, S.CSR_KERNEL_BINNED, 0
    yield "AUTO", {}, S.CSR_KERNEL_AUTO, 0


@contextlib.contextmanager
def options(opts):
    for k, v in opts.items():
        sm.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            sm.set_option(k, None)


def set_plan(A, plan):
    _, opts, kernel, param = plan
    with options(opts):
        A.set_kernel(kernel, param)


# =========================================================================================================== group: csr life cycle
def make_csr(kind, rows, cols, csr, first_row=0):
    """A CsrMatrix over host arrays, or over adopted device arrays (kept by the wrapper)."""
    rp, ci, v = csr
    if kind == "host":
        return sm.CsrMatrix(rows, cols, rp, ci, v, first_row=first_row)
    return sm.CsrMatrix(rows, cols, dev(rp), dev(ci if len(ci) else np.zeros(4, np.int32)), dev(v if len(v) else np.zeros(4)),
                        first_row=first_row)


def group_csr():
    import torch

    import mixed_structures as ms
    import spmm_cases as sc

    sources = [("ibm32",) + sample("ibm32.mtx")[:2] + (sample("ibm32.mtx")[3], 0),
               ("memplus",) + sample("memplus.mtx")[:2] + (sample("memplus.mtx")[3], 0)]
    M, _, _, csr = synth()
    sources.append(("synth 2^16", M, M, csr, 0))
    name = ms.BLOCKS[0]
    rows, cols, row0, _ = ms.structure(name)
    sources.append(("mixed " + name, rows, cols, ms.csr_of(name), row0))
    fz = sc.block_fuzz(3)
    sources.append(("spmm fuzz 3", fz[0], fz[1], fz[2:5], 0))

    for label, rows, cols, csr, row0 in sources:
        x = dev(np.random.default_rng(1).random(max(cols, 1)))
        plans = list(csr_plans(rows))
        for kind in ("host", "adopted"):
            what = "csr %s, %s arrays" % (label, kind)
            with balanced(what + ": create, every plan, destroy"):
                A = make_csr(kind, rows, cols, csr, row0)
                held = {}
                for plan in plans:
                    set_plan(A, plan)
                    csr_product(A, x)
                    first = snap()
                    for again in (2, 3):                       # the same re-plan: nothing accumulates
                        set_plan(A, plan)
                        require_same(first, snap(), "%s: %s planned the %d. time" % (what, plan[0], again))
                    held[plan[0]] = first
                for plan in reversed(plans):                   # the ring, backwards: a plan holds what it held on the way out
                    set_plan(A, plan)
                    csr_product(A, x)
                    require_same(held[plan[0]], snap(), "%s: %s on the way back" % (what, plan[0]))
                A.gather_spread()
                A.far_share()
                A.close()
        # adopted arrays stay the caller's: readable and unchanged after the handle is gone
        with balanced("csr %s: adopted arrays are still the caller's after destroy" % label):
            rp, ci, v = dev(csr[0]), dev(csr[1] if len(csr[1]) else np.zeros(4, np.int32)), dev(csr[2] if len(csr[2]) else np.zeros(4))
            A = sm.CsrMatrix(rows, cols, rp, ci, v, first_row=row0)
            for plan in plans:
                set_plan(A, plan)
            A.close()
            torch.cuda.synchronize()
            expect((rp.cpu().numpy() == csr[0]).all() and (ci.cpu().numpy()[:len(csr[1])] == csr[1]).all() and
                   (v.cpu().numpy()[:len(csr[2])].view(np.uint64) == np.asarray(csr[2]).view(np.uint64)).all(),
                   "csr %s: an adopted array changed" % label)
        # the SpMM plan (built by the first spmm, kept across re-plans), and A^T destroyed before and after its source
        k = 3
        X = dev(np.random.default_rng(2).random((max(cols, 1), k)))
        Y = torch.empty((max(rows, 1), k), dtype=torch.float64, device="cuda")
        with balanced("csr %s: first spmm, re-plans, destroy" % label):
            A = make_csr("host", rows, cols, csr, row0)
            before = snap()
            A.spmm(X[:cols], Y[:rows])
            torch.cuda.synchronize()
            built = snap()
            A.spmm(X[:cols], Y[:rows])
            torch.cuda.synchronize()
            require_same(built, snap(), "csr %s: the second spmm" % label)
            expect(at(built, DEVICE, BYTES) - at(before, DEVICE, BYTES) == (4 * rows if rows else 0),
                   "csr %s: the SpMM plan holds %d bytes, 4 * rows = %d expected" % (label, at(built, DEVICE, BYTES) - at(before, DEVICE, BYTES), 4 * rows))
            A.set_kernel(sm.CSR_KERNEL_VECTOR, 0)
            A.set_kernel(sm.CSR_KERNEL_AUTO, 0)
            A.close()
        for first_gone in ("source", "transposed"):
            with balanced("csr %s: create_transposed, %s destroyed first" % (label, first_gone)):
                A = make_csr("host", rows, cols, csr, row0)
                T = A.transposed()
                xt = dev(np.random.default_rng(3).random(max(rows, 1)))
                (A if first_gone == "source" else T).close()
                if first_gone == "source":
                    csr_product(T, xt)
                T.close()
                A.close()


# ========================================================================================================== group: tjds life cycle
def make_tjds(kind, t):
    if kind == "host":
        return sm.TjdsMatrix(t)
    d = sm.TjdsArrays()
    d.__dict__.update(t.__dict__)
    d.perm, d.start_pos = dev(t.perm if len(t.perm) else np.zeros(1, np.int32)), dev(t.start_pos)
    d.row_ind, d.val = dev(t.row_ind if len(t.row_ind) else np.zeros(1, np.int32)), dev(t.val if len(t.val) else np.zeros(1))
    return sm.TjdsMatrix(d)


TJDS_MODES = (sm.TJDS_MODE_ROW_GATHER, sm.TJDS_MODE_TWO_PHASE, sm.TJDS_MODE_ATOMIC)


def group_tjds():
    import torch

    import mixed_structures as ms

    sources = []
    for name in ("ibm32.mtx", "memplus.mtx"):
        m, n, coo, _ = sample(name)
        sources.append((name[:-4], m, n, coo))
    M, _, coo, _ = synth()
    sources.append(("synth 2^16", M, M, coo))
    name = ms.WHOLE[2]
    rows, cols, _, coo = ms.structure(name)
    sources.append(("mixed " + name, rows, cols, coo))

    for label, rows, cols, coo in sources:
        t = sm.tjds_from_coo(coo, rows, cols)
        x = dev(np.random.default_rng(1).random(max(cols, 1)))
        xr = dev(np.random.default_rng(2).random(max(rows, 1)))
        for kind in ("host", "adopted"):
            for index in (0, 1, 2):
                what = "tjds %s, %s arrays, tjds_index %d" % (label, kind, index)
                with balanced(what + ": create, modes, tiles, value cache, ref-quirks, destroy"), options({"tjds_index": index}):
                    T = make_tjds(kind, t)
                    held = {}
                    for mode in TJDS_MODES + TJDS_MODES[::-1]:
                        T.set_mode(mode)
                        tjds_product(T, x)
                        held[mode] = snap()
                    for mode in TJDS_MODES:                    # every plan exists now: a change of mode takes and frees nothing
                        T.set_mode(mode)
                        require_same(held[TJDS_MODES[0]], snap(), "%s: set_mode(%d) with every plan built" % (what, mode))
                    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
                    for tile in (256, 1024, 2048, 1024):
                        T.set_tile(tile)
                        tjds_product(T, x)
                        first = snap()
                        T.set_tile(tile)
                        require_same(first, snap(), "%s: set_tile(%d) again" % (what, tile))
                    for min_tiles in (0, 2, 4, 0, 2, 4):
                        if index == 2 and min_tiles:           # 32-bit columns in row order: no tile-ordered stream, no cache
                            expect(status("smvp_tjds_set_value_cache", T._h, min_tiles) == sm.ERR_UNSUPPORTED,
                                   "%s: a value cache on the row-ordered stream was not refused" % what)
                            continue
                        T.set_value_cache(min_tiles)
                        tjds_product(T, x)
                        first = snap()
                        T.set_value_cache(min_tiles)
                        require_same(first, snap(), "%s: set_value_cache(%d) again" % (what, min_tiles))
                    base = snap()
                    for on in (True, False, True, False):
                        T.set_ref_quirks(on)
                        if rows == cols or not on:
                            tjds_product(T, x)
                    require_same(base, snap(), "%s: ref-quirks on and off" % what)
                    T.close()
        with balanced("tjds %s: first spmm, spmv_transposed, spmm_transposed, diagonal, destroy" % label):
            T = make_tjds("host", t)
            k = 3
            X = dev(np.random.default_rng(3).random((max(cols, 1), k)))
            Y = torch.empty((max(rows, 1), k), dtype=torch.float64, device="cuda")
            before = snap()
            T.spmm(X[:cols], Y[:rows])
            torch.cuda.synchronize()
            built = snap()
            T.spmm(X[:cols], Y[:rows])
            torch.cuda.synchronize()
            require_same(built, snap(), "tjds %s: the second spmm" % label)
            expect(at(built, DEVICE, LIVE) - at(before, DEVICE, LIVE) == 4, "tjds %s: the SpMM plan is four arrays" % label)
            quiet = snap()
            yc = torch.empty(max(cols, 1), dtype=torch.float64, device="cuda")
            T.spmv_transposed(xr[:rows], yc[:cols])
            T.spmm_transposed(Y[:rows], X[:cols])
            if rows == cols:
                T.diagonal(yc[:rows])
            torch.cuda.synchronize()
            require_same(quiet, snap(), "tjds %s: the plan-less products take nothing" % label, counters=True)
            T.set_mode(sm.TJDS_MODE_TWO_PHASE)
            T.close()
        with balanced("tjds %s: adopted arrays are still the caller's after destroy" % label):
            d = sm.TjdsArrays()
            d.__dict__.update(t.__dict__)
            d.perm, d.start_pos, d.row_ind, d.val = dev(t.perm), dev(t.start_pos), dev(t.row_ind), dev(t.val)
            T = sm.TjdsMatrix(d)
            for mode in TJDS_MODES:
                T.set_mode(mode)
            T.close()
            torch.cuda.synchronize()
            expect((d.perm.cpu().numpy() == t.perm).all() and (d.row_ind.cpu().numpy() == t.row_ind).all() and
                   (d.val.cpu().numpy().view(np.uint64) == t.val.view(np.uint64)).all(), "tjds %s: an adopted array changed" % label)


# ======================================================================================================== group: the other objects
def group_objects():
    import torch

    import cg_method as cg

    import ilu0_method as im

    Mx = cg.spd(300)
    n = Mx.n
    Fx = im.as_matrix(im.grid(24))                     # columns ascending, a stored diagonal in every row: admits an ILU(0)
    # trsv plans: both triangles, both diagonal kinds, three chain widths
    for width in (256, 512, 1024):
        with balanced("trsv plans at trsv_chain_width %d" % width), options({"trsv_chain_width": width}):
            A = sm.CsrMatrix(n, n, *Mx.csr)
            b = dev(cg.rhs(n))
            xs = torch.empty(n, dtype=torch.float64, device="cuda")
            for uplo in (sm.TRSV_LOWER, sm.TRSV_UPPER):
                for diag in (sm.TRSV_DIAG_STORED, sm.TRSV_DIAG_UNIT):
                    P = A.trsv_plan(uplo, diag)
                    planned = snap()
                    P.solve(b, xs)
                    torch.cuda.synchronize()
                    require_same(planned, snap(), "trsv solve (uplo %d, diag %d, width %d)" % (uplo, diag, width), counters=True)
                    P.close()
            A.close()
    m, nn, coo, csr = sample("memplus.mtx")
    with balanced("trsv plans on memplus"):
        A = sm.CsrMatrix(m, nn, *csr)
        P, Q = A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT)
        Q.close()
        P.close()
        A.close()
    # ILU(0): every order of destruction tests/test_gpu_ilu0.py allows -- plans before the factor, the factor before its source;
    # closing the borrowed matrix destroys nothing
    for order in ("plans, matrix, factor, source", "matrix, plans, factor, source", "second plan first"):
        with balanced("ilu0 create / factor / matrix / plans, destroyed: " + order):
            A = sm.CsrMatrix(Fx.n, Fx.n, *Fx.csr)
            f = A.ilu0()
            made = snap()
            f.factor()
            f.factor()
            torch.cuda.synchronize()
            require_same(made, snap(), "ilu0 factor again")
            L, U = f.plans()
            if order.startswith("matrix"):
                f.matrix.close()
            if order == "second plan first":
                U.close()
                L.close()
            else:
                L.close()
                U.close()
            f.matrix.close()
            f.close()
            A.close()
    with balanced("two ilu0 objects of one source, the first destroyed first"):
        A = sm.CsrMatrix(Fx.n, Fx.n, *Fx.csr)
        f1, f2 = A.ilu0(), A.ilu0()
        f1.close()
        f2.factor()
        f2.close()
        A.close()
    # the device conversions: scratch only, the outputs are the caller's
    for label, (rows, cols, coo, _) in (("ibm32", sample("ibm32.mtx")), ("memplus", sample("memplus.mtx")), ("synth 2^16", synth())):
        d_coo = dev(np.frombuffer(np.ascontiguousarray(coo, dtype=sm.COO_DTYPE).tobytes(), dtype=np.uint8))
        for fn in (sm.csr_from_coo_device, sm.tjds_from_coo_device):
            with balanced("%s on %s" % (fn.__name__, label)):
                fn(d_coo, rows, cols, len(coo))
        # an entry outside the matrix: SMVP_ERR_INVALID with the scratch released
        bad = np.array(coo, dtype=sm.COO_DTYPE)
        bad["col"][len(bad) // 2] = cols
        d_bad = dev(np.frombuffer(bad.tobytes(), dtype=np.uint8))
        for fn in (sm.csr_from_coo_device, sm.tjds_from_coo_device):
            with balanced("%s on %s with an entry outside the matrix" % (fn.__name__, label)):
                try:
                    fn(d_bad, rows, cols, len(bad))
                    raise Failed("%s accepted an entry outside the matrix" % fn.__name__)
                except sm.SmvpError as e:
                    expect(e.code == sm.ERR_INVALID, "%s: status %d for an entry outside the matrix, SMVP_ERR_INVALID expected" % (fn.__name__, e.code))
    # the timed entry points: per-call scratch, both timing modes, beyond the timing rings
    m, nn, coo, _ = sample("ibm32.mtx")
    for fn in (sm.csr_compute, sm.tjds_compute):
        for timing in (sm.TIMING_EVENTS, sm.TIMING_DEVICE, sm.TIMING_DEVICE_GRAPH, sm.TIMING_AUTO):
            for kw in ({"iters": 2500}, {"iters": 40, "iterate": True, "normalize": True}, {"iters": 3, "device_convert": True}):
                with balanced("%s on ibm32, timing %d, %s" % (fn.__name__, timing, kw)):
                    try:
                        fn(coo, m, nn, timing=timing, **kw)
                        refused = False
                    except sm.SmvpError as e:          # device-side timing is documented as unavailable with iterate
                        refused = e.code == sm.ERR_UNSUPPORTED
                        expect(refused, "%s: status %d" % (fn.__name__, e.code))
                    expect(refused == (kw.get("iterate", False) and timing in (sm.TIMING_DEVICE, sm.TIMING_DEVICE_GRAPH)),
                           "%s, timing %d, %s: %s" % (fn.__name__, timing, kw, "refused" if refused else "not refused"))
    m, nn, coo, _ = sample("memplus.mtx")
    for fn in (sm.csr_compute, sm.tjds_compute):
        for timing in (sm.TIMING_EVENTS, sm.TIMING_DEVICE):
            with balanced("%s on memplus, timing %d, device_convert" % (fn.__name__, timing)):
                fn(coo, m, nn, iters=20, timing=timing, device_convert=True)
    # the sharded layer on one GPU with virtual ranks (the RCCL communicators are not counted: see the head of this file)
    rp, ci, v = sample("memplus.mtx")[3]
    for fmt in ("csr", "tjds"):
        for exchange in (sm.EXCHANGE_COPIES, sm.EXCHANGE_DIRECT):
            with balanced("sharded %s, 4 virtual ranks, exchange %s" % (fmt, sm.EXCHANGE_NAMES[exchange])):
                S = sm.ShardedMatrix(fmt, 4, m, nn, coo=coo, csr=(rp, ci, v), devices=[0, 0, 0, 0], chunks=2, exchange=exchange)
                S.set_x(np.random.default_rng(4).random(nn))
                made = snap()
                for gather in (sm.GATHER_OVERLAPPED, sm.GATHER_AFTER, sm.GATHER_NONE):
                    S.spmv(gather)
                    S.synchronize()
                S.spmv(sm.GATHER_OVERLAPPED)
                S.feed_back(normalize=True)
                S.spmv(sm.GATHER_OVERLAPPED)
                S.synchronize()
                S.get_y()
                require_same(made, snap(), "sharded %s: products and feed_back take nothing" % fmt)
                if fmt == "csr":
                    S.set_csr_kernel(sm.CSR_KERNEL_VECTOR, 0)
                    S.set_csr_kernel(sm.CSR_KERNEL_STREAM, 0)
                    S.spmv(sm.GATHER_OVERLAPPED)
                    S.synchronize()
                S.close()


# ============================================================================================== group: the per-call work spaces
def solver_calls(H, n, b, x0, m, plans, max_steps, tol, stream=None, x=None, every=3):
    """Every solver entry point of handle H as (name, thunk -> status, thunk -> the result block's integers, reason last); the
    thunks keep their operands alive.  plans: (first, second) TrsvPlans or None."""
    import torch

    csr = isinstance(H, sm.CsrMatrix)
    p = "smvp_csr_" if csr else "smvp_tjds_"
    if x is None:
        x = torch.zeros(max(n, 1), dtype=torch.float64, device="cuda")
    rr, rz, sig = np.zeros(max_steps + 1), np.zeros(max_steps + 1), np.zeros(max_steps + 1)
    po, pr = sm.power_opts(max_steps, tol, every), sm.PowerResult()
    co, cr, qr = sm.cg_opts(max_steps, tol, every), sm.CgResult(), sm.PcgResult()
    bo, br = sm.bicgstab_opts(max_steps, tol, every), sm.BicgstabResult()
    P, S = sm._dev_ptr, sm._stream_ptr(stream)
    first, second = (plans[0]._t, plans[1]._t) if plans else (None, None)
    power = lambda: (pr.steps, pr.index, pr.reason)              # noqa: E731
    cgr = lambda: (cr.steps, cr.updates, cr.reason)              # noqa: E731
    pcgr = lambda: (qr.steps, qr.updates, qr.reason)             # noqa: E731
    bir = lambda: (br.steps, br.full, br.half, br.reason)        # noqa: E731
    yield "power", lambda: status(p + "power_method", H._h, C.byref(po), P(x0), P(x), C.byref(pr), sm._p(rr), sm._p(sig), S), power
    yield "cg", lambda: status(p + "cg", H._h, C.byref(co), P(b), P(x0), P(x), C.byref(cr), sm._p(rr), sm._p(sig), S), cgr
    if m is not None:
        yield "pcg", lambda: status(p + "pcg", H._h, C.byref(co), P(b), P(x0), P(x), P(m), C.byref(qr), sm._p(rr), sm._p(rz), sm._p(sig), S), pcgr
    yield "bicgstab", lambda: status(p + "bicgstab", H._h, C.byref(bo), P(b), P(x0), P(x), C.byref(br), sm._p(rr), sm._p(sig), S), bir
    if m is not None:
        yield "pbicgstab jacobi", lambda: status(p + "pbicgstab", H._h, C.byref(bo), P(b), P(x0), P(x), None, P(m), None, C.byref(br),
                                                 sm._p(rr), sm._p(sig), S), bir
    if plans:
        yield "pcg_tri", lambda: status(p + "pcg_tri", H._h, C.byref(co), P(b), P(x0), P(x), first, P(m), second, C.byref(qr),
                                        sm._p(rr), sm._p(rz), sm._p(sig), S), pcgr
        yield "pbicgstab plans", lambda: status(p + "pbicgstab", H._h, C.byref(bo), P(b), P(x0), P(x), first, P(m), second, C.byref(br),
                                                sm._p(rr), sm._p(sig), S), bir


def solver_handles(M):
    """(CSR handle, TJDS handle, the CSR handle's LOWER and UPPER plans) of a square matrix."""
    A = sm.CsrMatrix(M.n, M.n, *M.csr)
    plans = (A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER)) if M.n > 0 else None
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    return A, T, plans


TAKEN = {}     # solver -> the stop reasons its runs ended with, over the whole group


def way_out(label, M, only, b, x0, m, plans, max_steps, tol, want, every=3):
    """The solvers named in `only` on the CSR handle and on the TJDS handle (both reproducible modes) of M: status OK, the result
    block's integers are `want` -- a tuple (None = any value), or the reason alone as an int, or None where the restatement's tests
    fix no reason -- and the call's work space is gone when it returns."""
    A = sm.CsrMatrix(M.n, M.n, *M.csr)
    T = sm.TjdsMatrix(sm.tjds_from_coo(M.coo, M.n, M.n))
    db, d0, dm = (None if v is None else dev(v) for v in (b, x0, m))
    for H, name, mode in ((A, "csr", None), (T, "tjds", sm.TJDS_MODE_ROW_GATHER), (T, "tjds", sm.TJDS_MODE_TWO_PHASE)):
        if mode is not None:
            H.set_mode(mode)
        for fn, call, result in solver_calls(H, M.n, db, d0, dm, plans, max_steps, tol, every=every):
            if fn not in only:
                continue
            what = "%s %s%s, %s" % (name, fn, "" if mode is None else " mode %d" % mode, label)
            with balanced(what):
                rc = call()
                expect(rc == sm.OK, "%s: status %d (%s)" % (what, rc, last_error()))
            got = result()
            full = want if isinstance(want, tuple) else (None,) * (len(got) - 1) + (want,) if want is not None else (None,) * len(got)
            expect(len(full) == len(got) and all(w is None or w == g for w, g in zip(full, got)),
                   "%s: the run ended with %r, %r expected: this way out was not taken" % (what, got, want))
            TAKEN.setdefault(fn, set()).add(got[-1])
    T.close()
    A.close()


def group_solvers():
    """Every way out the restatements produce: the stop cases of tests/test_gpu_cg.py, test_gpu_pcg.py and test_gpu_bicgstab.py
    with the result blocks those tests derive from cg_method / pcg_method / bicgstab_method, the matrices of all three modules,
    and the power method's special cases.  pcg_tri and pbicgstab have no table of their own: with the plans of an identity matrix
    (a solve that divides by 1.0 is exact) and no m their run is cg's / bicgstab's, so they must end with that table's reason."""
    import torch

    import bicgstab_method as bi
    import cg_method as cg
    import pcg_method as pcg
    import power_method as pm
    import test_gpu_bicgstab as k13
    import test_gpu_cg as k12
    import test_gpu_pcg as k14
    import test_gpu_power_method as k11

    def identity_plans(n):
        eye = sm.CsrMatrix(n, n, *cg.identity(n).csr)
        return eye, (eye.trsv_plan(sm.TRSV_LOWER), eye.trsv_plan(sm.TRSV_UPPER))

    def close_plans(eye, plans):
        for Q in plans:
            Q.close()
        eye.close()

    for name, M, b, tol, want in k12.stop_cases():
        way_out("cg stop case '%s'" % name, M, ("cg",), b, None, None, None, 10, tol, want)
        eye, plans = identity_plans(M.n)
        way_out("cg stop case '%s' behind identity plans" % name, M, ("pcg_tri",), b, None, None, plans, 10, tol, want[2])
        close_plans(eye, plans)
    for name, M, b, m, tol, want in k14.stop_cases():
        way_out("pcg stop case '%s'" % name, M, ("pcg",), b, None, m, None, 10, tol, want)
    for name, M, b, tol, want, _ in k13.stop_cases():
        way_out("bicgstab stop case '%s'" % name, M, ("bicgstab",), b, None, None, None, 10, tol, want)
        way_out("bicgstab stop case '%s' with m = ones" % name, M, ("pbicgstab jacobi",), b, None, np.ones(M.n), None, 10, tol, want[3])
        eye, plans = identity_plans(M.n)
        way_out("bicgstab stop case '%s' behind identity plans" % name, M, ("pbicgstab plans",), b, None, None, plans, 10, tol, want[3])
        close_plans(eye, plans)
    # the larger systems of the three modules.  Strictly dominant rows (off-diagonal sums of at most half the diagonal) make CG,
    # BiCGSTAB and their Jacobi and Gauss-Seidel forms contract by a constant factor a step: 80 steps are far more than 1e-10 needs.
    # tridiagonal(n) is not dominant: it is run for 4 steps at tol 0 as tests/test_gpu_pcg.py runs it, and ends at MAX_STEPS.
    CONV = cg.CONVERGED
    for label, M in (("spd(1003)", cg.spd(1003)), ("spd_long", cg.spd_long()), ("spd_shuffled", cg.spd_shuffled()),
                     ("scaled(spd(1003), 2)", pcg.scaled(cg.spd(1003), 2))):
        jac = pcg.diagonal(M)
        for x0 in (None, cg.rhs(M.n, 7)):
            tag = "%s%s" % (label, "" if x0 is None else " from an x0")
            # (scaled: S A S with S spanning two decades is dominant no longer; Jacobi undoes S, the plain forms have no fixed end)
            plain = None if label.startswith("scaled") else CONV
            way_out(tag, M, ("cg", "bicgstab"), cg.rhs(M.n), x0, jac, None, 80, 1e-10, plain)
            way_out(tag, M, ("pcg",), cg.rhs(M.n), x0, jac, None, 80, 1e-10, CONV)
            way_out(tag, M, ("pbicgstab jacobi",), cg.rhs(M.n), x0, 1.0 / jac, None, 80, 1e-10, CONV)
    for label, M in (("nonsym(1003)", bi.nonsym(1003)), ("nonsym_long", bi.nonsym_long()), ("nonsym_shuffled", bi.nonsym_shuffled()),
                     ("banded(2049)", bi.banded(2049))):
        jac = 1.0 / pcg.diagonal(M)
        A = sm.CsrMatrix(M.n, M.n, *M.csr)
        sgs = (A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER))
        way_out(label, M, ("bicgstab", "pbicgstab jacobi"), bi.rhs(M.n), None, jac, None, 80, 1e-10, bi.CONVERGED)
        way_out(label + ", symmetric Gauss-Seidel", M, ("pbicgstab plans",), bi.rhs(M.n), bi.rhs(M.n, 7), pcg.diagonal(M), sgs, 80, 1e-10, bi.CONVERGED)
        close_plans(A, sgs)
    M = cg.spd(1003)
    A = sm.CsrMatrix(M.n, M.n, *M.csr)
    sgs = (A.trsv_plan(sm.TRSV_LOWER), A.trsv_plan(sm.TRSV_UPPER))
    way_out("spd(1003), symmetric Gauss-Seidel", M, ("pcg_tri",), cg.rhs(M.n), None, pcg.diagonal(M), sgs, 80, 1e-10, CONV)
    way_out("spd(1003), symmetric Gauss-Seidel, 2 steps", M, ("pcg_tri", "pbicgstab plans"), cg.rhs(M.n), None, pcg.diagonal(M), sgs, 2, 1e-10, cg.MAX_STEPS)
    close_plans(A, sgs)
    M = pcg.tridiagonal(cg.TRIP + 1)
    way_out("tridiagonal(%d), 4 steps at tol 0" % M.n, M, ("pcg",), cg.rhs(M.n), None, pcg.diagonal(M), None, 4, 0.0, (4, 4, cg.MAX_STEPS))
    # the power method: tests/test_gpu_power_method.py's special cases (6 steps, tol 0, every step looked at: a vanished iterate
    # nobody looks at turns non-finite a step later) and its plain runs
    for name, M, x0, want in k11.special_cases():
        if want is not None:
            way_out("power special case '%s'" % name, M, ("power",), None, x0, None, None, 6, 0.0, (want[0], want[2], want[1]), every=1)
        else:
            way_out("power special case '%s'" % name, M, ("power",), None, x0, None, None, 6, 0.0, None, every=1)
    S = k11.matrix("short")
    way_out("power, 5 steps at tol 0", S, ("power",), None, None, None, None, 5, 0.0, (5, None, pm.MAX_STEPS))
    way_out("power on the identity: the first residual is 0", cg.identity(300), ("power",), None, None, None, None, 5, 1e-10, (1, None, pm.CONVERGED), every=1)
    # every exit has been taken by every solver that has it
    every = {cg.CONVERGED, cg.MAX_STEPS, cg.BREAKDOWN, cg.NONFINITE}
    for fn in ("cg", "pcg", "pcg_tri", "bicgstab", "pbicgstab jacobi", "pbicgstab plans"):
        expect(TAKEN.get(fn) == every, "%s ended with the reasons %r only, %r expected" % (fn, TAKEN.get(fn), every))
    expect(TAKEN.get("power") == {pm.CONVERGED, pm.MAX_STEPS, pm.ZERO, pm.NONFINITE}, "power ended with the reasons %r only" % TAKEN.get("power"))
    DONE.append("every solver took every way out")
    inf = cg.rhs(300)
    inf[17] = np.inf
    A, T, plans = solver_handles(cg.spd(300))
    # ---- refusals.  "before any HIP call" / "before anything is enqueued": not one counted call is made
    db, dm = dev(cg.rhs(300)), dev(np.ones(300))
    x = torch.zeros(300, dtype=torch.float64, device="cuda")
    P = sm._dev_ptr
    for H, name in ((A, "csr"), (T, "tjds")):
        p = "smvp_%s_" % name
        co, cr, qr = sm.cg_opts(10, 1e-10, 3), sm.CgResult(), sm.PcgResult()
        bo, br = sm.bicgstab_opts(10, 1e-10, 3), sm.BicgstabResult()
        po, pr = sm.power_opts(10, 0.0), sm.PowerResult()
        bad_c, bad_b, bad_p = sm.cg_opts(0, 1e-10, 3), sm.bicgstab_opts(10, -1.0, 3), sm.power_opts(10, 0.0)
        bad_p.struct_size = 4
        refusals = [
            ("power, null handle", lambda: status(p + "power_method", None, C.byref(po), None, P(x), C.byref(pr), None, None, None)),
            ("power, null result", lambda: status(p + "power_method", H._h, C.byref(po), None, P(x), None, None, None, None)),
            ("power, wrong struct_size", lambda: status(p + "power_method", H._h, C.byref(bad_p), None, P(x), C.byref(pr), None, None, None)),
            ("power, null d_x", lambda: status(p + "power_method", H._h, C.byref(po), None, None, C.byref(pr), None, None, None)),
            ("cg, null handle", lambda: status(p + "cg", None, C.byref(co), P(db), None, P(x), C.byref(cr), None, None, None)),
            ("cg, null d_b", lambda: status(p + "cg", H._h, C.byref(co), None, None, P(x), C.byref(cr), None, None, None)),
            ("cg, max_steps 0", lambda: status(p + "cg", H._h, C.byref(bad_c), P(db), None, P(x), C.byref(cr), None, None, None)),
            ("cg, d_b is d_x", lambda: status(p + "cg", H._h, C.byref(co), P(x), None, P(x), C.byref(cr), None, None, None)),
            ("pcg, null d_m", lambda: status(p + "pcg", H._h, C.byref(co), P(db), None, P(x), None, C.byref(qr), None, None, None, None)),
            ("pcg, d_m is d_x", lambda: status(p + "pcg", H._h, C.byref(co), P(db), None, P(x), P(x), C.byref(qr), None, None, None, None)),
            ("pcg_tri, null plans", lambda: status(p + "pcg_tri", H._h, C.byref(co), P(db), None, P(x), None, P(dm), None, C.byref(qr),
                                                    None, None, None, None)),
            ("bicgstab, null opts", lambda: status(p + "bicgstab", H._h, None, P(db), None, P(x), C.byref(br), None, None, None)),
            ("bicgstab, negative tol", lambda: status(p + "bicgstab", H._h, C.byref(bad_b), P(db), None, P(x), C.byref(br), None, None, None)),
            ("pbicgstab, no preconditioner", lambda: status(p + "pbicgstab", H._h, C.byref(bo), P(db), None, P(x), None, None, None,
                                                             C.byref(br), None, None, None)),
        ]
        for label, call in refusals:
            with unmoved("%s %s is refused without a counted call" % (name, label)):
                rc = call()
                expect(rc == sm.ERR_INVALID, "%s %s: status %d, SMVP_ERR_INVALID expected" % (name, label, rc))
    # a TJDS handle in ATOMIC mode or with ref-quirks on: SMVP_ERR_UNSUPPORTED, nothing taken
    T.set_mode(sm.TJDS_MODE_ATOMIC)
    for fn, call, _ in solver_calls(T, 300, db, None, dm, plans, 10, 1e-10):
        with unmoved("tjds %s in ATOMIC mode is refused without a counted call" % fn):
            expect(call() == sm.ERR_UNSUPPORTED, "tjds %s in ATOMIC mode was not refused" % fn)
    T.set_mode(sm.TJDS_MODE_ROW_GATHER)
    # ... and with ref-quirks on
    T.set_ref_quirks(True)
    for fn, call, _ in solver_calls(T, 300, db, None, dm, plans, 10, 1e-10):
        with unmoved("tjds %s with ref-quirks on is refused without a counted call" % fn):
            expect(call() == sm.ERR_UNSUPPORTED, "tjds %s with ref-quirks on was not refused" % fn)
    T.set_ref_quirks(False)
    # a CSR handle that is not plain CSR (the one a TJDS handle in ROW_GATHER mode keeps inside): SMVP_ERR_UNSUPPORTED
    from test_gpu_transposed import inner_csr_handle

    inner, out = inner_csr_handle(T, 300, 300, T.nnz), C.c_void_p()
    Y2 = torch.zeros((300, 2), dtype=torch.float64, device="cuda")
    X2 = torch.zeros((300, 2), dtype=torch.float64, device="cuda")
    cso, csr_, pso, psr = sm.cg_opts(10, 1e-10, 3), sm.CgResult(), sm.power_opts(10, 0.0), sm.PowerResult()
    bso, bsr, qsr = sm.bicgstab_opts(10, 1e-10, 3), sm.BicgstabResult(), sm.PcgResult()
    for label, call in (
            ("power", lambda: status("smvp_csr_power_method", inner, C.byref(pso), None, P(x), C.byref(psr), None, None, None)),
            ("cg", lambda: status("smvp_csr_cg", inner, C.byref(cso), P(db), None, P(x), C.byref(csr_), None, None, None)),
            ("pcg", lambda: status("smvp_csr_pcg", inner, C.byref(cso), P(db), None, P(x), P(dm), C.byref(qsr), None, None, None, None)),
            ("pcg_tri", lambda: status("smvp_csr_pcg_tri", inner, C.byref(cso), P(db), None, P(x), plans[0]._t, P(dm), plans[1]._t, C.byref(qsr),
                                       None, None, None, None)),
            ("bicgstab", lambda: status("smvp_csr_bicgstab", inner, C.byref(bso), P(db), None, P(x), C.byref(bsr), None, None, None)),
            ("pbicgstab", lambda: status("smvp_csr_pbicgstab", inner, C.byref(bso), P(db), None, P(x), None, P(dm), None, C.byref(bsr), None, None, None)),
            ("spmm", lambda: status("smvp_csr_spmm", inner, 2, P(X2), 2, P(Y2), 2, None)),
            ("diagonal", lambda: status("smvp_csr_diagonal", inner, P(x), None)),
            ("create_transposed", lambda: status("smvp_csr_create_transposed", C.byref(out), inner, None))):
        with unmoved("csr %s on a handle that is not plain CSR is refused without a counted call" % label):
            expect(call() == sm.ERR_UNSUPPORTED and not out.value, "csr %s on a handle that is not plain CSR: not SMVP_ERR_UNSUPPORTED" % label)
    # the other documented SMVP_ERR_INVALID refusals of every solver, each without a counted call: a matrix that is not square,
    # check_every < 1, a tol that is NaN or infinite, d_x0 and d_x that overlap without being the same vector, plans of another size
    W = cg.spd(5)
    wide_csr = sm.CsrMatrix(4, 5, W.row_ptr[:5].copy(), W.col_ind[:W.row_ptr[4]].copy(), W.val[:W.row_ptr[4]].copy())
    wc = sm.coo_from_csr(4, W.row_ptr[:5].copy(), W.col_ind[:W.row_ptr[4]].copy(), W.val[:W.row_ptr[4]].copy())
    wide_tjds = sm.TjdsMatrix(sm.tjds_from_coo(wc, 4, 5))
    eye2 = sm.CsrMatrix(2, 2, *cg.identity(2).csr)
    small = (eye2.trsv_plan(sm.TRSV_LOWER), eye2.trsv_plan(sm.TRSV_UPPER))
    buf = torch.zeros(301, dtype=torch.float64, device="cuda")
    d5 = torch.zeros(5, dtype=torch.float64, device="cuda")
    for H, W_, name in ((A, wide_csr, "csr"), (T, wide_tjds, "tjds")):
        cases = [("a matrix that is not square", solver_calls(W_, 4, d5, None, d5, None, 10, 1e-10, x=d5)),
                 ("check_every 0", solver_calls(H, 300, db, None, dm, plans, 10, 1e-10, every=0)),
                 ("tol NaN", solver_calls(H, 300, db, None, dm, plans, 10, float("nan"))),
                 ("tol infinite", solver_calls(H, 300, db, None, dm, plans, 10, float("inf"))),
                 ("d_x0 and d_x overlapping in part", solver_calls(H, 300, db, buf[:300], dm, plans, 10, 1e-10, x=buf[1:])),
                 ("plans of another size", (c for c in solver_calls(H, 300, db, None, dm, small, 10, 1e-10) if c[0] in ("pcg_tri", "pbicgstab plans")))]
        for label, calls in cases:
            for fn, call, _ in calls:
                with unmoved("%s %s, %s, is refused without a counted call" % (name, fn, label)):
                    rc = call()
                    expect(rc == sm.ERR_INVALID, "%s %s, %s: status %d, SMVP_ERR_INVALID expected" % (name, fn, label, rc))
    # a capturing stream: every call that allocates or synchronises refuses it with SMVP_ERR_INVALID before anything is enqueued or
    # taken, d_x is left alone, and the capture stays valid
    fresh_csr = sm.CsrMatrix(300, 300, *cg.spd(300).csr)                       # (no SpMM plan yet)
    fresh_tjds = sm.TjdsMatrix(sm.tjds_from_coo(cg.spd(300).coo, 300, 300))
    side = torch.cuda.Stream()
    dZ = torch.zeros(16, dtype=torch.float64, device="cuda")
    dx = torch.full((300,), -12345.678, dtype=torch.float64, device="cuda")
    S_ = sm._stream_ptr(side)
    captured = [("%s %s" % (name, fn), call) for H, name in ((A, "csr"), (T, "tjds"))
                for fn, call, _ in solver_calls(H, 300, db, None, dm, plans, 10, 1e-10, stream=side, x=dx)]
    captured += [
        ("the first smvp_csr_spmm", lambda: status("smvp_csr_spmm", fresh_csr._h, 2, P(X2), 2, P(Y2), 2, S_)),
        ("the first smvp_tjds_spmm", lambda: status("smvp_tjds_spmm", fresh_tjds._h, 2, P(X2), 2, P(Y2), 2, S_)),
        ("smvp_csr_create_transposed", lambda: status("smvp_csr_create_transposed", C.byref(out), A._h, S_)),
        ("smvp_csr_trsv_create", lambda: status("smvp_csr_trsv_create", C.byref(out), A._h, sm.TRSV_LOWER, sm.TRSV_DIAG_STORED, S_)),
        ("smvp_csr_ilu0_create", lambda: status("smvp_csr_ilu0_create", C.byref(out), A._h, S_))]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            dZ.add_(1.0)                               # (keeps the captured graph from being empty)
            for label, call in captured:
                with unmoved("%s on a capturing stream is refused without a counted call" % label):
                    rc = call()
                    expect(rc == sm.ERR_INVALID and "captur" in last_error() and not out.value,
                           "%s on a capturing stream: status %d (%s)" % (label, rc, last_error()))
            dZ.add_(1.0)
    g.replay()
    torch.cuda.synchronize()
    expect(dZ.cpu().numpy().tolist() == [2.0] * 16 and (dx.cpu().numpy() == -12345.678).all() and (Y2.cpu().numpy() == 0).all(),
           "the capture did not stay valid, or a refused call wrote its output")
    DONE.append("the capture stayed valid")
    del g
    with balanced("the same stream outside a capture is fine"):
        for label, call in captured[:-5]:                     # (the solvers: they leave nothing behind)
            expect(call() == sm.OK, "%s on the same stream outside the capture: %s" % (label, last_error()))
    for Q in small:
        Q.close()
    for Hh in (eye2, wide_csr, wide_tjds, fresh_csr, fresh_tjds):
        Hh.close()
    # the products' own refusals: before anything is enqueued
    Y = torch.zeros((300, 2), dtype=torch.float64, device="cuda")
    A.spmm(Y, torch.zeros((300, 2), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    for label, call in (
            ("csr spmm, null handle", lambda: status("smvp_csr_spmm", None, 2, P(Y), 2, P(Y), 2, None)),
            ("csr spmm, k 0", lambda: status("smvp_csr_spmm", A._h, 0, P(Y), 2, P(Y), 2, None)),
            ("csr spmm, overlapping operands", lambda: status("smvp_csr_spmm", A._h, 2, P(Y), 2, P(Y), 2, None)),
            ("tjds spmm (no plan yet), ldx < k", lambda: status("smvp_tjds_spmm", T._h, 2, P(Y), 1, P(x), 2, None)),
            ("tjds spmm_transposed, overlapping operands", lambda: status("smvp_tjds_spmm_transposed", T._h, 2, P(Y), 2, P(Y), 2, None)),
            ("tjds spmv_transposed, null d_y", lambda: status("smvp_tjds_spmv_transposed", T._h, P(x), None, None)),
            ("create_transposed, null source", lambda: status("smvp_csr_create_transposed", C.byref(C.c_void_p()), None, None))):
        with unmoved(label + " is refused without a counted call"):
            expect(call() == sm.ERR_INVALID, label + ": not refused with SMVP_ERR_INVALID")
    for Q in plans:
        Q.close()
    T.close()
    A.close()
    # ---- the malformed arrays smvp_csr_create / smvp_tjds_create refuse on the host: checked before anything is uploaded
    m, n, coo, (rp, ci, v) = sample("ibm32.mtx")
    out = C.c_void_p()
    bad_rp, bad_ci = rp.copy(), ci.copy()
    bad_rp[3], bad_rp[4] = rp[4], rp[3] - 1
    bad_ci[5] = n
    t = sm.tjds_from_coo(coo, m, n)
    bad_sp, bad_ri, bad_perm = t.start_pos.copy(), t.row_ind.copy(), t.perm.copy()
    bad_sp[1] = 0
    bad_ri[2] = m
    bad_perm[0] = -1
    p_ = sm._p
    for label, call in (
            ("csr create, negative rows", lambda: status("smvp_csr_create", C.byref(out), 0, -1, n, len(ci), p_(rp), p_(ci), p_(v), sm.MEM_HOST, None)),
            ("csr create, bad mem_kind", lambda: status("smvp_csr_create", C.byref(out), 0, m, n, len(ci), p_(rp), p_(ci), p_(v), 7, None)),
            ("csr create, row_ptr not ascending", lambda: status("smvp_csr_create", C.byref(out), 0, m, n, len(ci), p_(bad_rp), p_(ci), p_(v), sm.MEM_HOST, None)),
            ("csr create, a column outside", lambda: status("smvp_csr_create", C.byref(out), 0, m, n, len(ci), p_(rp), p_(bad_ci), p_(v), sm.MEM_HOST, None)),
            ("csr create_block, negative first_row", lambda: status("smvp_csr_create_block", C.byref(out), 0, m, n, len(ci), p_(rp), p_(ci), p_(v), sm.MEM_HOST, None, -1)),
            ("tjds create, bad start_pos", lambda: status("smvp_tjds_create", C.byref(out), 0, m, n, t.nnz, t.num_diag, p_(t.perm), p_(bad_sp), p_(t.row_ind), p_(t.val), sm.MEM_HOST)),
            ("tjds create, a row outside", lambda: status("smvp_tjds_create", C.byref(out), 0, m, n, t.nnz, t.num_diag, p_(t.perm), p_(t.start_pos), p_(bad_ri), p_(t.val), sm.MEM_HOST)),
            ("tjds create, a bad perm", lambda: status("smvp_tjds_create", C.byref(out), 0, m, n, t.nnz, t.num_diag, p_(bad_perm), p_(t.start_pos), p_(t.row_ind), p_(t.val), sm.MEM_HOST))):
        with unmoved(label + " is refused without a counted call"):
            expect(call() == sm.ERR_INVALID and not out.value, label + ": not refused with SMVP_ERR_INVALID and *out left alone")
    # adopted arrays are range-checked on the device: one int of scratch comes and goes, nothing else; a misaligned array and a
    # bad row_ptr are refused before that
    d_rp, d_ci, d_v, d_bad = dev(rp), dev(ci), dev(v), dev(bad_ci)
    with unmoved("csr create, adopted arrays off a 16-byte boundary, is refused without a counted call"):
        rc = status("smvp_csr_create", C.byref(out), 0, m, n, len(ci), P(d_rp), C.c_void_p(d_ci.data_ptr() + 4), P(d_v), sm.MEM_DEVICE, p_(rp))
        expect(rc == sm.ERR_INVALID and not out.value, "a misaligned adopted col_ind was not refused")
    before = snap()
    rc = status("smvp_csr_create", C.byref(out), 0, m, n, len(ci), P(d_rp), P(d_bad), P(d_v), sm.MEM_DEVICE, p_(rp))
    after = snap()
    expect(rc == sm.ERR_INVALID and not out.value, "an adopted col_ind with a column outside was not refused")
    require_same(before, after, "csr create, adopted col_ind with a column outside")
    expect(at(after, DEVICE, OBTAINS) - at(before, DEVICE, OBTAINS) == 1 and at(after, DEVICE, RELEASES) - at(before, DEVICE, RELEASES) == 1,
           "csr create, adopted col_ind with a column outside: the range check's one int is all the header's order of checks implies; "
           + difference(before, after, counters=True))
    DONE.append("csr create, adopted col_ind with a column outside: one int of scratch")


# ================================================================================================ the allocation refusal sweep
# For every builder -- a call that allocates -- the number N of obtaining calls it makes unhindered is counted on a throw-away
# object; then, for each i in 1 .. N on a fresh object, the i-th such call is refused once (the wrapper returns
# hipErrorOutOfMemory without reaching the runtime: a host-side return code, nothing reaches the device) and the builder has to
# fail cleanly.  The same with the stream / event / pinned-memory switches where the builder creates those.
CODE_NAMES = {sm.ERR_ALLOC: "SMVP_ERR_ALLOC", sm.ERR_HIP: "SMVP_ERR_HIP"}
ANY_CODE = (sm.ERR_ALLOC, sm.ERR_HIP)


def count_obtains(kind, thunk):
    before = snap()
    r = thunk()
    return at(snap(), kind, OBTAINS) - at(before, kind, OBTAINS), r


def refused_once(kind, i, thunk, what):
    """thunk() with the i-th obtaining call of `kind` refused; the switch must have fired (exactly once: it disarms itself)."""
    before = snap()
    arm(kind, i)
    try:
        r = thunk()
    finally:
        arm(kind, -1)
    expect(snap()[REFUSED] == before[REFUSED] + 1, "%s: the switch for %s call %d did not fire" % (what, KINDS[kind], i))
    return r


def report_sweep(what, kind, n, seen):
    codes = sorted(set(seen.values()))
    print("swept %-72s %-18s N = %3d  %s" % (what, KINDS[kind], n, ", ".join(
        "%s at i = %s" % (CODE_NAMES[c], ",".join(str(i) for i in seen if seen[i] == c)) for c in codes)))
    DONE.append("sweep of %s, %s" % (what, KINDS[kind]))


def sweep_create(what, create, destroy, kinds=(DEVICE,), codes=ANY_CODE):
    """create() -> (status, object or None).  After a refusal: a documented status, no object, and the snapshot back at its start
    at once."""
    import torch

    for kind in kinds:
        base = snap()
        n, (rc, obj) = count_obtains(kind, create)
        expect(rc == sm.OK and obj, "%s: the unhindered call failed with status %d (%s)" % (what, rc, last_error()))
        destroy(obj)
        torch.cuda.synchronize()
        require_same(base, snap(), "%s: created and destroyed" % what)
        seen = {}
        for i in range(1, n + 1):
            where = "%s with %s call %d of %d refused" % (what, KINDS[kind], i, n)
            rc, obj = refused_once(kind, i, create, where)
            expect(rc in codes, "%s: status %d (%s); one of %s expected" % (where, rc, last_error(), [CODE_NAMES[c] for c in codes]))
            expect(not obj, "%s: *out is not NULL / not left alone" % where)
            torch.cuda.synchronize()
            require_same(base, snap(), where + " (status %s)" % CODE_NAMES[rc])
            seen[i] = rc
        report_sweep(what, kind, n, seen)


def sweep_handle(what, make, call, check, destroy, kinds=(DEVICE,), codes=ANY_CODE, same=same_bits):
    """make() -> a fresh object; call(obj) -> status, the builder on it; check(obj) -> bits of a product on it (or None).  After a
    refusal: a documented status; the object still works -- the same call un-failed succeeds and the product is the one of an object
    that never saw a failure --; and after destroy the snapshot is back at its start (buffers kept from the failed build may
    live until then)."""
    import torch

    for kind in kinds:
        base = snap()
        obj = make()
        n, rc = count_obtains(kind, lambda: call(obj))
        expect(rc == sm.OK, "%s: the unhindered call failed with status %d (%s)" % (what, rc, last_error()))
        want = check(obj)
        destroy(obj)
        torch.cuda.synchronize()
        require_same(base, snap(), "%s: made, called and destroyed" % what)
        seen = {}
        for i in range(1, n + 1):
            where = "%s with %s call %d of %d refused" % (what, KINDS[kind], i, n)
            obj = make()
            rc = refused_once(kind, i, lambda: call(obj), where)
            expect(rc in codes, "%s: status %d (%s); one of %s expected" % (where, rc, last_error(), [CODE_NAMES[c] for c in codes]))
            rc2 = call(obj)
            expect(rc2 == sm.OK, "%s: the same call afterwards, unhindered, failed with status %d (%s)" % (where, rc2, last_error()))
            got = check(obj)
            if want is not None:
                same(got, want, where + ", then called again")
            destroy(obj)
            torch.cuda.synchronize()
            require_same(base, snap(), where + " (status %s), called again, destroyed" % CODE_NAMES[rc])
            seen[i] = rc
        report_sweep(what, kind, n, seen)


def sweep_call(what, call, kinds=(DEVICE,), codes=ANY_CODE):
    """call() -> status: a call that frees its work space on every way out.  After a refusal the snapshot is back at once, and the
    call works again."""
    import torch

    for kind in kinds:
        base = snap()
        n, rc = count_obtains(kind, call)
        expect(rc == sm.OK, "%s: the unhindered call failed with status %d (%s)" % (what, rc, last_error()))
        torch.cuda.synchronize()
        require_same(base, snap(), "%s: unhindered" % what)
        seen = {}
        for i in range(1, n + 1):
            where = "%s with %s call %d of %d refused" % (what, KINDS[kind], i, n)
            rc = refused_once(kind, i, call, where)
            expect(rc in codes, "%s: status %d (%s); one of %s expected" % (where, rc, last_error(), [CODE_NAMES[c] for c in codes]))
            torch.cuda.synchronize()
            require_same(base, snap(), where + " (status %s)" % CODE_NAMES[rc])
            seen[i] = rc
        rc = call()
        expect(rc == sm.OK, "%s: the call after the sweep failed with status %d" % (what, rc))
        torch.cuda.synchronize()
        require_same(base, snap(), "%s: after the sweep" % what)
        report_sweep(what, kind, n, seen)


def raw_csr_create(rows, cols, arrays, mem_kind, host_rp=None, first_row=None):
    out = C.c_void_p()
    rp, ci, v = arrays
    ptr = sm._p if mem_kind == sm.MEM_HOST else sm._dev_ptr
    nnz = int((rp if host_rp is None else host_rp)[rows])
    if first_row is None:
        rc = status("smvp_csr_create", C.byref(out), 0, rows, cols, nnz, ptr(rp), ptr(ci), ptr(v), mem_kind, None if host_rp is None else sm._p(host_rp))
    else:
        rc = status("smvp_csr_create_block", C.byref(out), 0, rows, cols, nnz, ptr(rp), ptr(ci), ptr(v), mem_kind,
                    None if host_rp is None else sm._p(host_rp), first_row)
    return rc, out.value


def csr_destroy(h):
    sm.lib().smvp_csr_destroy(C.c_void_p(h))


def group_sweep_csr():
    import torch

    import ilu0_method as im
    import mixed_structures as ms

    m, n, _, csr = sample("memplus.mtx")
    sweep_create("smvp_csr_create, host arrays (memplus)", lambda: raw_csr_create(m, n, csr, sm.MEM_HOST), csr_destroy)
    d_csr = tuple(dev(a) for a in csr)
    sweep_create("smvp_csr_create, adopted arrays (memplus)", lambda: raw_csr_create(m, n, d_csr, sm.MEM_DEVICE, host_rp=csr[0]), csr_destroy)
    name = ms.BLOCKS[0]
    brows, bcols, row0, _ = ms.structure(name)
    bcsr = ms.csr_of(name)
    sweep_create("smvp_csr_create_block (%s)" % name, lambda: raw_csr_create(brows, bcols, bcsr, sm.MEM_HOST, first_row=row0), csr_destroy)
    expect((d_csr[1].cpu().numpy() == csr[1]).all(), "an adopted array changed")

    # every family of smvp_csr_set_kernel on an existing handle (a VECTOR handle holds no plan)
    S, _, _, scsr = synth()
    # memplus runs every family; the 2^16 block adds the builders whose allocation lists depend on the matrix: the column sweep
    # (plain and XCD parts) and both near forms of BINNED, whose far part memplus barely has.  The tile plans' lists are the same
    # on every matrix, so they are not repeated there.
    big = {"COLSWEEP", "COLSWEEP parts 8", "BINNED near=0 overlap=1", "BINNED near=1 overlap=0"}
    for label, rows, cols, arrays, which in (("memplus", m, n, csr, None), ("synth 2^16", S, S, scsr, big)):
        x = dev(np.random.default_rng(1).random(cols))

        def make():
            A = sm.CsrMatrix(rows, cols, *arrays)
            A.set_kernel(sm.CSR_KERNEL_VECTOR, 0)
            return A

        for plan in csr_plans(rows):
            pname, opts, kernel, param = plan
            if pname.startswith("VECTOR") or (which is not None and pname not in which):
                continue

            def call(A):
                with options(opts):
                    return status("smvp_csr_set_kernel", A._h, kernel, param)

            kinds = (DEVICE, STREAM, EVENT) if kernel == sm.CSR_KERNEL_BINNED else (DEVICE,)
            sweep_handle("smvp_csr_set_kernel %s (%s)" % (pname, label), make, call, lambda A: csr_product(A, x), lambda A: A.close(), kinds)

    # the first smvp_csr_spmm
    k = 3
    X = dev(np.random.default_rng(2).random((n, k)))

    def spmm(A):
        Y = torch.full((m, k), float("nan"), dtype=torch.float64, device="cuda")
        A._Y = Y
        return status("smvp_csr_spmm", A._h, k, sm._dev_ptr(X), k, sm._dev_ptr(Y), k, None)

    def spmm_bits(A):
        torch.cuda.synchronize()
        return A._Y.cpu().numpy().ravel()

    sweep_handle("the first smvp_csr_spmm (memplus)", lambda: sm.CsrMatrix(m, n, *csr), spmm, spmm_bits, lambda A: A.close())

    # smvp_csr_create_transposed: SMVP_ERR_ALLOC when memory runs out (nothing leaked), *out NULL after every failure
    A = sm.CsrMatrix(m, n, *csr)

    def transposed():
        out = C.c_void_p(0xdead0)
        rc = status("smvp_csr_create_transposed", C.byref(out), A._h, None)
        return rc, out.value

    sweep_create("smvp_csr_create_transposed (memplus)", transposed, csr_destroy, codes=(sm.ERR_ALLOC,))
    A.close()

    # smvp_csr_trsv_create and smvp_csr_ilu0_create
    G = im.as_matrix(im.grid(24))
    A = sm.CsrMatrix(G.n, G.n, *G.csr)
    for uplo, diag in ((sm.TRSV_LOWER, sm.TRSV_DIAG_STORED), (sm.TRSV_UPPER, sm.TRSV_DIAG_UNIT)):
        def trsv_create():
            out = C.c_void_p()
            rc = status("smvp_csr_trsv_create", C.byref(out), A._h, uplo, diag, None)
            return rc, out.value

        sweep_create("smvp_csr_trsv_create (uplo %d, diag %d)" % (uplo, diag), trsv_create, lambda t: sm.lib().smvp_trsv_destroy(C.c_void_p(t)))

    def ilu0_create():
        out = C.c_void_p()
        rc = status("smvp_csr_ilu0_create", C.byref(out), A._h, None)
        return rc, out.value

    sweep_create("smvp_csr_ilu0_create", ilu0_create, lambda f: sm.lib().smvp_ilu0_destroy(C.c_void_p(f)))
    A.close()


def group_sweep_tjds():
    import torch

    m, n, coo, _ = sample("memplus.mtx")
    t = sm.tjds_from_coo(coo, m, n)
    x = dev(np.random.default_rng(1).random(n))

    def raw_create(arrays, mem_kind):
        out = C.c_void_p()
        ptr = sm._p if mem_kind == sm.MEM_HOST else sm._dev_ptr
        rc = status("smvp_tjds_create", C.byref(out), 0, m, n, t.nnz, t.num_diag, ptr(arrays[0]), ptr(arrays[1]), ptr(arrays[2]), ptr(arrays[3]), mem_kind)
        return rc, out.value

    host = (t.perm, t.start_pos, t.row_ind, t.val)
    adopted = tuple(dev(a) for a in host)
    destroy = lambda h: sm.lib().smvp_tjds_destroy(C.c_void_p(h))   # noqa: E731
    for index in (0, 1, 2):                            # (the create builds the row-gather plan of that index stream)
        with options({"tjds_index": index}):
            sweep_create("smvp_tjds_create, host arrays, tjds_index %d (memplus)" % index, lambda: raw_create(host, sm.MEM_HOST), destroy)
    sweep_create("smvp_tjds_create, adopted arrays (memplus)", lambda: raw_create(adopted, sm.MEM_DEVICE), destroy)
    expect((adopted[2].cpu().numpy() == t.row_ind).all(), "an adopted array changed")

    make = lambda: sm.TjdsMatrix(t)                    # noqa: E731
    close = lambda T: T.close()                        # noqa: E731
    bits = lambda T: tjds_product(T, x)                # noqa: E731
    # ATOMIC and the ref-quirks product add in the order the hardware takes the atomics: no two runs give the same bits, so those
    # two products are held to the rounding bound of smoke(), 1e-9 * sum |a x| per row, instead
    _, _, _, (rp, ci, v) = sample("memplus.mtx")
    scale = ob.csr_spmv(rp, ci, np.abs(v), np.abs(x.cpu().numpy()))

    def close_enough(got, want, what):
        expect(np.all(np.abs(got - want) <= 1e-9 * scale), "%s: the product is off by more than 1e-9 * sum |a x|" % what)

    for mode in (sm.TJDS_MODE_TWO_PHASE, sm.TJDS_MODE_ATOMIC):
        sweep_handle("smvp_tjds_set_mode(%d)" % mode, make, lambda T: status("smvp_tjds_set_mode", T._h, mode), bits, close,
                     same=close_enough if mode == sm.TJDS_MODE_ATOMIC else same_bits)
    for index in (0, 1, 2):                            # (index 2, 32-bit columns in row order, has no value cache: set_tile only)
        with options({"tjds_index": index}):
            for tile in (256, 1024, 2048):
                sweep_handle("smvp_tjds_set_tile(%d), tjds_index %d" % (tile, index), make, lambda T: status("smvp_tjds_set_tile", T._h, tile), bits, close)
            for min_tiles in (0, 2, 4) if index != 2 else ():
                sweep_handle("smvp_tjds_set_value_cache(%d), tjds_index %d" % (min_tiles, index), make,
                             lambda T: status("smvp_tjds_set_value_cache", T._h, min_tiles), bits, close)
    sweep_handle("smvp_tjds_set_ref_quirks(on)", make, lambda T: status("smvp_tjds_set_ref_quirks", T._h, 1, t.ref_num_tjdiag, t.last_diag_single),
                 bits, close, same=close_enough)
    k = 3
    X = dev(np.random.default_rng(2).random((n, k)))

    def spmm(T):
        Y = torch.full((m, k), float("nan"), dtype=torch.float64, device="cuda")
        T._Y = Y
        return status("smvp_tjds_spmm", T._h, k, sm._dev_ptr(X), k, sm._dev_ptr(Y), k, None)

    def spmm_bits(T):
        torch.cuda.synchronize()
        return T._Y.cpu().numpy().ravel()

    sweep_handle("the first smvp_tjds_spmm (memplus)", make, spmm, spmm_bits, close)


def group_sweep_calls():
    import torch

    import cg_method as cg

    # the device conversions: the outputs are the caller's, the scratch is the call's
    m, n, coo, _ = sample("memplus.mtx")
    nnz = len(coo)
    d_coo = dev(np.frombuffer(np.ascontiguousarray(coo, dtype=sm.COO_DTYPE).tobytes(), dtype=np.uint8))
    i32 = lambda k: torch.empty(max(k, 1), dtype=torch.int32, device="cuda")   # noqa: E731
    rp, ci, v = i32(m + 1), i32(nnz), torch.empty(nnz, dtype=torch.float64, device="cuda")
    P = sm._dev_ptr
    sweep_call("smvp_csr_from_coo_device (memplus)", lambda: status("smvp_csr_from_coo_device", P(d_coo), m, n, nnz, P(rp), P(ci), P(v), None))
    cap = max(m, nnz) + 2
    perm, sp, ri = i32(n), i32(cap), i32(nnz)
    nd, rn, ls = C.c_int(), C.c_int(), C.c_int()
    sweep_call("smvp_tjds_from_coo_device (memplus)",
               lambda: status("smvp_tjds_from_coo_device", P(d_coo), m, n, nnz, P(perm), P(sp), cap, P(ri), P(v), C.byref(nd), C.byref(rn), C.byref(ls), None))
    # one solver of each kind, and the power method, on a CSR and on a TJDS handle: the work space has device and pinned memory
    M = cg.spd(300)
    A, T, plans = solver_handles(M)
    db, dm = dev(cg.rhs(300)), dev(np.ones(300))
    for H, name in ((A, "csr"), (T, "tjds")):
        for fn, call, _ in solver_calls(H, 300, db, None, dm, plans, 12, 1e-10):
            sweep_call("smvp_%s_%s" % (name, fn.replace(" ", ", ")), call, kinds=(DEVICE, PINNED))
    for Q in plans:
        Q.close()
    T.close()
    A.close()
    # the timed entry points: a stream, events, the operands, the timers' buffers, the handle and (device_convert) the arrays
    m, n, coo, _ = sample("ibm32.mtx")
    y, ms, st = np.zeros(m), np.zeros(3), sm.TimeStats()
    for fn in ("smvp_csr_compute", "smvp_tjds_compute"):
        for timing in (sm.TIMING_EVENTS, sm.TIMING_DEVICE):
            for convert in (False, True):
                o, _ = sm._run_opts(0, sm.CSR_KERNEL_AUTO, 0, False, None, device_convert=convert, timing=timing)
                sweep_call("%s (ibm32, 3 products, timing %d, device_convert %d)" % (fn, timing, convert),
                           lambda: status(fn, sm._p(coo), m, n, len(coo), 3, C.byref(o), sm._p(y), sm._p(ms), C.byref(st)),
                           kinds=(DEVICE, STREAM, EVENT))


    # the sharded layer's creates on one GPU with two virtual ranks of two chunks: per rank two streams, the events, the vectors,
    # and a handle per chunk (its RCCL communicators are not counted and not created by the push forms)
    m, n, coo, (rp, ci, v) = sample("memplus.mtx")
    so = sm.ShardOpts()
    sm.lib().smvp_shard_opts_default(C.byref(so))
    so.chunks, so.exchange = 2, sm.EXCHANGE_COPIES
    devs = (C.c_int * 2)(0, 0)
    coo_c = np.ascontiguousarray(coo, dtype=sm.COO_DTYPE)

    def sharded_csr():
        out = C.c_void_p()
        return status("smvp_csr_sharded_create_ex", C.byref(out), 2, devs, m, n, len(ci), sm._p(rp), sm._p(ci), sm._p(v), C.byref(so)), out.value

    def sharded_tjds():
        out = C.c_void_p()
        return status("smvp_tjds_sharded_create_ex", C.byref(out), 2, devs, sm._p(coo_c), m, n, len(coo_c), C.byref(so)), out.value

    for what, create in (("smvp_csr_sharded_create_ex", sharded_csr), ("smvp_tjds_sharded_create_ex", sharded_tjds)):
        sweep_create(what + " (memplus, 2 virtual ranks x 2 chunks)", create, lambda h: sm.lib().smvp_sharded_destroy(C.c_void_p(h)),
                     kinds=(DEVICE, STREAM, EVENT))


# ==================================================================================================== plan_bytes against what is held
# The counted build gives what a plan really holds: the handle's live device bytes minus those of the same handle without the
# plan.  smvp_*_plan_info().plan_bytes -- "bytes the plan keeps beside them (second copies included)" -- may differ from that
# by the padding of the allocation sizes only.  Every allocation helper of csrc/ rounds a count up to four elements
# (`std::max<size_t>(count, 4)` in upload / Scratch::get / own, `std::max(nnz, 4)`, `std::max(rows, 4)`): at most four elements of
# at most eight bytes, 32 bytes, where the count is 0.  The explicit pads are smaller: `rows + 4` ints (16 bytes; reported as
# held), `nnz + 8` 16-bit offsets (16 bytes), `ntiles + 2` ints (reported as held), one more tile of column bases (4 bytes).  The
# one array of wider elements is the TJDS work list of int4 (upload: up to four of 16 bytes, 64 bytes).
PAD_PER_ALLOCATION = 32
PAD_WORK_LIST = 64


def compare_bytes(what, reported, held, allocations, extra=0):
    allowance = PAD_PER_ALLOCATION * allocations + extra
    # every pad in csrc/ rounds a size UP (a floor of four elements, + 4, + 8, + 2, one more tile), and plan_info counts the
    # unpadded sizes: the report is never above what is held, and below it by the pads at the most.  A plan_info that forgot an
    # array fails the upper side as soon as the array is larger than the pads; one that counted an array twice fails the lower.
    ok = 0 <= held - reported <= allowance
    print("plan_bytes %-58s reported %12.0f  held %12d  allocations %3d  allowance %5d  %s" % (
        what, reported, held, allocations, allowance, "ok" if ok else "DIFFERS by %+.0f" % (reported - held)))
    return ok


def group_plan_bytes():
    import torch

    bad = []
    k = 3
    for label, (rows, cols, coo, csr) in (("memplus", sample("memplus.mtx")), ("synth 2^16", synth())):
        nnz = len(coo)
        # ---- CSR
        before = snap()
        A = sm.CsrMatrix(rows, cols, *csr)
        A.set_kernel(sm.CSR_KERNEL_VECTOR, 0)
        bare = snap()
        own = at(bare, DEVICE, BYTES) - at(before, DEVICE, BYTES)
        expect(at(bare, DEVICE, LIVE) - at(before, DEVICE, LIVE) == 3, "csr %s on VECTOR holds more than its three arrays" % label)
        if not compare_bytes("csr %s: matrix_bytes" % label, A.plan_info()["matrix_bytes"], own, 3):
            bad.append("csr %s matrix_bytes" % label)
        expect(A.plan_info()["plan_bytes"] == 0, "csr %s on VECTOR reports plan bytes" % label)
        for plan in csr_plans(rows):
            set_plan(A, plan)
            now = snap()
            held, allocs = at(now, DEVICE, BYTES) - at(bare, DEVICE, BYTES), at(now, DEVICE, LIVE) - at(bare, DEVICE, LIVE)
            if not compare_bytes("csr %s: %s" % (label, plan[0]), A.plan_info()["plan_bytes"], held, allocs):
                bad.append("csr %s %s" % (label, plan[0]))
        A.set_kernel(sm.CSR_KERNEL_VECTOR, 0)
        X = dev(np.random.default_rng(2).random((cols, k)))
        Y = torch.empty((rows, k), dtype=torch.float64, device="cuda")
        expect(A.spmm_describe(k)[2]["plan_bytes"] == 0, "the SpMM plan reports bytes before the first spmm")
        A.spmm(X, Y)
        torch.cuda.synchronize()
        now = snap()
        if not compare_bytes("csr %s: the SpMM plan" % label, A.spmm_describe(k)[2]["plan_bytes"], at(now, DEVICE, BYTES) - at(bare, DEVICE, BYTES),
                             at(now, DEVICE, LIVE) - at(bare, DEVICE, LIVE)):
            bad.append("csr %s spmm" % label)
        A.close()
        # ---- TJDS.  A handle is created in ROW_GATHER mode with that mode's plan, and a mode's plan is kept when the mode changes:
        # no mode of an existing handle is without plans, so what the plans hold is the handle's live bytes minus those of its own
        # four arrays -- which matrix_bytes is held to, as for CSR.
        t = sm.tjds_from_coo(coo, rows, cols)
        for index in (0, 1, 2):
            with options({"tjds_index": index}):
                before = snap()
                T = sm.TjdsMatrix(t)
                # (not read from the counters, which see the handle whole: the sizes smvp::upload gives the four arrays.  What is
                # held against live bytes is the sum, arrays + plans, in the rows below.)
                own = sum(max(len(a), 4) * a.itemsize for a in (t.perm, t.start_pos, t.row_ind, t.val))
                if not compare_bytes("tjds %s: matrix_bytes (held: upload's sizes)" % label, T.plan_info()["matrix_bytes"], own, 4):
                    bad.append("tjds %s matrix_bytes" % label)
                steps = [("ROW_GATHER (as created)", lambda: None), ("+ TWO_PHASE", lambda: T.set_mode(sm.TJDS_MODE_TWO_PHASE)),
                         ("ATOMIC (both plans kept)", lambda: T.set_mode(sm.TJDS_MODE_ATOMIC)),
                         ("ROW_GATHER, 256-entry tiles", lambda: (T.set_mode(sm.TJDS_MODE_ROW_GATHER), T.set_tile(256))),
                         ("ROW_GATHER, 2048-entry tiles", lambda: T.set_tile(2048)), ("ROW_GATHER, 1024-entry tiles", lambda: T.set_tile(1024))]
                if index != 2:
                    steps += [("value cache 0", lambda: T.set_value_cache(0)), ("value cache 4", lambda: T.set_value_cache(4)),
                              ("value cache 2", lambda: T.set_value_cache(2))]
                steps += [("ref-quirks on", lambda: T.set_ref_quirks(True)), ("ref-quirks off", lambda: T.set_ref_quirks(False))]
                for name, step in steps:
                    step()
                    now = snap()
                    held = at(now, DEVICE, BYTES) - at(before, DEVICE, BYTES) - own
                    allocs = at(now, DEVICE, LIVE) - at(before, DEVICE, LIVE) - 4
                    if not compare_bytes("tjds %s, tjds_index %d: %s" % (label, index, name), T.plan_info()["plan_bytes"], held, allocs,
                                         PAD_WORK_LIST - PAD_PER_ALLOCATION):
                        bad.append("tjds %s index %d %s" % (label, index, name))
                if index == 0:
                    base = snap()
                    X = dev(np.random.default_rng(2).random((cols, k)))
                    Y = torch.empty((rows, k), dtype=torch.float64, device="cuda")
                    T.spmm(X, Y)
                    torch.cuda.synchronize()
                    now = snap()
                    if not compare_bytes("tjds %s: the SpMM plan" % label, T.spmm_describe(k)[2]["plan_bytes"],
                                         at(now, DEVICE, BYTES) - at(base, DEVICE, BYTES), at(now, DEVICE, LIVE) - at(base, DEVICE, LIVE)):
                        bad.append("tjds %s spmm" % label)
                T.close()
    expect(not bad, "plan_info and the bytes really held differ by more than the allocations' padding: " + "; ".join(bad))
    DONE.append("plan_bytes")


GROUPS = {"csr": group_csr, "tjds": group_tjds, "objects": group_objects, "solvers": group_solvers, "sweep_csr": group_sweep_csr,
          "sweep_tjds": group_sweep_tjds, "sweep_calls": group_sweep_calls, "plan_bytes": group_plan_bytes}


def main(argv):
    import torch

    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: resource_scenarios.py {%s}" % " | ".join(GROUPS))
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
        expect(snap()[FOREIGN] == 0, "foreign frees")
    except Failed as e:
        for what in DONE[-3:]:
            print("ok   " + what)
        print("FAIL " + str(e))
        return 1
    print("%d scenarios" % len(DONE))
    print("group %s ok" % argv[1])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
