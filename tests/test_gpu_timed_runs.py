"""The timed entry points (csr_compute / tjds_compute) on every device-timed form of the tile kernel.

A handle's spmv launches csr_stream_owner<VPT, FLAVOR, false>.  A device-timed run of the entry points never does: it goes
through the repeating kernel csr_stream_owner_repeat<VPT, FLAVOR> (up to 1024 products per launch, a barrier between products
that is one level wide up to 24 workgroups, 8 shards up to 640, 16 beyond) or through the stamped launch
csr_stream_owner<VPT, FLAVOR, true> replayed from a hipGraph in rings of 256.  These tests run both on every (VPT, FLAVOR) the
entry points can resolve to, on every barrier width and on both sides of every ring edge, and hold

  y      to an int64 reference bit for bit (exact operands), to the oracle within parity.check_y's bound and to the bits of the
         plain product of a handle built the same way (real operands), the same bits under all four timing forms;
  times  to timed_runs.check_times: one per product, finite, positive, whole ticks of the device clock, none beyond the loop's
         wall time, windows of one repeating launch not overlapping, statistics that are the times';
  info   to the form that must have run: repeat_launches / graph_replays / repeat_gave_up of smvp_last_run_info.

The structures, operands and references are timed_runs.py's (tested on the host by test_timed_runs_host.py).
"""
import functools
import re

import numpy as np
import pytest

import oracle_binding as ob
import smvp_toolkit_amd as sm
import timed_runs as tr
from parity import check_y
from special_values import check_bits

pytestmark = pytest.mark.gpu

TIMINGS = (sm.TIMING_EVENTS, sm.TIMING_DEVICE, sm.TIMING_DEVICE_GRAPH, sm.TIMING_AUTO)
KINDS = ("exact", "real")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def case(name, tile):
    """A named structure with both sets of operands and their references (x given, and x = None: the row sums of the values),
    computed once and shared read-only."""
    rows, cols, row_ptr, col_ind = tr.structure(name, tile)
    nnz = int(row_ptr[-1])
    c = {"rows": rows, "cols": cols, "row_ptr": row_ptr, "col_ind": col_ind, "nnz": nnz, "terms": np.diff(row_ptr)}
    ones = np.ones(cols)
    for kind, (val, x) in (("exact", tr.exact_operands(nnz, cols)), ("real", tr.real_operands(nnz, cols))):
        k = {"val": val, "x": x, "coo": tr.coo_of(row_ptr, col_ind, val)}
        if kind == "exact":
            k["ref"] = {True: tr.exact_reference(row_ptr, col_ind, val, x), False: tr.exact_reference(row_ptr, col_ind, val, ones)}
        else:
            k["ref"] = {True: ob.csr_spmv(row_ptr, col_ind, val, x), False: ob.csr_spmv(row_ptr, col_ind, val, ones)}
            k["scale"] = {True: tr.row_scale(row_ptr, col_ind, val, x), False: tr.row_scale(row_ptr, col_ind, val, ones)}
        for a in [val, x, k["coo"]] + list(k["ref"].values()) + list(k.get("scale", {}).values()):
            a.setflags(write=False)
        c[kind] = k
    for a in (row_ptr, col_ind):
        a.setflags(write=False)
    return c


class options:
    """Several plan options at once around a compute call or the construction of a handle (they are process-wide and read when
    the plan is built)."""

    def __init__(self, **kw):
        self.ctx = [sm.option(k, v) for k, v in kw.items()]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()

    def __exit__(self, *exc):
        for c in reversed(self.ctx):
            c.__exit__(*exc)
        return False


def form_of(describe):
    m = re.fullmatch(r"csr_stream_owner<(\d+), (\d+), false>", describe[0])
    assert m, describe[0]
    return int(m.group(1)), int(m.group(2))


def handle_product(torch, fmt, c, kind, x_given, param=0):
    """(y, (vpt, flavor)): the plain product of a handle built under the plan options in force -- CsrMatrix.set_kernel(STREAM,
    param) then spmv, TjdsMatrix then set_x and spmv -- into a y full of NaN, and the kernel it resolved to."""
    k = c[kind]
    dx = torch.from_numpy(np.array(k["x"] if x_given else np.ones(c["cols"]), dtype=np.float64)).cuda()   # (a copy: the case is read-only)
    dy = torch.full((c["rows"],), float("nan"), dtype=torch.float64, device="cuda")
    if fmt == "csr":
        H = sm.CsrMatrix(c["rows"], c["cols"], c["row_ptr"], c["col_ind"], k["val"])
        H.set_kernel(sm.CSR_KERNEL_STREAM, param)
        H.spmv(dx, dy)
    else:
        H = sm.TjdsMatrix(sm.tjds_from_coo(k["coo"], c["rows"], c["cols"]))
        H.set_x(dx)
        H.spmv(dy)
    torch.cuda.synchronize()
    form = form_of(H.describe())
    H.close()
    return dy.cpu().numpy(), form


def timed(fmt, c, kind, x_given, timing, iters, param=0):
    """One run of an entry point; the times are checked here (check_times), y and the run's info go back."""
    k = c[kind]
    x = k["x"] if x_given else None
    if fmt == "csr":
        y, ms, st = sm.csr_compute(k["coo"], c["rows"], c["cols"], iters=iters, x=x, timing=timing,
                                   kernel=sm.CSR_KERNEL_STREAM if param else sm.CSR_KERNEL_AUTO, param=param)
    else:
        y, ms, st = sm.tjds_compute(k["coo"], c["rows"], c["cols"], iters=iters, x=x, timing=timing)
    info = sm.last_run_info()
    print("%s %s x=%s timing %d iters %d: timing %d launches %d replays %d gave_up %d wall %.3f ms, min / mean / max %.5f / %.5f / %.5f ms" % (
        fmt, kind, "given" if x_given else "None", timing, iters, info.timing, info.repeat_launches, info.graph_replays,
        info.repeat_gave_up, info.wall_ms, ms.min(), ms.mean(), ms.max()))
    tr.check_times(ms, st, info, iters)
    return y, info


def check_product(c, kind, x_given, y, what):
    k = c[kind]
    if kind == "exact":
        check_bits(y, k["ref"][x_given], what + ": the int64 reference's bits")
    else:
        check_y(y, k["ref"][x_given], k["scale"][x_given], c["terms"])
        check_bits(y[c["terms"] == 0], np.zeros(int((c["terms"] == 0).sum())), what + ": +0.0 in empty rows")


def check_info(info, timing, iters, repeating):
    """The form that must have run.  repeating: the resolved kernel has a repeating instantiation and its grid is resident at
    once.  A launch that gave up at the default patience is a failure whatever was asked."""
    launches, replays = (info.repeat_launches, info.graph_replays)
    assert info.repeat_gave_up == 0, "the repeating launch gave up at a barrier"
    if timing == sm.TIMING_EVENTS:
        assert (info.timing, launches, replays) == (sm.TIMING_EVENTS, 0, 0)
    elif timing == sm.TIMING_DEVICE_GRAPH or not repeating:
        assert (info.timing, launches, replays) == (sm.TIMING_DEVICE, 0, tr.ceil_div(iters, tr.GRAPH_RING))
    else:                                      # TIMING_DEVICE, and TIMING_AUTO for a launch of at most 4096 workgroups
        assert (info.timing, launches, replays) == (sm.TIMING_DEVICE, tr.ceil_div(iters, tr.REPEAT_RING), 0)


# ------------------------------------------------------------------------------- (a) every reachable form, every timing form
# (format, structure, tile the structure is sized for, plan options, the kernel (vpt, flavor) it must resolve to).  CSR names its
# tile; 16-bit column offsets exist for tiles of 1024 and 2048 only, so at 256 the plan keeps (1, Csr) whatever csr_col16 says.
# A TJDS run cannot name its tile (smvp_run_opts_t has no such field): the plan takes 256 below 512 K entries, 1024 from there and
# 2048 from 12 M entries on, so t25 reaches the forms at 256 and t640 sized for 1024 (655 K entries) those at 1024; tjds_index 2
# is the row-ordered stream TjdsK, which has no repeating instantiation.
COMBOS = [
    ("csr", "t25", 256, {"csr_col16": 0}, (1, tr.CSR)),
    ("csr", "t25", 256, {"csr_col16": 1}, (1, tr.CSR)),
    ("csr", "t25", 1024, {"csr_col16": 0}, (4, tr.CSR)),
    ("csr", "t25", 1024, {"csr_col16": 1}, (4, tr.CSR16)),
    ("csr", "t25", 2048, {"csr_col16": 0}, (8, tr.CSR)),
    ("csr", "t25", 2048, {"csr_col16": 1}, (8, tr.CSR16)),
    ("csr", "t25", 1024, {"csr_col16": 0, "csr_rowrel": 0}, (4, tr.CSR)),
    ("csr", "t25", 1024, {"csr_col16": 1, "csr_rowrel": 0}, (4, tr.CSR16)),
    ("tjds", "t25", 256, {"tjds_index": 0}, (1, tr.TJDS_H)),
    ("tjds", "t25", 256, {"tjds_index": 1}, (1, tr.TJDS_S)),
    ("tjds", "t25", 256, {"tjds_index": 2}, (1, tr.TJDS_K)),
    ("tjds", "t640", 1024, {"tjds_index": 0}, (4, tr.TJDS_H)),
    ("tjds", "t640", 1024, {"tjds_index": 1}, (4, tr.TJDS_S)),
]
# The repeating instantiations the entry points can reach with matrices of at most 1.45 M entries.  The other two of the eleven,
# (8, TjdsS) and (8, TjdsH), are the plan's choice for a TJDS stream of 12 M entries or more only: not run here.
REACHABLE_REPEAT_FORMS = {(1, tr.CSR), (4, tr.CSR), (8, tr.CSR), (4, tr.CSR16), (8, tr.CSR16),
                          (1, tr.TJDS_S), (1, tr.TJDS_H), (4, tr.TJDS_S), (4, tr.TJDS_H)}
COMBO_IDS = ["%s-%s-%d-%s" % (f, n, t, "-".join("%s%d" % (k.split("_")[-1], v) for k, v in o.items())) for f, n, t, o, _ in COMBOS]


@pytest.mark.parametrize("fmt,name,tile,opts,form", COMBOS, ids=COMBO_IDS)
def test_every_form_under_every_timing(torch, fmt, name, tile, opts, form):
    """260 products (one repeating launch; two graph replays, the second a ring of 4 with a graph of its own) of every reachable
    kernel form under the four timing forms, exact and real operands, x given and x = None."""
    c = case(name, tile)
    param = tile if fmt == "csr" else 0
    iters = 260
    for kind in KINDS:
        for x_given in (True, False):
            with options(**opts):
                want, got_form = handle_product(torch, fmt, c, kind, x_given, param)
            assert got_form == form, (got_form, form)
            check_product(c, kind, x_given, want, "the handle's plain product")
            for timing in TIMINGS:
                with options(**opts):
                    y, info = timed(fmt, c, kind, x_given, timing, iters, param)
                what = "%s %s %r x %s timing %d" % (fmt, name, opts, "given" if x_given else "None", timing)
                check_product(c, kind, x_given, y, what)
                check_bits(y, want, what + ": the bits of the handle's plain product (and so of every timing form)")
                check_info(info, timing, iters, form in tr.REPEAT_FORMS)


def test_the_reachable_repeating_forms_all_ran(torch):
    """Every combination once more under TIMING_DEVICE: the set of kernels that ran as ONE repeating launch is exactly the set of
    repeating instantiations the entry points can reach."""
    seen = set()
    for fmt, name, tile, opts, _ in COMBOS:
        c = case(name, tile)
        with options(**opts):
            _, form = handle_product(torch, fmt, c, "exact", True, tile if fmt == "csr" else 0)
            y, info = timed(fmt, c, "exact", True, sm.TIMING_DEVICE, 3, tile if fmt == "csr" else 0)
        check_product(c, "exact", True, y, "%s %s %r" % (fmt, name, opts))
        print(fmt, name, tile, opts, "->", form, tr.regime(c["nnz"], tile, fmt)["grid"], "workgroups")
        if info.repeat_launches == 1 and info.repeat_gave_up == 0 and info.graph_replays == 0:
            seen.add(form)
    assert seen == REACHABLE_REPEAT_FORMS, (sorted(seen), sorted(REACHABLE_REPEAT_FORMS))
    assert seen <= tr.REPEAT_FORMS and tr.REPEAT_FORMS - seen == {(8, tr.TJDS_S), (8, tr.TJDS_H)}


# ------------------------------------------------------------------------------------------------------- (b) barrier widths
# Which grids are resident at once -- at most (occupancy - 1) * CUs * 3 / 4 workgroups, repeat_capacity() -- and so took the
# repeating form on the MI355X, for (1, Csr) and (1, TjdsH).  Grids up to 640 must; 720 and 792 are recorded from the device.
REPEATING_ON_MI355X = {8: True, 24: True, 32: True, 640: True, 720: True, 792: True}
WIDTHS = [("csr", n) for n in ("t1", "t24", "t25", "t640", "t641", "t705")] + [("tjds", "t25"), ("tjds", "t640")]


@pytest.mark.parametrize("fmt,name", WIDTHS, ids=["%s-%s" % w for w in WIDTHS])
def test_barrier_widths(torch, fmt, name):
    """40 products in one repeating launch on each barrier shape: one level with 8 workgroups (7 of them own no tile) and with
    24, 8 shards at 32 and at 640 workgroups, 16 shards at 720 (45 members each) and at 792 (50 and 49 members).
    On the MI355X the grids of 8, 24, 32, 640, 720 and 792 workgroups all took the repeating form."""
    tile, iters = 256, 40
    c = case(name, tile)
    g = tr.regime(c["nnz"], tile, fmt)
    assert (g["ntiles"], g["grid"], g["shards"]) == tr.NAMED[name]
    for kind in KINDS:
        want, form = handle_product(torch, fmt, c, kind, True, tile if fmt == "csr" else 0)
        assert form == ((1, tr.CSR) if fmt == "csr" else (1, tr.TJDS_H))
        y, info = timed(fmt, c, kind, True, sm.TIMING_DEVICE, iters, tile if fmt == "csr" else 0)
        what = "%s %s %s, grid %d, %d shards" % (fmt, name, kind, g["grid"], g["shards"])
        check_product(c, kind, True, y, what)
        check_bits(y, want, what + ": the bits of the handle's plain product")
        check_info(info, sm.TIMING_DEVICE, iters, REPEATING_ON_MI355X[g["grid"]])


# ---------------------------------------------------------------------------------------------------------- (d) ring edges
@pytest.mark.parametrize("name", ["t1", "t25"])
@pytest.mark.parametrize("fmt", ["csr", "tjds"])
def test_ring_edges(torch, fmt, name):
    """Either side of the rings: 256 products per graph replay (257 and 513 end in a ring of one product, which instantiates a
    second graph), 1024 per repeating launch (the host waits for the first launch of a run before it queues the others).  The
    default forms: (1, Csr) and (1, TjdsH)."""
    c = case(name, 256)
    first, _ = timed(fmt, c, "exact", True, sm.TIMING_EVENTS, 1)
    check_product(c, "exact", True, first, "%s %s, one product" % (fmt, name))
    for timing, counts in ((sm.TIMING_DEVICE_GRAPH, (1, 2, 255, 256, 257, 513)), (sm.TIMING_DEVICE, (1, 1023, 1024, 1025, 2049))):
        for iters in counts:
            y, info = timed(fmt, c, "exact", True, timing, iters)
            check_bits(y, first, "%s %s timing %d, %d products: the bits of one product" % (fmt, name, timing, iters))
            check_info(info, timing, iters, True)


# ------------------------------------------------------------------------------ (e) edge structures through the entry points
PATHS = {"csr_auto": (sm.csr_compute, {}), "csr_stream": (sm.csr_compute, {"kernel": sm.CSR_KERNEL_STREAM, "param": 1024}),
         "tjds": (sm.tjds_compute, {})}
CONVERT_ON_DEVICE_TOO = ("leading_and_trailing_empty_rows", "rows_just_past_a_tile_edge")


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("name", tr.EDGES)
def test_edge_structures_through_the_entry_points(torch, name, path):
    """Under TIMING_AUTO every edge structure runs: y is the oracle's (+0.0 in empty rows, no NaN left of the poisoned y), the
    times are times.  Under explicit TIMING_DEVICE it runs the same way, or -- where the product cannot stamp itself: STREAM_CARRY
    (AUTO's kernel for a row of 16385 entries) and a matrix without rows, whose product launches nothing -- is refused with
    SMVP_ERR_UNSUPPORTED (timed_runs.device_timing_is_refused); AUTO then times with events."""
    rows, cols, row_ptr, col_ind, val, x = tr.edge(name)
    coo = tr.coo_of(row_ptr, col_ind, val)
    fn, kw = PATHS[path]
    refused = tr.device_timing_is_refused(name, path)
    ref = ob.csr_spmv(row_ptr, col_ind, val, x) if rows else np.zeros(0)
    scale = tr.row_scale(row_ptr, col_ind, val, x) if rows else np.zeros(0)
    terms = np.diff(row_ptr)
    iters = 5
    for convert in (False, True) if name in CONVERT_ON_DEVICE_TOO else (False,):
        for timing in (sm.TIMING_AUTO, sm.TIMING_DEVICE):
            if timing == sm.TIMING_DEVICE and refused:
                with pytest.raises(sm.SmvpError) as e:
                    fn(coo, rows, cols, iters=iters, x=x, timing=timing, device_convert=convert, **kw)
                assert e.value.code == sm.ERR_UNSUPPORTED, str(e.value)
                continue
            y, ms, st = fn(coo, rows, cols, iters=iters, x=x, timing=timing, device_convert=convert, **kw)
            info = sm.last_run_info()
            print(name, path, "convert", convert, "timing", timing, "->", info.timing, info.repeat_launches, info.graph_replays, ms)
            assert info.timing == (sm.TIMING_EVENTS if refused else sm.TIMING_DEVICE) and info.repeat_gave_up == 0
            tr.check_times(ms, st, info, iters, positive=rows > 0)
            assert y.shape == (rows,)
            check_y(y, ref, scale, terms)
            check_bits(y[terms == 0], np.zeros(int((terms == 0).sum())), "+0.0 in empty rows")
