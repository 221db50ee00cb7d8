"""GPU: the packed tile kernel (csr_stream_owner<8, 6, .>) requesting a tile's plan words together and reading a packable tile's
streams in one flight of loads.

Every product of the family -- forced by name, SMVP_CSR_KERNEL_STREAM_PACKED, under plan option csr_packed = 1 -- is compared with
STREAM's at 2048-entry tiles on the same handle's arrays, bit for bit (int64 views): the family multiplies the very doubles val
holds and sums every row as STREAM does, so there is no tolerance anywhere.  Rows of at most 32 entries are also held to the serial
loop's bits, computed on the host once per case.  tests/tile_record.py has the structures -- the smallest at which the plan words or
the one flight can go wrong -- and tests/test_tile_record_host.py holds the words' own invariants on them; the value sets and what the
plan must find of them come from tests/packed_values.py.  Each structure runs with the read-once form forced off and on, through the
stamped form of a timed entry point, and on a stream of the caller's with x and y still in flight.  y lies in a guarded buffer.
"""
import functools

import numpy as np
import pytest

import packed_values as pv
import smvp_toolkit_amd as sm
import stream_order as so
import tile_record as trec
from parity import check_guards, guarded_y

pytestmark = pytest.mark.gpu

PACKED, STREAM = sm.CSR_KERNEL_STREAM_PACKED, sm.CSR_KERNEL_STREAM
NEW = sorted(trec.NEW_STRUCTURES)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def side(torch):
    return so.side_stream(torch)


@functools.lru_cache(maxsize=None)
def case(name, kind):
    """(rows, cols, row_ptr, col_ind, val, x, the serial loop's y as int64, which rows are short): built once, shared, read-only."""
    rows, cols, rp, ci = trec.STRUCTURES[name]()
    val = pv.values(kind, rp, ci)
    x = np.random.default_rng(24680).random(cols) - 0.25
    serial = np.zeros(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = val * x[ci]                              # every product rounded by itself, as the kernels (built without contraction) do
        for r in range(rows):
            acc = 0.0
            for j in range(int(rp[r]), int(rp[r + 1])):
                acc += prod[j]
            serial[r] = acc
    short = np.diff(rp) <= pv.LONG_ROW
    for a in (rp, ci, val, x, serial, short):
        a.setflags(write=False)
    return rows, cols, rp, ci, val, x, serial.view(np.int64), short


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def product(torch, A, dx, rows, stream=None):
    buf, y = guarded_y(torch, rows)
    A.spmv(dx, y, stream=torch.cuda.current_stream() if stream is None else stream)
    torch.cuda.synchronize()
    check_guards(buf, rows)
    return y.cpu().numpy().view(np.int64)


def plan_packed(A, hint=0, rowrel=1):
    with sm.option("csr_packed", 1), sm.option("csr_read_once", hint), sm.option("csr_rowrel", rowrel):
        A.set_kernel(PACKED, 0)
    assert A.get_kernel() == (PACKED, 2048) and A.describe()[0] == "csr_stream_owner<8, 6, false>" and A.launches() == 1


def plan_stream(A, hint=0, rowrel=1):
    with sm.option("csr_read_once", hint), sm.option("csr_rowrel", rowrel):
        A.set_kernel(STREAM, 2048)
    assert A.get_kernel() == (STREAM, 2048)


def same_bits(got, want, what, mask=None):
    g, w = (got, want) if mask is None else (got[mask], want[mask])
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d rows differ, first %d: %#x against %#x" % (what, bad.size, bad[0], g[bad[0]], w[bad[0]])


def check(name, kind, got, want, serial, short, what):
    """got against STREAM's y and, on the short rows, the serial loop's.  The special value sets put NaNs and infinities into rows
    of every length: the bits of a row a wavefront sums are then those of STREAM only as far as both are NaN (as the family's own
    tests hold it)."""
    if kind.startswith("special"):
        same_bits(got, want, what + " against STREAM", short)
        assert np.array_equal(np.isnan(got.view(np.float64)), np.isnan(want.view(np.float64))), what
        nan = np.isnan(serial.view(np.float64))
        same_bits(got, serial, what + " against the serial loop", short & ~nan)
        assert np.all(np.isnan(got.view(np.float64))[short & nan]), what
    else:
        same_bits(got, want, what + " against STREAM")
        same_bits(got, serial, what + " against the serial loop", short)
        assert not np.isnan(got.view(np.float64)).any(), what


def forced_off_and_on(torch, name, kind, rowrel=1):
    rows, cols, rp, ci, val, x, serial, short = case(name, kind)
    dx = dev(torch, x)
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    try:
        for hint in (0, 1):
            plan_stream(A, hint, rowrel)
            want = product(torch, A, dx, rows)
            plan_packed(A, hint, rowrel)
            got, again = product(torch, A, dx, rows), product(torch, A, dx, rows)
            same_bits(again, got, "%s, %s, read-once %d: the second product against the first" % (name, kind, hint))
            check(name, kind, got, want, serial, short, "%s, %s, read-once %d, row_rel %d" % (name, kind, hint, rowrel))
    finally:
        A.close()


# ------------------------------------------------------------------------------------------------------------ single launches
@pytest.mark.parametrize("kind", pv.KINDS)
def test_six_tiles_and_a_tail_on_every_value_set(torch, kind):
    """Six packable tiles and a partial one; `half` puts a wavefront without escapes next to one with 512 and pads odd counts."""
    forced_off_and_on(torch, "six tiles and a tail", kind)


@pytest.mark.parametrize("kind", ["half", "distinct"])
def test_a_wide_tile_between_packable_ones(torch, kind):
    """The tile behind the wide one takes its escapes where its own plan words say, not where the wide tile's would have ended."""
    rows, cols, rp, ci = trec.STRUCTURES["a wide tile"]()
    assert list(pv.packable_tiles(rp, ci)) == [True, True, True, False, True, True, False]
    forced_off_and_on(torch, "a wide tile", kind)


@pytest.mark.parametrize("kind", ["half", "hot64"])
def test_long_and_giant_rows(torch, kind):
    rows, cols, rp, ci = trec.STRUCTURES["long and giant rows"]()
    lens = np.diff(rp)
    assert (lens > pv.LONG_ROW).any() and lens.max() > pv.OVER
    forced_off_and_on(torch, "long and giant rows", kind)


@pytest.mark.parametrize("kind", ["half", "hot64", "distinct"])
@pytest.mark.parametrize("name", NEW)
def test_the_small_structures(torch, name, kind):
    forced_off_and_on(torch, name, kind)


@pytest.mark.parametrize("name", ["six tiles and a tail", "rows of one and two entries", "empty rows at the tiles' edges"])
def test_without_row_rel_the_generic_path(torch, name):
    """Plan option csr_rowrel = 0: phase 2 reads row_ptr, and a packable tile takes the generic path -- codes and escapes all the same."""
    forced_off_and_on(torch, name, "half", rowrel=0)


# ------------------------------------------------------------------------------------- the stamped form; a stream of the caller's
@pytest.mark.parametrize("name", sorted(trec.STRUCTURES))
def test_the_stamped_form_through_a_timed_entry_point(torch, name):
    """smvp_csr_compute with device timing: single stamped launches of csr_stream_owner<8, 6, true> (the family has no repeating form)."""
    rows, cols, rp, ci, val, x, serial, short = case(name, "half")
    coo = sm.make_coo(np.repeat(np.arange(rows), np.diff(rp)), ci, val)
    want, _, _ = sm.csr_compute(coo, rows, cols, iters=2, kernel=STREAM, param=2048, x=x, timing=sm.TIMING_DEVICE)
    with sm.option("csr_packed", 1):
        got, ms, _ = sm.csr_compute(coo, rows, cols, iters=2, kernel=PACKED, param=0, x=x, timing=sm.TIMING_DEVICE)
    assert np.all(ms > 0) and np.all(ms < 50.0)
    check(name, "half", got.view(np.int64), want.view(np.int64), serial, short, name + ", stamped")


@pytest.mark.parametrize("name", sorted(trec.STRUCTURES))
def test_on_a_stream_of_the_callers_with_x_and_y_in_flight(torch, side, name):
    rows, cols, rp, ci, val, x, serial, short = case(name, "half")
    A = sm.CsrMatrix(rows, cols, rp, ci, val)
    try:
        plan_stream(A)
        want = product(torch, A, dev(torch, x), rows)
        plan_packed(A)
        dx = dev(torch, x)
        buf, y = guarded_y(torch, rows)
        torch.cuda.synchronize()
        pair = so.stage(torch, dx)
        torch.cuda.synchronize()
        ev = so.in_flight(torch, side, [pair], [y])
        so.pending(ev, "before the product")
        A.spmv(dx, y, stream=side)
        so.pending(ev, "after the product had been enqueued")
        (got,), clones = so.read_on(torch, side, [y])
        so.settled(torch, [y], clones, [(buf, rows)], name)
        check(name, "half", got.view(np.int64), want, serial, short, name + ", in flight")
    finally:
        A.close()


# ------------------------------------------------------------------------------------------------- the plan follows the values
def test_a_replan_and_a_set_kernel_after_changed_values(torch):
    """Adopted device arrays whose values change in place: every set_kernel builds the packed arrays again, so the runs of escapes the
    kernel reads are those of the values it multiplies -- `hot64` has none, `distinct` 512 per wavefront, `half` odd and even counts."""
    rows, cols, rp, ci, _, x, _, _ = case("six tiles and a tail", "half")
    sets = [(k, pv.values(k, rp, ci)) for k in ("half", "hot64", "distinct", "half")]
    d_rp, d_ci = (torch.from_numpy(np.array(a)).cuda() for a in (rp, ci))
    d_val = torch.from_numpy(np.array(sets[0][1])).cuda()
    dx = dev(torch, x)
    A = sm.CsrMatrix(rows, cols, d_rp, d_ci, d_val)
    try:
        ys = []
        for i, (kind, v) in enumerate(sets):
            d_val.copy_(torch.from_numpy(v))
            torch.cuda.synchronize()
            plan_stream(A)
            want = product(torch, A, dx, rows)
            if i % 2:
                plan_packed(A)                       # PACKED after STREAM: a plan from nothing
            else:
                plan_packed(A)
                plan_packed(A, hint=1)               # ... and PACKED re-planned in place
            got = product(torch, A, dx, rows)
            same_bits(got, want, "values %d (%s)" % (i, kind))
            ys.append(got)
        assert np.array_equal(ys[0], ys[3]) and not np.array_equal(ys[0], ys[1]) and not np.array_equal(ys[1], ys[2])
    finally:
        A.close()

