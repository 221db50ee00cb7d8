"""The tile kernel's 16-bit column offsets in lane order and its read-once streams (csr_stream_owner<4 | 8, 5, .>): y must not
notice either.

At 2048-entry tiles the plan keeps the offsets of a full, narrow tile at smvp_tile_map.h's col16_slot, so that a lane reads its 8
offsets with one load; 1024-entry tiles, the last, partial tile and the wide tiles keep the entry order, and the array is laid
out for one tile size: a handle whose tile size changes gets a new one.  A plan may also ask for the kernel form whose val and
col16 loads carry the read-once hint (by the product's size; plan option csr_read_once forces it off / on -- these matrices are
far below the size, so every test that wants the hint forces it).  Everything behind the loads is as before, so the yardsticks
are those of test_gpu_tile_layout.py -- rows of at most 32 entries have the serial loop's bits, longer rows lie inside
parity.check_y's bound -- and, on every path, the bits of the same handle reading col_ind alone (plan option csr_col16 = 0).
The operand is a seeded random x, y is poisoned with NaN between guards before every product.

The matrices are tile_layout's, and one more ("distinct"): all columns different and all x different, so that an offset read
from any other slot of its tile gathers another number.
"""
import functools

import numpy as np
import pytest

import smvp_toolkit_amd as sm
from parity import check_guards, check_y, guarded_y
from tile_layout import KINDS, LONG_ROW, TILES, expected_flavor, matrix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                        # (a copy: the matrices are read-only)


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def check_product(m, y, what):
    """Short rows: the serial loop's bits.  Long rows: the oracle within the row-wise bound.  No NaN anywhere."""
    short = m["lens"] <= LONG_ROW
    bad = np.flatnonzero(y[short].view(np.int64) != m["serial"][short].view(np.int64))
    assert not len(bad), "%s: %d rows of at most %d entries differ from the serial sum (%d NaN); first row %d: %r against %r" % (
        what, len(bad), LONG_ROW, np.isnan(y[short][bad]).sum(), np.flatnonzero(short)[bad[0]], y[short][bad[0]], m["serial"][short][bad[0]])
    check_y(y, m["oracle"], m["scale"], m["lens"])


def product(torch, A, dx, rows):
    buf, dy = guarded_y(torch, rows)
    A.spmv(dx, dy)
    torch.cuda.synchronize()
    check_guards(buf, rows)
    return dy.cpu().numpy()


def stream_handle(m, tile, first_row=0):
    A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"], first_row=first_row)
    A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
    return A


@functools.lru_cache(maxsize=None)
def distinct(tile):
    """Two full tiles and a partial one (389 entries), rows of 1 ... 24 entries.  The columns are a seeded sample without
    repetition of [0, 60000): all of them distinct -- in every chunk of 64 * VPT entries, which is what counts -- and every tile
    narrow; the x values are all distinct and no value is 0.  An entry that takes the offset of another slot of its chunk then
    multiplies by another x, and its row's sum (left to right, one lane: every row is short) is the serial loop's no more."""
    import oracle_binding as ob
    rng = np.random.default_rng(1600 + tile)
    nnz, cols = 2 * tile + 389, 60000
    lens, left = [], nnz
    while left > 0:
        lens.append(min(int(rng.integers(1, 25)), left))
        left -= lens[-1]
    lens = np.array(lens, dtype=np.int64)
    rows = len(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col_ind = rng.choice(cols, size=nnz, replace=False).astype(np.int32)
    val = (rng.random(nnz) + 0.25) * rng.choice([-1.0, 1.0], size=nnz)
    x = 0.5 + rng.permutation(cols) / float(cols)
    # what the test relies on
    chunk = 64 * (tile // 256)
    for s in range(0, nnz, chunk):
        assert len(np.unique(col_ind[s:s + chunk])) == len(col_ind[s:s + chunk]), "columns repeat inside a chunk"
    assert len(np.unique(x)) == cols and len(np.unique(x[col_ind])) == nnz, "x values repeat"
    assert (val != 0.0).all() and lens.min() >= 1 and lens.max() <= 24
    assert all(int(col_ind[s:s + tile].max()) - int(col_ind[s:s + tile].min()) < 65536 for s in range(0, nnz, tile))
    serial = np.zeros(rows)
    for r in range(rows):
        acc = 0.0
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc += float(val[j]) * float(x[col_ind[j]])
        serial[r] = acc
    m = {"rows": rows, "cols": cols, "nnz": nnz, "lens": lens, "row_ptr": row_ptr, "col_ind": col_ind, "val": val, "x": x,
         "serial": serial, "oracle": ob.csr_spmv(row_ptr, col_ind, val, x),
         "scale": ob.csr_spmv(row_ptr, col_ind, np.abs(val), np.abs(x))}
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def both_column_forms(torch, m, tile, flavor, what, first_row=0, hint=0):
    """y through the 16-bit offsets, held to the yardsticks, and bit-equal to the same handle re-planned onto col_ind alone.
    hint: plan option csr_read_once for the first plan (matrices this small never get the hint by themselves)."""
    with sm.option("csr_read_once", hint):
        A = stream_handle(m, tile, first_row)
    try:
        assert A.describe()[0] == "csr_stream_owner<%d, %d, false>" % (tile // 256, flavor)
        dx = dev(torch, m["x"])
        y = product(torch, A, dx, m["rows"])
        check_product(m, y, what)
        with sm.option("csr_col16", 0):
            A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
        assert A.describe()[0] == "csr_stream_owner<%d, 0, false>" % (tile // 256)
        y32 = product(torch, A, dx, m["rows"])
        assert bits_equal(y32, y), "%s: 32-bit columns and 16-bit offsets give different bits" % what
    finally:
        A.close()
    return y


@pytest.mark.parametrize("hint", (0, 1))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_structure(torch, kind, tile, hint):
    """3 tiles + 517 entries, a wide tile beside narrow ones, all tiles wide, a giant row, exact tiles; without and with the
    read-once hint on the value and offset loads."""
    both_column_forms(torch, matrix(kind, tile), tile, expected_flavor(kind, tile), "%s, tiles of %d, hint %d" % (kind, tile, hint), hint=hint)


@pytest.mark.parametrize("hint", (0, 1))
@pytest.mark.parametrize("tile", TILES)
def test_distinct_columns_and_operands(torch, tile, hint):
    m = distinct(tile)
    y = both_column_forms(torch, m, tile, 5, "distinct, tiles of %d, hint %d" % (tile, hint), hint=hint)
    assert bits_equal(y, m["serial"]), "every row is short: y is the serial loop's, bit for bit"


def test_tile_size_changed_on_one_handle(torch):
    """1024 -> 2048 -> 1024 on one handle: the offsets are laid out again for every size; each product has the bits of a fresh
    handle at that size."""
    m = matrix("tail", 2048)
    dx = dev(torch, m["x"])
    A = sm.CsrMatrix(m["rows"], m["cols"], m["row_ptr"], m["col_ind"], m["val"])
    try:
        for tile in (1024, 2048, 1024):
            A.set_kernel(sm.CSR_KERNEL_STREAM, tile)
            assert A.describe()[0] == "csr_stream_owner<%d, 5, false>" % (tile // 256)
            y = product(torch, A, dx, m["rows"])
            check_product(m, y, "tail, re-planned to tiles of %d" % tile)
            F = stream_handle(m, tile)
            try:
                assert bits_equal(y, product(torch, F, dx, m["rows"])), "re-planned to %d: differs from a fresh handle" % tile
            finally:
                F.close()
    finally:
        A.close()


@pytest.mark.parametrize("tile", TILES)
def test_forward_and_backward_sweep(torch, tile):
    """csr_sweep_alternate = 1: the second product of a handle sweeps the tiles backward."""
    for m, what in ((matrix("tail", tile), "tail"), (distinct(tile), "distinct")):
        with sm.option("csr_sweep_alternate", 1):
            A = stream_handle(m, tile)
        try:
            dx = dev(torch, m["x"])
            fwd, back = product(torch, A, dx, m["rows"]), product(torch, A, dx, m["rows"])
        finally:
            A.close()
        check_product(m, fwd, "%s, tiles of %d, forward" % (what, tile))
        assert bits_equal(back, fwd), "%s, tiles of %d: the backward sweep differs from the forward one" % (what, tile)


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("kind", ("exact", "tail"))
def test_repeating_launch(torch, kind, tile):
    """Three products in one repeating launch (csr_stream_owner_repeat inlines the same body) on matrices with full tiles: y
    is the single launch's."""
    m = matrix(kind, tile)
    A = stream_handle(m, tile)
    try:
        want = product(torch, A, dev(torch, m["x"]), m["rows"])
    finally:
        A.close()
    check_product(m, want, "%s, tiles of %d" % (kind, tile))
    y, ms, st = sm.csr_compute(m["coo"], m["rows"], m["cols"], iters=3, x=m["x"], timing=sm.TIMING_DEVICE,
                               kernel=sm.CSR_KERNEL_STREAM, param=tile)
    info = sm.last_run_info()
    assert (info.timing, info.repeat_launches, info.graph_replays, info.repeat_gave_up) == (sm.TIMING_DEVICE, 1, 0, 0)
    assert len(ms) == 3 and np.isfinite(ms).all() and (ms > 0).all()
    assert bits_equal(y, want), "the repeating launch's y differs from the single launch's"


@pytest.mark.parametrize("tile", TILES)
def test_read_once_hint_forced_off_and_on(torch, tile):
    """Plan option csr_read_once: the single launches' val and col16 loads without and with the read-once hint (the default
    goes by the product's size, and these matrices are far below it): the same bits, forward and backward."""
    m = matrix("tail", tile)
    dx = dev(torch, m["x"])
    ys = []
    for hint in (0, 1):
        with sm.option("csr_read_once", hint), sm.option("csr_sweep_alternate", 1):
            A = stream_handle(m, tile)
        try:
            assert A.describe()[0] == "csr_stream_owner<%d, 5, false>" % (tile // 256)
            ys += [product(torch, A, dx, m["rows"]), product(torch, A, dx, m["rows"])]
        finally:
            A.close()
    check_product(m, ys[0], "tail, tiles of %d, no hint" % tile)
    for i, y in enumerate(ys[1:]):
        assert bits_equal(y, ys[0]), "tail, tiles of %d: product %d (hint %d) differs from the first" % (tile, i + 1, (i + 1) // 2)


@pytest.mark.parametrize("tile", TILES)
def test_row_block_handle(torch, tile):
    """A row block of a larger matrix (first_row > 0) whose columns lie far beyond the block's own rows."""
    m = distinct(tile)
    assert int(m["col_ind"].max()) > 4000 + m["rows"]
    y = both_column_forms(torch, m, tile, 5, "distinct as a row block, tiles of %d" % tile, first_row=4000)
    assert bits_equal(y, m["serial"])
